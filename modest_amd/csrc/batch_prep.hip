// Training-batch preparation: what OpenPCDet's DataBaseSampler (gt_sampling), DataAugmentor (random_world_flip /
// _rotation / _scaling) and DataProcessor (mask_points_and_boxes_outside_range, sample_points, shuffle_points) do to a
// sample between the raw scan and the model's first module, for a whole batch, hand-written for gfx950.  Two entry points
// (include/modest_hip.h, "a39"): modest_batch_prep_stage1 (blocking: the call's one synchronise) and
// modest_batch_prep_order (enqueue only).
//
// Arithmetic (tests/batch_prep_seq.py restates it in numpy; the build has -ffp-contract=off, every fused product is written):
//   collision   a candidate is kept iff iou_bev (csrc/iou_bev.h: the host's cosf / sinf of the headings, handed in with the
//               boxes; atan2 as the double function rounded once) == 0 against every gt, every kept candidate of an earlier
//               group and every other candidate of its own group
//   object row  xyz = row + box centre (float32); with a road plane z = float(double(z) - mv_height)
//   scene row   dropped iff inside a kept candidate's box (lowered z, extents + REMOVE_EXTRA_WIDTH in float32): the predicate of
//               roiaware_pool3d.cpp:121-168 with the host's cosf(-rz) / sinf(-rz), decided in float32 against f32_down / f32_up
//               of the double bounds (csrc/box_predicate.h)
//   flip        along x: y = -y, heading = -heading; along y: x = -x, heading = -(heading + float(pi))
//   rotation    x' = fmaf(y, -s, x c), y' = fmaf(y, c, x s) with the host's float32 c, s; heading += float(angle)
//   scaling     xyz and box columns 0-5 times float(scale)
//   heading     v - floorf(v / float(2 pi) + 0.5f) float(2 pi)
//   corners     (+-0.5 dx, +-0.5 dy, +-0.5 dz) turned by the heading (cos / sin as the double function rounded once, the same
//               fmaf forms) plus the centre; a corner counts when its three coordinates are inside the range, ends included
//   range       x0 <= x <= x1 and y0 <= y <= y1 in float32 (false for NaN);  near: sqrtf((x x + y y) + z z) < 40
// Nothing here adds into memory: counts are ballots, offsets are scans, so no result depends on an order of atomics, and no
// workgroup waits for another (three launches order the count pass, the scan and the write pass).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "iou_bev.h"
#include "box_predicate.h"

namespace {

constexpr int BP_MAX_BOXES = 512;    // gts + candidates of a sample: what the box workgroup stages in LDS
constexpr int BP_TILE = 1024;        // rows of a points workgroup; a tile never spans two samples
constexpr int BP_BOX_T = 256;        // lanes of a box workgroup: four wavefronts, a polygon buffer each
constexpr int BP_BOX_COLS = 12;      // box7, cosf h, sinf h, cosf(-h), sinf(-h), class index
constexpr int BP_SAMP_COLS = 10;     // int64 per sample, below
constexpr int BP_MAX_OPS = 4;
constexpr int BP_TABLE_WORDS = 6;    // points kept, far points, boxes kept, candidates kept, candidates dropped, 0
constexpr int BP_MAX_BATCH = 65535;
constexpr int BP_GATHER_T = 256;
enum { S_VROW = 0, S_NOBJ, S_SCENE, S_NSCENE, S_BOX, S_NGT, S_NCAND, S_CAND, S_TILE, S_SPARE };
enum { OP_FLIP_X = 1, OP_FLIP_Y = 2, OP_ROTATION = 3, OP_SCALING = 4 };
enum { X_FLIP_X = 0, X_FLIP_Y, X_COS, X_SIN, X_ANGLE, X_SCALE, X_COLS = 8 };

struct BpParams {
    int B, F, n_tiles;
    const float *scene, *db, *boxes, *xf;
    const int64_t *samp, *cand;
    const double *cand_f64;
    const int32_t *cand_grp;
    int nops, ops[BP_MAX_OPS];
    float range[6], extra[3];
    int road_plane, want_near, remove_outside, min_corners;
    int32_t *valid;
    uint8_t *flags;
    int32_t *tile_cnt;     // (n_tiles, 2): kept, near; after the scan their exclusive sums within the sample
    int32_t *samp_cnt;     // (B, 2): kept, near
    int64_t *out_begin;    // (B + 1)
    float *points;
    int32_t *lists;
    float *gt_out;
    int gcap;
    int32_t *table;
};

struct BpLayout {
    size_t flags, tile_cnt, samp_cnt, out_begin, total;
};
BpLayout bp_layout(int64_t n_rows, int b) {
    BpLayout l;
    const size_t bb = (size_t)(b > 0 ? b : 1);
    l.flags = 0;
    l.tile_cnt = l.flags + arena_sz((size_t)n_rows);
    l.samp_cnt = l.tile_cnt + arena_sz(8 * ((size_t)n_rows / BP_TILE + bb + 1));
    l.out_begin = l.samp_cnt + arena_sz(8 * bb);
    l.total = l.out_begin + arena_sz(8 * (bb + 1));
    return l;
}

// rank of this lane among the workgroup's lanes with `keep`, and their number; every lane calls it.  s_w: NW words.
template <int NW>
__device__ __forceinline__ int block_rank(bool keep, int *s_w, int &total) {
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int before = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int c = s_w[k];
        if (k < w) off += c;
        total += c;
    }
    __syncthreads();
    return off + before;
}

__device__ __forceinline__ void bp_augment_xyz(const BpParams &p, const float *__restrict__ xf, float &x, float &y, float &z) {
    for (int k = 0; k < p.nops; ++k) {
        const int op = p.ops[k];
        if (op == OP_FLIP_X) {
            if (xf[X_FLIP_X] != 0.f) y = -y;
        } else if (op == OP_FLIP_Y) {
            if (xf[X_FLIP_Y] != 0.f) x = -x;
        } else if (op == OP_ROTATION) {
            const float c = xf[X_COS], s = xf[X_SIN];
            const float nx = fmaf(y, -s, x * c), ny = fmaf(y, c, x * s);
            x = nx;
            y = ny;
        } else {
            const float sc = xf[X_SCALE];
            x = x * sc;
            y = y * sc;
            z = z * sc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- boxes
// One workgroup per sample: which candidates stay, then the sample's box list through the augmentors and the masks.
__global__ __launch_bounds__(BP_BOX_T) void bp_boxes(BpParams p) {
    __shared__ PolyLds L[BP_BOX_T / NMS_TPB];
    __shared__ float s_box[BP_MAX_BOXES][BP_BOX_COLS];
    __shared__ float s_out[BP_MAX_BOXES][8];
    __shared__ int s_grp[BP_MAX_BOXES], s_hit[BP_MAX_BOXES], s_valid[BP_MAX_BOXES];
    __shared__ int s_w[BP_BOX_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t *sm = p.samp + (size_t)b * BP_SAMP_COLS;
    const int n_gt = (int)sm[S_NGT], n_cand = (int)sm[S_NCAND];
    const int64_t box0 = sm[S_BOX], cand0 = sm[S_CAND];
    const int n = n_gt + n_cand;
    if (n_gt < 0 || n_cand < 0 || n > BP_MAX_BOXES) return;   // refused on the host; never reached
    for (int i = tid; i < n * BP_BOX_COLS; i += BP_BOX_T) s_box[i / BP_BOX_COLS][i % BP_BOX_COLS] = p.boxes[box0 * BP_BOX_COLS + i];
    for (int i = tid; i < n_cand; i += BP_BOX_T) {
        s_grp[i] = p.cand_grp[cand0 + i];
        s_hit[i] = 0;
        s_valid[i] = 0;
    }
    __syncthreads();
    PolyLds &Lw = L[tid >> 6];
    int g0 = 0;
    while (g0 < n_cand) {   // the class groups in order: a run of equal group numbers
        int g1 = g0 + 1;
        while (g1 < n_cand && s_grp[g1] == s_grp[g0]) ++g1;
        const int others = n_gt + g1;
        const int pairs = (g1 - g0) * others;
        for (int q = tid; q < pairs; q += BP_BOX_T) {
            const int i = g0 + q / others, j = q % others;
            if (j >= n_gt) {
                const int jc = j - n_gt;
                if (jc == i) continue;                      // iou2's diagonal is set to zero
                if (jc < g0 && !s_valid[jc]) continue;      // a dropped candidate blocks nobody
            }
            float a[7], c[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                a[k] = s_box[n_gt + i][k];
                c[k] = s_box[j][k];
            }
            const float4 ta = make_float4(s_box[n_gt + i][7], s_box[n_gt + i][8], s_box[n_gt + i][9], s_box[n_gt + i][10]);
            const float4 tc = make_float4(s_box[j][7], s_box[j][8], s_box[j][9], s_box[j][10]);
            const float v = iou_bev(a, c, ta, tc, Lw);
            if (!(v == 0.f)) s_hit[i] = 1;                  // every writer stores the same word
        }
        __syncthreads();
        for (int i = g0 + tid; i < g1; i += BP_BOX_T) s_valid[i] = s_hit[i] ? 0 : 1;
        __syncthreads();
        g0 = g1;
    }
    for (int i = tid; i < n_cand; i += BP_BOX_T) p.valid[cand0 + i] = s_valid[i];

    // the box list: gts in order, then the kept candidates in candidate order with their lowered z
    const float *xf = p.xf + (size_t)b * X_COLS;
    const float PI_F = 3.14159274101257324f, TWO_PI_F = 6.28318548202514648f;
    int kept_total = 0;
    for (int k0 = 0; k0 < n; k0 += BP_BOX_T) {
        const int k = k0 + tid;
        bool keep = false;
        float x = 0.f, y = 0.f, z = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, h = 0.f, cls = 0.f;
        if (k < n) {
            const bool live = k < n_gt || s_valid[k - n_gt];
            x = s_box[k][0]; y = s_box[k][1]; z = s_box[k][2];
            dx = s_box[k][3]; dy = s_box[k][4]; dz = s_box[k][5]; h = s_box[k][6];
            cls = s_box[k][11];
            if (k >= n_gt && p.road_plane) z = (float)p.cand_f64[(cand0 + (k - n_gt)) * 2 + 1];
            for (int q = 0; q < p.nops; ++q) {
                const int op = p.ops[q];
                if (op == OP_FLIP_X) {
                    if (xf[X_FLIP_X] != 0.f) { y = -y; h = -h; }
                } else if (op == OP_FLIP_Y) {
                    if (xf[X_FLIP_Y] != 0.f) { x = -x; h = -(h + PI_F); }
                } else if (op == OP_ROTATION) {
                    const float c = xf[X_COS], s = xf[X_SIN];
                    const float nx = fmaf(y, -s, x * c), ny = fmaf(y, c, x * s);
                    x = nx;
                    y = ny;
                    h = h + xf[X_ANGLE];
                } else {
                    const float sc = xf[X_SCALE];
                    x = x * sc; y = y * sc; z = z * sc;
                    dx = dx * sc; dy = dy * sc; dz = dz * sc;
                }
            }
            h = h - floorf(h / TWO_PI_F + 0.5f) * TWO_PI_F;
            keep = live && cls > 0.f;
            if (keep && p.remove_outside) {
                const float c = modest::cos_f32(h), s = modest::sin_f32(h);
                int inside = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float lx = dx * ((q & 1) ? -0.5f : 0.5f), ly = dy * ((q & 2) ? -0.5f : 0.5f);
                    const float lz = dz * ((q & 4) ? -0.5f : 0.5f);
                    const float cx = fmaf(ly, -s, lx * c) + x, cy = fmaf(ly, c, lx * s) + y, cz = lz + z;
                    inside += (cx >= p.range[0] && cx <= p.range[3] && cy >= p.range[1] && cy <= p.range[4] &&
                               cz >= p.range[2] && cz <= p.range[5]) ? 1 : 0;
                }
                keep = inside >= p.min_corners;
            }
        }
        int total;
        const int rank = block_rank<BP_BOX_T / 64>(keep, s_w, total);
        if (keep) {
            float *o = s_out[kept_total + rank];
            o[0] = x; o[1] = y; o[2] = z; o[3] = dx; o[4] = dy; o[5] = dz; o[6] = h; o[7] = cls;
        }
        kept_total += total;
    }
    __syncthreads();
    float *out = p.gt_out + (size_t)b * p.gcap * 8;
    for (int i = tid; i < p.gcap * 8; i += BP_BOX_T) out[i] = i < kept_total * 8 ? s_out[i / 8][i % 8] : 0.f;
    // the candidates kept: a ballot count, one writer
    int ck = 0;
    for (int i0 = 0; i0 < n_cand; i0 += BP_BOX_T) {
        int total;
        block_rank<BP_BOX_T / 64>(i0 + tid < n_cand && s_valid[i0 + tid], s_w, total);
        ck += total;
    }
    if (tid == 0) {
        int32_t *t = p.table + (size_t)b * BP_TABLE_WORDS;
        t[2] = kept_total;
        t[3] = ck;
        t[4] = n_cand - ck;
        t[5] = 0;
    }
}

// --------------------------------------------------------------------------------------------------------------- points
struct BpTile {
    int b;
    int row0;        // first row of the tile within the sample's virtual concatenation
    int nrows;       // rows of the sample: object rows of all candidates, then the scene
    int nobj;
};
__device__ __forceinline__ BpTile bp_tile(const BpParams &p, int t) {
    int lo = 0, hi = p.B - 1;    // the last sample whose first tile is <= t (samples without rows have no tile)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.samp[(size_t)mid * BP_SAMP_COLS + S_TILE] <= t) lo = mid; else hi = mid - 1;
    }
    const int64_t *sm = p.samp + (size_t)lo * BP_SAMP_COLS;
    BpTile r;
    r.b = lo;
    r.row0 = (int)((t - sm[S_TILE]) * BP_TILE);
    r.nobj = (int)sm[S_NOBJ];
    r.nrows = r.nobj + (int)sm[S_NSCENE];
    return r;
}

// the row's source and its coordinates ahead of the augmentors; false: an object row of a dropped candidate.
// s_cobj: first object row of each candidate of the sample, and nobj behind the last
__device__ __forceinline__ bool bp_row(const BpParams &p, const int64_t *sm, const BpTile &T, int r, const int *s_cobj, int n_cand,
                                       const int *s_cvalid, const float *__restrict__ &src, float &x, float &y, float &z, int &cand) {
    if (r < T.nobj) {
        int lo = 0, hi = n_cand - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_cobj[mid] <= r) lo = mid; else hi = mid - 1;
        }
        cand = lo;
        const int64_t c = sm[S_CAND] + lo;
        src = p.db + (size_t)(p.cand[c * 3 + 0] + (r - s_cobj[lo])) * p.F;
        if (!s_cvalid[lo]) return false;
        const float *bx = p.boxes + (size_t)(sm[S_BOX] + sm[S_NGT] + lo) * BP_BOX_COLS;
        x = src[0] + bx[0];
        y = src[1] + bx[1];
        z = src[2] + bx[2];
        if (p.road_plane) z = (float)((double)z - p.cand_f64[c * 2 + 0]);
        return true;
    }
    cand = -1;
    src = p.scene + (size_t)(sm[S_SCENE] + (r - T.nobj)) * p.F;
    x = src[0];
    y = src[1];
    z = src[2];
    return true;
}

__global__ __launch_bounds__(BP_TILE) void bp_points_count(BpParams p) {
    __shared__ float s_term[BP_MAX_BOXES][8];     // cx cy cz cosa sina tz tx ty of the candidates' enlarged boxes
    __shared__ int s_cobj[BP_MAX_BOXES + 1], s_cvalid[BP_MAX_BOXES];
    __shared__ int s_w[BP_TILE / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const BpTile T = bp_tile(p, t);
    const int64_t *sm = p.samp + (size_t)T.b * BP_SAMP_COLS;
    const int n_cand = min((int)sm[S_NCAND], BP_MAX_BOXES);
    for (int j = tid; j < n_cand; j += BP_TILE) {
        const int64_t c = sm[S_CAND] + j;
        s_cobj[j] = (int)p.cand[c * 3 + 2];
        const int v = p.valid[c];
        s_cvalid[j] = v;
        const float *bx = p.boxes + (size_t)(sm[S_BOX] + sm[S_NGT] + j) * BP_BOX_COLS;
        const float dx = bx[3] + p.extra[0], dy = bx[4] + p.extra[1], dz = bx[5] + p.extra[2];
        s_term[j][0] = bx[0];
        s_term[j][1] = bx[1];
        s_term[j][2] = p.road_plane ? (float)p.cand_f64[c * 2 + 1] : bx[2];
        s_term[j][3] = bx[9];
        s_term[j][4] = bx[10];
        s_term[j][5] = f32_down((double)dz / 2.0);
        s_term[j][6] = f32_up((double)dx / 2.0 + (double)1e-2f);
        s_term[j][7] = f32_up((double)dy / 2.0 + (double)1e-2f);
    }
    if (tid == 0) s_cobj[n_cand] = T.nobj;
    __syncthreads();
    const int r = T.row0 + tid;
    bool keep = false, near = false;
    if (r < T.nrows) {
        const float *src;
        float x, y, z;
        int cand;
        keep = bp_row(p, sm, T, r, s_cobj, n_cand, s_cvalid, src, x, y, z, cand);
        if (keep && cand < 0) {
            for (int j = 0; j < n_cand; ++j) {
                if (!s_cvalid[j]) continue;
                if (pt_in_box(x, y, z, s_term[j][0], s_term[j][1], s_term[j][2], s_term[j][3], s_term[j][4], -s_term[j][4],
                              s_term[j][5], s_term[j][6], s_term[j][7])) {
                    keep = false;
                    break;
                }
            }
        }
        if (keep) {
            bp_augment_xyz(p, p.xf + (size_t)T.b * X_COLS, x, y, z);
            keep = x >= p.range[0] && x <= p.range[3] && y >= p.range[1] && y <= p.range[4];
            near = keep && sqrtf((x * x + y * y) + z * z) < 40.f;
        }
        p.flags[sm[S_VROW] + r] = (uint8_t)((keep ? 1 : 0) | (near ? 2 : 0));
    }
    int kept, nnear;
    block_rank<BP_TILE / 64>(keep, s_w, kept);
    block_rank<BP_TILE / 64>(near, s_w, nnear);
    if (tid == 0) {
        p.tile_cnt[2 * (size_t)t] = kept;
        p.tile_cnt[2 * (size_t)t + 1] = nnear;
    }
}

// one workgroup: the tile counts become exclusive sums within their sample, the samples' totals their first output rows
__global__ __launch_bounds__(BP_TILE) void bp_scan(BpParams p) {
    __shared__ long long s_part[BP_TILE];
    __shared__ long long s_carry;
    const int tid = threadIdx.x;
    for (int b = tid; b < p.B; b += BP_TILE) {
        const int64_t *sm = p.samp + (size_t)b * BP_SAMP_COLS;
        const int64_t t0 = sm[S_TILE];
        const int64_t nt = (sm[S_NOBJ] + sm[S_NSCENE] + BP_TILE - 1) / BP_TILE;
        int kept = 0, nnear = 0;
        for (int64_t t = t0; t < t0 + nt; ++t) {
            const int k = p.tile_cnt[2 * t], m = p.tile_cnt[2 * t + 1];
            p.tile_cnt[2 * t] = kept;
            p.tile_cnt[2 * t + 1] = nnear;
            kept += k;
            nnear += m;
        }
        p.samp_cnt[2 * b] = kept;
        p.samp_cnt[2 * b + 1] = nnear;
        int32_t *tab = p.table + (size_t)b * BP_TABLE_WORDS;
        tab[0] = kept;
        tab[1] = kept - nnear;
    }
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < p.B; b0 += BP_TILE) {    // exclusive sums of the samples' totals, 1024 samples a round
        const int b = b0 + tid;
        const long long own = b < p.B ? p.samp_cnt[2 * b] : 0;
        s_part[tid] = own;
        __syncthreads();
        for (int o = 1; o < BP_TILE; o <<= 1) {
            const long long add = tid >= o ? s_part[tid - o] : 0;
            __syncthreads();
            s_part[tid] += add;
            __syncthreads();
        }
        const long long base = s_carry;
        if (b < p.B) p.out_begin[b] = base + s_part[tid] - own;
        __syncthreads();
        if (tid == BP_TILE - 1) s_carry = base + s_part[tid];
        __syncthreads();
    }
    if (tid == 0) p.out_begin[p.B] = s_carry;
}

__global__ __launch_bounds__(BP_TILE) void bp_points_write(BpParams p) {
    __shared__ int s_cobj[BP_MAX_BOXES + 1], s_cvalid[BP_MAX_BOXES];
    __shared__ int s_w[BP_TILE / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const BpTile T = bp_tile(p, t);
    const int64_t *sm = p.samp + (size_t)T.b * BP_SAMP_COLS;
    const int n_cand = min((int)sm[S_NCAND], BP_MAX_BOXES);
    for (int j = tid; j < n_cand; j += BP_TILE) {
        s_cobj[j] = (int)p.cand[(sm[S_CAND] + j) * 3 + 2];
        s_cvalid[j] = p.valid[sm[S_CAND] + j];
    }
    if (tid == 0) s_cobj[n_cand] = T.nobj;
    __syncthreads();
    const int r = T.row0 + tid;
    const int fl = r < T.nrows ? p.flags[sm[S_VROW] + r] : 0;
    const bool keep = fl & 1, near = (fl & 2) != 0;
    int tot;
    const int rk = block_rank<BP_TILE / 64>(keep, s_w, tot);
    const int rn = block_rank<BP_TILE / 64>(near, s_w, tot);
    if (!keep) return;
    const int tk = p.tile_cnt[2 * (size_t)t], tn = p.tile_cnt[2 * (size_t)t + 1];
    const int64_t base = p.out_begin[T.b];
    const int pos = tk + rk;                         // the row's place among the sample's survivors
    const float *src;
    float x, y, z;
    int cand;
    bp_row(p, sm, T, r, s_cobj, n_cand, s_cvalid, src, x, y, z, cand);
    bp_augment_xyz(p, p.xf + (size_t)T.b * X_COLS, x, y, z);
    float *o = p.points + (size_t)(base + pos) * (p.F + 1);
    o[0] = (float)T.b;
    o[1] = x;
    o[2] = y;
    o[3] = z;
    for (int k = 3; k < p.F; ++k) o[1 + k] = src[k];
    if (p.want_near) {
        if (near) p.lists[base + tn + rn] = pos;
        else p.lists[base + p.samp_cnt[2 * T.b + 1] + (tk - tn) + (rk - rn)] = pos;
    }
}

// ------------------------------------------------------------------------------------------------------------- stage 2
struct BpOrder {
    int B, F;
    int64_t n_out;
    const float *points;
    const int32_t *lists, *picks, *samp_cnt;
    const int32_t *perm;      // shuffle_points ahead of sample_points: the survivors' order, per sample (NULL: their own order)
    int32_t *lists2;          // ... and the near / far lists of that order, written by bp_shuffled_lists
    const int64_t *out_begin;
    float *out;
};

// shuffle_points ahead of sample_points: the near list and the far list of a sample whose survivors stand in the order `perm`
// (place i holds survivor perm[i]).  One workgroup per sample walks the places 1024 at a time; a survivor is near iff it is in
// the sample's near list, which is ascending (binary search); ranks are ballots, the running sums are the workgroup's own.
__global__ __launch_bounds__(BP_TILE) void bp_shuffled_lists(BpOrder p) {
    __shared__ int s_w[BP_TILE / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int kept = p.samp_cnt[2 * b], nnear = p.samp_cnt[2 * b + 1];
    const int64_t base = p.out_begin[b];
    const int32_t *nl = p.lists + base;
    int cn = 0, cf = 0;
    for (int i0 = 0; i0 < kept; i0 += BP_TILE) {
        const int i = i0 + tid;
        bool live = i < kept, near = false;
        if (live) {
            const int s = p.perm[base + i];
            live = s >= 0 && s < kept;      // refused on the host; never false here
            int lo = 0, hi = nnear;         // the first entry >= s
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (nl[mid] < s) lo = mid + 1; else hi = mid;
            }
            near = live && lo < nnear && nl[lo] == s;
        }
        int tn, tf;
        const int rn = block_rank<BP_TILE / 64>(near, s_w, tn);
        const int rf = block_rank<BP_TILE / 64>(live && !near, s_w, tf);
        if (near) p.lists2[base + cn + rn] = i;
        else if (live) p.lists2[base + nnear + cf + rf] = i;
        cn += tn;
        cf += tf;
    }
}
__global__ __launch_bounds__(BP_GATHER_T) void bp_gather(BpOrder p) {
    const int64_t i = (int64_t)blockIdx.x * BP_GATHER_T + threadIdx.x;
    if (i >= p.n_out) return;
    const int w = p.picks[2 * i], pos = p.picks[2 * i + 1];
    const int b = w >> 2, list = w & 3;
    float *o = p.out + (size_t)i * (p.F + 1);
    bool ok = b >= 0 && b < p.B && pos >= 0 && list <= 2;
    int64_t srow = 0;
    if (ok) {
        const int kept = p.samp_cnt[2 * b], nnear = p.samp_cnt[2 * b + 1];
        const int64_t base = p.out_begin[b];
        int place = pos;                // among the sample's survivors, in their own order or in perm's
        if (list == 0) {
            ok = pos < kept;
        } else {
            ok = list == 1 ? pos < nnear : pos < kept - nnear;
            if (ok) place = (p.perm ? p.lists2 : p.lists)[base + (list == 2 ? nnear : 0) + pos];
        }
        if (ok && p.perm) {
            place = p.perm[base + place];
            ok = place >= 0 && place < kept;
        }
        srow = base + place;
    }
    if (!ok) {          // refused on the host (ops.batch_prep_order checks the picks against the table); never reached
        o[0] = -1.f;
        for (int k = 0; k < p.F; ++k) o[1 + k] = 0.f;
        return;
    }
    const float *s = p.points + (size_t)srow * (p.F + 1);
    for (int k = 0; k <= p.F; ++k) o[k] = s[k];
}

int64_t bp_total(int64_t n_rows, int b) { return (int64_t)bp_layout(n_rows, b).total; }

}  // namespace

extern "C" int modest_batch_prep_max_boxes(void) { return BP_MAX_BOXES; }

extern "C" int modest_batch_prep_tile(void) { return BP_TILE; }

extern "C" int modest_batch_prep_table_words(void) { return BP_TABLE_WORDS; }

extern "C" int64_t modest_batch_prep_workspace_bytes(int64_t n_rows, int batch_size) {
    if (n_rows < 0 || n_rows > 2147483647LL || batch_size < 0 || batch_size > BP_MAX_BATCH) {
        modest_set_error("modest_batch_prep_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 and 0 <= batch_size <= 65535");
        return MODEST_ERR_ARG;
    }
    return bp_total(n_rows, batch_size);
}

extern "C" int modest_batch_prep_stage1(int batch_size, int features, int64_t n_scene_rows, const float *scene_dev,
                                        int64_t n_db_rows, const float *db_dev, const int64_t *samp_host, const int64_t *samp_dev,
                                        int64_t n_boxes, const float *boxes_dev, int64_t n_cand, const int64_t *cand_host,
                                        const int64_t *cand_dev, const double *cand_f64_dev, const int32_t *cand_group_dev,
                                        const float *xf_dev, int n_ops, const int32_t *ops_host, const float *range_host,
                                        const float *extra_width_host, int road_plane, int want_near, int remove_outside_boxes,
                                        int min_num_corners, int64_t n_rows, int32_t *valid_dev, float *points_dev,
                                        int32_t *lists_dev, float *gt_boxes_dev, int gt_capacity, int32_t *table_pinned_host,
                                        void *workspace_dev, int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= BP_MAX_BATCH, "a batch of at most 65535 samples");
    MODEST_REQUIRE(features >= 4 && features <= 8, "4 to 8 point features");
    MODEST_REQUIRE(n_ops >= 0 && n_ops <= BP_MAX_OPS && (n_ops == 0 || ops_host), "at most 4 augmentor steps");
    MODEST_REQUIRE(n_scene_rows >= 0 && n_db_rows >= 0 && n_boxes >= 0 && n_cand >= 0 && n_rows >= 0 && gt_capacity >= 0,
                   "negative count");
    MODEST_REQUIRE(n_rows <= 2147483647LL && n_scene_rows <= 2147483647LL && n_db_rows <= 2147483647LL,
                   "at most 2^31 - 1 rows in a call");
    MODEST_REQUIRE(n_boxes <= (int64_t)BP_MAX_BATCH * BP_MAX_BOXES && n_cand <= n_boxes, "more boxes than the samples may hold");
    if (batch_size == 0) return MODEST_OK;
    MODEST_REQUIRE(samp_host && (n_cand == 0 || cand_host) && range_host && extra_width_host, "NULL host table");
    for (int k = 0; k < n_ops; ++k)
        MODEST_REQUIRE(ops_host[k] >= OP_FLIP_X && ops_host[k] <= OP_SCALING, "augmentor steps are 1 (flip x), 2 (flip y), 3 (rotation), 4 (scaling)");
    // every index a kernel forms is checked here, against the host's copy of the tables
    int64_t vrow = 0, box = 0, cand = 0, tile = 0;
    for (int b = 0; b < batch_size; ++b) {
        const int64_t *sm = samp_host + (size_t)b * BP_SAMP_COLS;
        MODEST_REQUIRE(sm[S_NGT] >= 0 && sm[S_NCAND] >= 0 && sm[S_NGT] + sm[S_NCAND] <= BP_MAX_BOXES,
                       "gts plus candidates of a sample: at most modest_batch_prep_max_boxes() = 512");
        MODEST_REQUIRE(sm[S_NGT] + sm[S_NCAND] <= gt_capacity, "gt_capacity below a sample's gts plus candidates");
        MODEST_REQUIRE(sm[S_VROW] == vrow && sm[S_BOX] == box && sm[S_CAND] == cand && sm[S_TILE] == tile,
                       "sample table: rows, boxes, candidates and tiles must follow one another");
        MODEST_REQUIRE(sm[S_NOBJ] >= 0 && sm[S_NSCENE] >= 0 && sm[S_SCENE] >= 0 && sm[S_SCENE] + sm[S_NSCENE] <= n_scene_rows,
                       "sample table: scene rows outside the scene points");
        int64_t obj = 0;
        for (int64_t j = 0; j < sm[S_NCAND]; ++j) {
            const int64_t *c = cand_host + (size_t)(cand + j) * 3;
            MODEST_REQUIRE(c[0] >= 0 && c[1] >= 0 && c[0] + c[1] <= n_db_rows, "candidate table: object rows outside the database points");
            MODEST_REQUIRE(c[2] == obj, "candidate table: object rows must follow one another");
            obj += c[1];
        }
        MODEST_REQUIRE(obj == sm[S_NOBJ], "sample table: object rows differ from the candidates' sum");
        MODEST_REQUIRE(obj + sm[S_NSCENE] <= 2147483647LL, "at most 2^31 - 1 rows in a sample");
        vrow += obj + sm[S_NSCENE];
        box += sm[S_NGT] + sm[S_NCAND];
        cand += sm[S_NCAND];
        tile += (obj + sm[S_NSCENE] + BP_TILE - 1) / BP_TILE;
    }
    MODEST_REQUIRE(vrow == n_rows && box == n_boxes && cand == n_cand, "sample table: totals differ from n_rows, n_boxes, n_cand");
    MODEST_REQUIRE(tile <= GRID_MAX, "too many tiles");
    MODEST_REQUIRE(samp_dev && xf_dev && table_pinned_host, "NULL table");
    MODEST_REQUIRE(n_cand == 0 || (cand_dev && cand_f64_dev && cand_group_dev && valid_dev), "NULL candidate table");
    MODEST_REQUIRE(n_boxes == 0 || boxes_dev, "NULL boxes");
    MODEST_REQUIRE((n_scene_rows == 0 || scene_dev) && (n_db_rows == 0 || db_dev), "NULL points");
    MODEST_REQUIRE(n_rows == 0 || (points_dev && lists_dev), "NULL output");
    MODEST_REQUIRE(gt_capacity == 0 || gt_boxes_dev, "NULL gt_boxes output");
    const BpLayout lay = bp_layout(n_rows, batch_size);
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)lay.total, "workspace smaller than modest_batch_prep_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    BpParams p;
    p.B = batch_size;
    p.F = features;
    p.n_tiles = (int)tile;
    p.scene = scene_dev;
    p.db = db_dev;
    p.boxes = boxes_dev;
    p.xf = xf_dev;
    p.samp = samp_dev;
    p.cand = cand_dev;
    p.cand_f64 = cand_f64_dev;
    p.cand_grp = cand_group_dev;
    p.nops = n_ops;
    for (int k = 0; k < BP_MAX_OPS; ++k) p.ops[k] = k < n_ops ? ops_host[k] : 0;
    for (int k = 0; k < 6; ++k) p.range[k] = range_host[k];
    for (int k = 0; k < 3; ++k) p.extra[k] = extra_width_host[k];
    p.road_plane = road_plane ? 1 : 0;
    p.want_near = want_near ? 1 : 0;
    p.remove_outside = remove_outside_boxes ? 1 : 0;
    p.min_corners = min_num_corners;
    p.valid = valid_dev;
    p.flags = reinterpret_cast<uint8_t *>(ws + lay.flags);
    p.tile_cnt = reinterpret_cast<int32_t *>(ws + lay.tile_cnt);
    p.samp_cnt = reinterpret_cast<int32_t *>(ws + lay.samp_cnt);
    p.out_begin = reinterpret_cast<int64_t *>(ws + lay.out_begin);
    p.points = points_dev;
    p.lists = lists_dev;
    p.gt_out = gt_boxes_dev;
    p.gcap = gt_capacity;
    p.table = table_pinned_host;
    bp_boxes<<<(unsigned)batch_size, BP_BOX_T, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    if (tile > 0) {
        bp_points_count<<<(unsigned)tile, BP_TILE, 0, st>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    bp_scan<<<1, BP_TILE, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    if (tile > 0) {
        bp_points_write<<<(unsigned)tile, BP_TILE, 0, st>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    MODEST_HIP_CHECK(hipStreamSynchronize(st));
    return MODEST_OK;
}

extern "C" int modest_batch_prep_order(int batch_size, int features, int64_t n_rows, const float *points_dev,
                                       const int32_t *lists_dev, const void *workspace_dev, int64_t workspace_bytes,
                                       int64_t n_out, const int32_t *picks_dev, const int32_t *perm_dev, int32_t *lists2_dev,
                                       float *out_dev, void *stream) {
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= BP_MAX_BATCH, "a batch of at most 65535 samples");
    MODEST_REQUIRE(features >= 4 && features <= 8, "4 to 8 point features");
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= 2147483647LL && n_out >= 0 && n_out <= 2147483647LL, "at most 2^31 - 1 rows in a call");
    if (n_out == 0 || batch_size == 0) return MODEST_OK;
    MODEST_REQUIRE(points_dev && lists_dev && picks_dev && out_dev, "NULL buffer");
    MODEST_REQUIRE(perm_dev == nullptr || lists2_dev, "a permutation needs the buffer of its lists");
    const BpLayout lay = bp_layout(n_rows, batch_size);
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)lay.total, "workspace smaller than modest_batch_prep_workspace_bytes");
    const char *ws = static_cast<const char *>(workspace_dev);
    BpOrder p;
    p.B = batch_size;
    p.F = features;
    p.n_out = n_out;
    p.points = points_dev;
    p.lists = lists_dev;
    p.picks = picks_dev;
    p.samp_cnt = reinterpret_cast<const int32_t *>(ws + lay.samp_cnt);
    p.out_begin = reinterpret_cast<const int64_t *>(ws + lay.out_begin);
    p.out = out_dev;
    p.perm = perm_dev;
    p.lists2 = lists2_dev;
    if (perm_dev) {
        bp_shuffled_lists<<<(unsigned)batch_size, BP_TILE, 0, as_stream(stream)>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    bp_gather<<<(unsigned)((n_out + BP_GATHER_T - 1) / BP_GATHER_T), BP_GATHER_T, 0, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
