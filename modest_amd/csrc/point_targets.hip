// Point-head target assignment of OpenPCDet's point heads (PointHeadTemplate.assign_stack_targets,
// pcdet/models/dense_heads/point_head_template.py:49-129, with set_ignore_flag=True, use_ball_constraint=False, what
// PointHeadBox, PointHeadSimple and PointIntraPartOffsetHead pass), hand-written for gfx950.  One entry point
// (include/modest_hip.h, "a30") assigns a whole stacked batch: enqueue only, no synchronise, no context, no device
// allocation, no workspace, no atomics, nothing read back; every element of every output handed in is written.
//
// One kernel, one lane per point.  A workgroup serves the samples its points name one after the other, lowest first
// (one round when the points are grouped by sample, as a batch normally is): the first 2 * PT_TILE lanes evaluate the
// per-box terms of the predicate (csrc/box_predicate.h) for a tile of the sample's gt boxes and of its enlarged boxes,
// once per box, into LDS; then every lane of that sample reads them back, each from one address (a broadcast), and
// tests its point.  A point whose first column names no sample in [0, B) takes part in no round.  The foreground
// lanes then encode their box (PointResidualCoder.encode_torch) and their part offsets.
// The arithmetic is the contract of DESIGN.md section 7l: float32, one rounding per operation in the written order
// (built with -ffp-contract=off), log / cos / sin as the double function rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "box_predicate.h"

namespace {

constexpr int PT_T = 256;      // lanes (points) per workgroup
constexpr int PT_TILE = 64;    // boxes of each of the two sets staged in LDS at a time
constexpr int PT_TERMS = 9;    // the floats of a BoxTerms
constexpr int PT_NONE = 0x7fffffff;

struct Params {
    int64_t n;                     // points (n, 4)
    int ps;                        // their row stride in elements
    int b, m;                      // boxes (b, m, 8)
    int gs_b, gs_m, gs_c;          // strides of gt in elements (32 bits: the kernel's scalar registers are all in use)
    int es_b, es_m, es_c;          // strides of the enlarged boxes
    int num_class, n_mean;         // n_mean rows of mean_size (0 without)
    const float *points, *gt, *ext, *mean;
    int64_t *labels;
    float *box, *part;             // (n, 8) / (n, 3) or NULL
};

// cos and sin of a as box_terms evaluates them, out of line: the kernel holds one copy of the double functions
__device__ __noinline__ float2 cos_sin(float a) { return make_float2(modest::cos_f32(a), modest::sin_f32(a)); }

// box_terms of a strided row
__device__ __forceinline__ BoxTerms strided_terms(const float *row, int64_t sc) {
    BoxTerms t;
    t.cx = row[0]; t.cy = row[sc]; t.cz = row[2 * sc];
    const float dx = row[3 * sc], dy = row[4 * sc], dz = row[5 * sc], rz = row[6 * sc];
    const float2 cs = cos_sin(-rz);
    t.cosa = cs.x;
    t.sina = cs.y;
    t.nsina = -t.sina;
    const double margin = (double)1e-5f;
    t.tz = f32_down((double)dz / 2.0);
    t.tx = f32_up((double)dx / 2.0 + margin);
    t.ty = f32_up((double)dy / 2.0 + margin);
    return t;
}

__global__ __launch_bounds__(PT_T) void pt_assign(Params p) {
    __shared__ float s_t[2][PT_TERMS][PT_TILE];
    __shared__ int s_next[PT_T / 64];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * PT_T + tid;
    const bool ok = i < p.n;
    float x = 0.f, y = 0.f, z = 0.f;
    int k = -1;   // the point's sample, -1: none
    if (ok) {
        const float *pt = p.points + i * p.ps;
        const float bs = pt[0];
        x = pt[1]; y = pt[2]; z = pt[3];
        if (bs >= 0.f && bs < (float)p.b) {   // NaN fails both
            const int t = (int)bs;
            if ((float)t == bs) k = t;
        }
    }
    int idx = -1;       // lowest gt box of sample k holding the point
    bool ext = false;   // some enlarged box of sample k holds it
    int done = -1;      // samples <= done are served
    for (;;) {
        int next = k > done ? k : PT_NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) next = min(next, __shfl_xor(next, off));
        if ((tid & 63) == 0) s_next[tid >> 6] = next;
        __syncthreads();
        int s = s_next[0];
#pragma unroll
        for (int w = 1; w < PT_T / 64; ++w) s = min(s, s_next[w]);
        if (s == PT_NONE) break;   // the same for every lane of the workgroup
        const bool mine = k == s;
        for (int j0 = 0; j0 < p.m; j0 += PT_TILE) {
            const int cnt = min(PT_TILE, p.m - j0);
            if (tid < 2 * PT_TILE) {
                const int set = tid / PT_TILE, j = tid % PT_TILE;
                if (j < cnt) {
                    const float *row = set ? p.ext + (int64_t)s * p.es_b + (int64_t)(j0 + j) * p.es_m
                                           : p.gt + (int64_t)s * p.gs_b + (int64_t)(j0 + j) * p.gs_m;
                    const BoxTerms t = strided_terms(row, set ? p.es_c : p.gs_c);
                    float(*d)[PT_TILE] = s_t[set];
                    d[0][j] = t.cx; d[1][j] = t.cy; d[2][j] = t.cz; d[3][j] = t.cosa; d[4][j] = t.sina;
                    d[5][j] = t.nsina; d[6][j] = t.tz; d[7][j] = t.tx; d[8][j] = t.ty;
                }
            }
            __syncthreads();
            if (mine) {
                for (int j = 0; j < cnt; ++j) {
                    if (idx < 0 && pt_in_box(x, y, z, s_t[0][0][j], s_t[0][1][j], s_t[0][2][j], s_t[0][3][j], s_t[0][4][j],
                                             s_t[0][5][j], s_t[0][6][j], s_t[0][7][j], s_t[0][8][j]))
                        idx = j0 + j;
                    if (!ext)
                        ext = pt_in_box(x, y, z, s_t[1][0][j], s_t[1][1][j], s_t[1][2][j], s_t[1][3][j], s_t[1][4][j],
                                        s_t[1][5][j], s_t[1][6][j], s_t[1][7][j], s_t[1][8][j]);
                }
            }
            __syncthreads();   // the tile has been read
        }
        done = s;
        __syncthreads();       // s_next has been read (m == 0 has no tile barrier)
    }
    if (!ok) return;
    const bool fg = idx >= 0;
    const float *g = p.gt + (fg ? (int64_t)k * p.gs_b + (int64_t)idx * p.gs_m : 0);
    const int64_t sc = p.gs_c;
    int64_t cls = 0;
    if (fg) cls = (int64_t)g[7 * sc];   // .long(): truncated
    int64_t label = 0;
    if (fg != ext) label = -1;
    if (fg) label = p.num_class == 1 ? 1 : cls;
    p.labels[i] = label;
    const float tiny = 1e-5f;
    // cos / sin of the heading (box labels) and of its negation (part labels): one copy of the double functions
    float cs_rg = 0.f, sn_rg = 0.f, cs_nrg = 0.f, sn_nrg = 0.f;
    if (fg) {
        const float rg = g[6 * sc];
        if (p.box) { const float2 cs = cos_sin(rg); cs_rg = cs.x; sn_rg = cs.y; }
        if (p.part) { const float2 cs = cos_sin(-rg); cs_nrg = cs.x; sn_nrg = cs.y; }
    }
    if (p.box) {
        float *t = p.box + i * 8;
        if (!fg) {
#pragma unroll
            for (int c = 0; c < 8; ++c) t[c] = 0.f;
        } else {
            // PointResidualCoder.encode_torch of gt row idx against the point
            const float dxg = fmaxf(g[3 * sc], tiny), dyg = fmaxf(g[4 * sc], tiny), dzg = fmaxf(g[5 * sc], tiny);
            const float ex = g[0] - x, ey = g[sc] - y, ez = g[2 * sc] - z;
            if (p.mean) {
                int64_t r = cls - 1;
                if (r < 0) r += p.n_mean;   // Python's wrap: class 0 names the last row
                if (r >= 0 && r < p.n_mean) {
                    const float dxa = p.mean[r * 3], dya = p.mean[r * 3 + 1], dza = p.mean[r * 3 + 2];
                    const float diag = sqrtf(dxa * dxa + dya * dya);
                    t[0] = ex / diag;
                    t[1] = ey / diag;
                    t[2] = ez / dza;
                    t[3] = (float)log((double)(dxg / dxa));
                    t[4] = (float)log((double)(dyg / dya));
                    t[5] = (float)log((double)(dzg / dza));
                } else {   // a class beyond the table (the reference asserts): nothing is read, the six labels are NaN
#pragma unroll
                    for (int c = 0; c < 6; ++c) t[c] = __uint_as_float(0x7fc00000u);
                }
            } else {
                t[0] = ex; t[1] = ey; t[2] = ez;
                t[3] = (float)log((double)dxg);
                t[4] = (float)log((double)dyg);
                t[5] = (float)log((double)dzg);
            }
            t[6] = cs_rg;
            t[7] = sn_rg;
        }
    }
    if (p.part) {
        float *t = p.part + i * 3;
        if (!fg) {
            t[0] = 0.f; t[1] = 0.f; t[2] = 0.f;
        } else {
            // the coder clamps the sizes of the foreground rows in place, so they reach here clamped when it ran
            float dx = g[3 * sc], dy = g[4 * sc], dz = g[5 * sc];
            if (p.box) { dx = fmaxf(dx, tiny); dy = fmaxf(dy, tiny); dz = fmaxf(dz, tiny); }
            const float c = cs_nrg, s = sn_nrg;
            const float sx = x - g[0], sy = y - g[sc], sz = z - g[2 * sc];
            const float lx = sx * c + sy * (-s);
            const float ly = sx * s + sy * c;
            t[0] = lx / dx + 0.5f;
            t[1] = ly / dy + 0.5f;
            t[2] = sz / dz + 0.5f;
        }
    }
}

}  // namespace

extern "C" int modest_point_targets(int64_t n, const float *points_dev, int64_t points_stride, int b, int m,
                                    const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_m, int64_t gt_stride_c,
                                    const float *ext_dev, int64_t ext_stride_b, int64_t ext_stride_m,
                                    int64_t ext_stride_c, const float *mean_size_dev, int n_mean, int num_class,
                                    int64_t *cls_labels_dev, float *box_labels_dev, float *part_labels_dev,
                                    void *stream) {
    MODEST_REQUIRE(n >= 0 && b >= 0 && m >= 0 && n_mean >= 0, "negative size");
    MODEST_REQUIRE(b <= (1 << 24), "more than 2^24 samples");
    MODEST_REQUIRE((points_stride >= 4 || n <= 1) && points_stride <= 2147483647, "points row stride below 4 or beyond 2^31");
    for (int64_t st : {gt_stride_b, gt_stride_m, gt_stride_c, ext_stride_b, ext_stride_m, ext_stride_c})
        MODEST_REQUIRE(st >= -2147483647 && st <= 2147483647, "box stride beyond 32 bits");
    MODEST_REQUIRE((mean_size_dev != nullptr) == (n_mean > 0), "mean_size and its row count disagree");
    if (n == 0) return MODEST_OK;
    const int64_t blocks = (n + PT_T - 1) / PT_T;
    MODEST_REQUIRE(blocks <= 2147483647, "grid too large");
    MODEST_REQUIRE(points_dev && cls_labels_dev, "NULL buffer");
    MODEST_REQUIRE(b == 0 || m == 0 || (gt_dev && ext_dev), "NULL buffer");
    Params p;
    p.n = n; p.ps = (int)points_stride;
    p.b = m == 0 ? 0 : b;   // without boxes no point has a sample to test
    p.m = m;
    p.gs_b = (int)gt_stride_b; p.gs_m = (int)gt_stride_m; p.gs_c = (int)gt_stride_c;
    p.es_b = (int)ext_stride_b; p.es_m = (int)ext_stride_m; p.es_c = (int)ext_stride_c;
    p.num_class = num_class; p.n_mean = n_mean;
    p.points = points_dev; p.gt = gt_dev; p.ext = ext_dev; p.mean = mean_size_dev;
    p.labels = cls_labels_dev; p.box = box_labels_dev; p.part = part_labels_dev;
    pt_assign<<<dim3((unsigned)blocks), PT_T, 0, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
