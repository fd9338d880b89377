// The two box-membership ops PointRCNN needs besides BEV IoU and the PointNet++ ops, hand-written for gfx950:
//   * modest_roipoint_pool3d  -- roipoint_pool3d_cuda.forward   (OpenPCDet pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu)
//   * modest_points_in_boxes  -- roiaware_pool3d_cuda.points_in_boxes_gpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:313-336)
// Two entry points (include/modest_hip.h, "a23"): enqueue only, no synchronise, no context, no device allocation.
//
// The predicate (the contract).  Box [cx, cy, cz, dx, dy, dz, rz], point (x, y, z):
//     outside  if  (double)fabsf(z - cz) > (double)dz / 2.0
//     lx = sx * cosa + sy * (-sina),  ly = sx * sina + sy * cosa      (float32, one rounding per operation, no contraction)
//     inside   if  (double)|lx| < (double)dx / 2.0 + (double)1e-5f  and  (double)|ly| < (double)dy / 2.0 + (double)1e-5f
// with sx = x - cx, sy = y - cy in float32 and cosa / sina the double cos / sin of (double)(-rz) rounded once to float32
// (trig_f32.h), evaluated once per box (pooling) or once per box and workgroup (points in boxes), never per pair.
//
// The three comparisons are between a float32 value a and a double bound D.  They are decided here in float32 against
// a per-box threshold, exactly:
//     a > D  <=>  a > down(D),   down(D) = the largest float32 <= D
//     a < D  <=>  a < up(D),     up(D)   = the smallest float32 >= D
// Proof of the first (the second is its mirror image).  "=>": down(D) <= D < a.  "<=": a is a float32 above the
// largest float32 that is <= D, so a is not <= D.  D = +-inf: down / up are the same infinity and both sides agree
// (a > +inf never, a > -inf for every a but NaN).  NaN: a NaN bound gives a NaN threshold and a NaN a compares false
// on both sides.  So a NaN dz or a NaN z does NOT reject (the reference's `>` is false), a NaN anywhere else does.
// The plain float32 rule `a < dx * 0.5f + 1e-5f` is not equivalent: that sum may round below D.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "box_predicate.h"
#include "common.h"
#include "modest_hip.h"
#include "trig_f32.h"

namespace {

// ---------------------------------------------------------------- RoI point pooling -------------------------------
// One workgroup of four wavefronts per (cloud, box); the box's terms are computed once (every lane the same values, in
// registers).  The cloud is walked in index order in chunks of 1024 points = 16 sub-blocks of 64; wavefront w takes the
// sub-blocks j with j mod 4 == w (four loads in flight per lane, a chunk's loads contiguous over the workgroup).  A
// ballot per sub-block gives its hits; the 16 hit counts go through LDS (two alternating rows: one barrier per chunk),
// every wavefront adds up the counts of the sub-blocks before its own and writes its hits at their rank into the LDS
// list, so the list is in index order whatever the wavefronts' timing.  All wavefronts see the same counts and leave
// the walk together once `want` hits are known -- the early exit is at chunk granularity.  Then the k % cnt fill of
// the list and the copy of the S rows of 3 + C floats, consecutive lanes on consecutive output floats.
constexpr int RP_WAVES = 4, RP_T = RP_WAVES * 64, RP_UNROLL = 4, RP_SUB = RP_WAVES * RP_UNROLL, RP_CHUNK = RP_SUB * 64;
constexpr int RP_MAX_S = 15360;   // the LDS list: 60 KB of dynamic LDS at the most

__global__ __launch_bounds__(RP_T) void roipoint_pool(int n, int m, int c, int s, const float *__restrict__ xyz_,
                                                     const float *__restrict__ boxes, const float *__restrict__ feat_,
                                                     float *__restrict__ pooled, int32_t *__restrict__ empty_flag) {
    extern __shared__ int list[];
    __shared__ int counts[2][RP_SUB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bm = blockIdx.x;   // b * m + box
    const int64_t b = bm / m;
    const float *p = xyz_ + b * n * 3;
    const BoxTerms t = box_terms(boxes + bm * 7);
    const int given = empty_flag[bm];
    // a box whose flag is already set gets no rows: all that matters is whether it has a point at all
    const int want = given ? min(s, 1) : s;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0, par = 0;
    for (int k0 = 0; k0 < n && cnt < want; k0 += RP_CHUNK, par ^= 1) {
        bool hit[RP_UNROLL];
#pragma unroll
        for (int u = 0; u < RP_UNROLL; ++u) {
            const int k = k0 + (u * RP_WAVES + wave) * 64 + lane;   // k0 + 960 + 63 < n + 1024: n <= INT_MAX - 1024
            hit[u] = false;
            if (k < n) {
                const float x = p[(int64_t)k * 3 + 0], y = p[(int64_t)k * 3 + 1], z = p[(int64_t)k * 3 + 2];
                hit[u] = pt_in_box(x, y, z, t.cx, t.cy, t.cz, t.cosa, t.sina, t.nsina, t.tz, t.tx, t.ty);
            }
        }
        unsigned long long mask[RP_UNROLL];
#pragma unroll
        for (int u = 0; u < RP_UNROLL; ++u) {
            mask[u] = __ballot(hit[u]);
            if (lane == 0) counts[par][u * RP_WAVES + wave] = __popcll(mask[u]);
        }
        __syncthreads();
        int run = cnt;
#pragma unroll
        for (int u = 0; u < RP_UNROLL; ++u) {
#pragma unroll
            for (int w = 0; w < RP_WAVES; ++w) {
                if (w == wave) {
                    const int pos = run + __popcll(mask[u] & below);
                    if (hit[u] && pos < want) list[pos] = k0 + (u * RP_WAVES + wave) * 64 + lane;
                }
                run += counts[par][u * RP_WAVES + w];
            }
        }
        cnt = run;
    }
    if (cnt == 0) {
        if (tid == 0) empty_flag[bm] = 1;
        return;
    }
    if (given) return;
    cnt = min(cnt, s);
    __syncthreads();
    for (int l = cnt + tid; l < s; l += RP_T) list[l] = list[l % cnt];   // reads below cnt, writes at or above it
    __syncthreads();
    const int width = 3 + c;
    const float *feat = feat_ + b * n * c;
    float *out = pooled + bm * s * width;
    const int64_t total = (int64_t)s * width;
    // element e = row * width + col; a thread's e advances by RP_T: (row, col) follow without a division per element
    const int drow = RP_T / width, dcol = RP_T % width;
    int row = tid / width, col = tid % width;
    for (int64_t e = tid; e < total; e += RP_T) {
        const int64_t i = list[row];
        out[e] = col < 3 ? p[i * 3 + col] : feat[i * c + (col - 3)];
        row += drow;
        col += dcol;
        if (col >= width) { col -= width; ++row; }
    }
}

// ---------------------------------------------------------------- points in boxes ---------------------------------
// One lane per point, 256 points per workgroup.  The cloud's boxes pass through LDS in tiles of PB_TILE: thread i of
// the workgroup computes the terms of the tile's box i (trig once per box and workgroup), every lane then walks the
// tile in index order reading each box's terms from one LDS address (a broadcast) and keeps its first hit.  A
// wavefront leaves a tile once all its lanes are decided, the workgroup stops staging tiles once all its lanes are.
constexpr int PB_T = 256, PB_TILE = 128;

__global__ __launch_bounds__(PB_T) void points_in_boxes(int m, int n, int blocks_per_cloud, const float *__restrict__ boxes_,
                                                       const float *__restrict__ pts, int32_t *__restrict__ box_idx) {
    __shared__ float terms[PB_TILE][9];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / blocks_per_cloud;
    const int pt = (int)(blockIdx.x % blocks_per_cloud) * PB_T + tid;
    const bool ok = pt < n;
    const int64_t q = (b * n + (ok ? pt : 0)) * 3;
    const float x = pts[q + 0], y = pts[q + 1], z = pts[q + 2];
    const float *boxes = boxes_ + b * m * 7;
    int res = ok ? -1 : 0;   // a lane without a point is decided from the start
    for (int k0 = 0; k0 < m; k0 += PB_TILE) {
        const int cnt = min(PB_TILE, m - k0);
        if (tid < cnt) {
            const BoxTerms t = box_terms(boxes + (int64_t)(k0 + tid) * 7);
            float *d = terms[tid];
            d[0] = t.cx; d[1] = t.cy; d[2] = t.cz; d[3] = t.cosa; d[4] = t.sina; d[5] = t.nsina;
            d[6] = t.tz; d[7] = t.tx; d[8] = t.ty;
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            if (__ballot(res < 0) == 0ull) break;
            const float *d = terms[k];
            if (res < 0 && pt_in_box(x, y, z, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8])) res = k0 + k;
        }
        if (__syncthreads_and(res >= 0)) break;   // also the barrier ahead of the next tile's staging
    }
    if (ok && res >= 0) box_idx[b * n + pt] = res;
}

}  // namespace

extern "C" int modest_roipoint_pool3d(int b, int n, int m, int c, int s, const float *xyz_dev, const float *boxes_dev,
                                      const float *feat_dev, float *pooled_dev, int32_t *empty_flag_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c >= 0 && s >= 0, "negative size");
    MODEST_REQUIRE(n <= 2147483647 - RP_CHUNK, "too many points per cloud");
    MODEST_REQUIRE(s <= RP_MAX_S, "more sampled points per box than the LDS list holds (15360)");
    const int64_t pairs = (int64_t)b * m;
    if (pairs == 0) return MODEST_OK;
    MODEST_REQUIRE(pairs <= GRID_MAX, "grid too large");
    MODEST_REQUIRE(boxes_dev && empty_flag_dev, "NULL buffer");
    MODEST_REQUIRE(n == 0 || (xyz_dev && (c == 0 || feat_dev) && (s == 0 || pooled_dev)), "NULL buffer");
    const size_t lds = (size_t)(s > 0 ? s : 1) * sizeof(int);
    roipoint_pool<<<(unsigned)pairs, RP_T, lds, as_stream(stream)>>>(n, m, c, s, xyz_dev, boxes_dev, feat_dev, pooled_dev,
                                                                   empty_flag_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_points_in_boxes(int b, int m, int n, const float *boxes_dev, const float *pts_dev,
                                      int32_t *box_idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && n >= 0, "negative size");
    if (b == 0 || m == 0 || n == 0) return MODEST_OK;
    MODEST_REQUIRE(boxes_dev && pts_dev && box_idx_dev, "NULL buffer");
    const int bpc = (int)(((int64_t)n + PB_T - 1) / PB_T);
    const int64_t blocks = (int64_t)b * bpc;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    points_in_boxes<<<(unsigned)blocks, PB_T, 0, as_stream(stream)>>>(m, n, bpc, boxes_dev, pts_dev, box_idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
