// The RoI-aware voxel pooling of PartA2, hand-written for gfx950:
//   * modest_roiaware_pool3d_forward   -- roiaware_pool3d_cuda.forward  (OpenPCDet pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:39-233)
//   * modest_roiaware_pool3d_backward  -- roiaware_pool3d_cuda.backward (roiaware_pool3d_kernel.cu:236-310)
// Entry points of include/modest_hip.h, "a28": enqueue only, no synchronise, no context, no device allocation.
//
// The contract is DESIGN.md section 7j.  The inside test is the predicate of section 7e (box_predicate.h).  The voxel
// of an inside point, all in float32 with one rounding per operation and correctly rounded divisions:
//     res_x = dx / (float)out_x,   q_x = (lx + dx / 2.0f) / res_x        (the same for y; for z with lz = z - cz)
//     index = min(max((unsigned)(int)q, 0), out - 1)   with the int cast to unsigned, conversions saturating, NaN -> 0:
//             NaN -> 0;  q <= -1 -> out - 1;  q >= out -> out - 1;  otherwise truncation toward zero.
// A voxel's list is [count, point, point, ...] in ascending point index, at most max_pts_each_voxel - 1 points; the
// count word is WRITTEN (the reference increments what it is given).  Pooling walks a list in slot order.  The
// backward sums, for every (point, channel), over the boxes in ascending box index, without atomics.
//
// No intermediate over (boxes, points) in the forward: the reference's (N, npoints) mask, its cudaMalloc / cudaFree
// per call and its one-thread-per-box collect loop are replaced by one workgroup per box that walks the cloud once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "box_predicate.h"
#include "common.h"
#include "modest_hip.h"

namespace {

// min(max((unsigned)(int)q, 0), out - 1) of the reference, its cases written out: nothing here converts a NaN or an
// out-of-range float to int.  1 <= out <= 256.
__device__ __forceinline__ int voxel_index(float q, int out) {
    if (q != q) return 0;                  // NaN converts to 0
    if (q <= -1.0f) return out - 1;        // a negative int is a huge unsigned: clamped from above (-inf -> INT_MIN too)
    if (q >= (float)out) return out - 1;   // +inf / overflow -> INT_MAX: clamped from above
    return (int)q;                         // -1 < q < out <= 256: truncation toward zero, (-1, 0) -> 0
}

// ---------------------------------------------------------------- collect: the per-voxel lists -------------------------
// One workgroup of four wavefronts per box; the box's terms are computed once.  The cloud is walked in index order in
// chunks of 1024 points = 16 sub-blocks of 64, wavefront w takes the sub-blocks j with j mod 4 == w (as roipoint_pool
// does).  A ballot per sub-block gives its hits, the 16 hit counts go through LDS, and every wavefront writes its hits
// (point index, voxel id) at their rank into the chunk's hit list in LDS: the hit list is in index order whatever the
// wavefronts' timing.  Then the insert step: wavefront w takes the hits whose voxel id is == w (mod 4), 64 consecutive
// entries of the hit list at a time, so no two wavefronts ever touch the same voxel counter.  Within such a group
// every lane first reads its voxel's counter (dynamic LDS, one word per voxel), then the lanes of one voxel are found
// with a ballot per distinct voxel -- registers only -- and a hit's slot is that counter plus the number of LOWER lanes
// of the same voxel: lane order is hit-list order is point-index order.  The voxel's highest lane then adds the
// group's size to the counter.  Nothing depends on the order in which an atomic lands: there is none.  At the end
// every voxel's count word is written, capped at max_pts - 1.
constexpr int RA_WAVES = 4, RA_T = RA_WAVES * 64, RA_UNROLL = 4, RA_SUB = RA_WAVES * RA_UNROLL, RA_CHUNK = RA_SUB * 64;
constexpr int RA_MAX_VOXELS = 13824;   // 24^3 counters = 54 KB of dynamic LDS; with the 8 KB hit list below 64 KB

__global__ __launch_bounds__(RA_T) void roiaware_collect(int pts_num, int max_pts, int out_x, int out_y, int out_z,
                                                        const float *__restrict__ rois, const float *__restrict__ pts,
                                                        int32_t *__restrict__ lists) {
    extern __shared__ int counter[];
    __shared__ int hit_k[RA_CHUNK], hit_v[RA_CHUNK];
    __shared__ int counts[RA_SUB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t box = blockIdx.x;
    const int nvox = out_x * out_y * out_z;
    const float *bx = rois + box * 7;
    const BoxTerms t = box_terms(bx);
    const float dx = bx[3], dy = bx[4], dz = bx[5];
    const float res_x = dx / (float)out_x, res_y = dy / (float)out_y, res_z = dz / (float)out_z;
    const float half_x = dx / 2.0f, half_y = dy / 2.0f, half_z = dz / 2.0f;
    int32_t *mine = lists + box * nvox * max_pts;
    const int cap = max_pts - 1;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int v = tid; v < nvox; v += RA_T) counter[v] = 0;
    // (the first barrier of the walk, or the one behind it, orders the zeroes before the first insert)
    for (int k0 = 0; k0 < pts_num; k0 += RA_CHUNK) {
        bool hit[RA_UNROLL];
        int vox[RA_UNROLL];
#pragma unroll
        for (int u = 0; u < RA_UNROLL; ++u) {
            const int k = k0 + (u * RA_WAVES + wave) * 64 + lane;   // k0 + 960 + 63 < n + 1024: n <= INT_MAX - 1024
            hit[u] = false;
            vox[u] = 0;
            if (k < pts_num) {
                const float x = pts[(int64_t)k * 3 + 0], y = pts[(int64_t)k * 3 + 1], z = pts[(int64_t)k * 3 + 2];
                float lx, ly;
                hit[u] = pt_in_box_local(x, y, z, t.cx, t.cy, t.cz, t.cosa, t.sina, t.nsina, t.tz, t.tx, t.ty, lx, ly);
                const float lz = z - t.cz;
                const int ix = voxel_index((lx + half_x) / res_x, out_x);
                const int iy = voxel_index((ly + half_y) / res_y, out_y);
                const int iz = voxel_index((lz + half_z) / res_z, out_z);
                vox[u] = (ix * out_y + iy) * out_z + iz;
            }
        }
        unsigned long long mask[RA_UNROLL];
#pragma unroll
        for (int u = 0; u < RA_UNROLL; ++u) {
            mask[u] = __ballot(hit[u]);
            if (lane == 0) counts[u * RA_WAVES + wave] = __popcll(mask[u]);
        }
        __syncthreads();   // the counts are known; every wavefront is done with the previous chunk's hit list
        int run = 0;
#pragma unroll
        for (int u = 0; u < RA_UNROLL; ++u) {
#pragma unroll
            for (int w = 0; w < RA_WAVES; ++w) {
                if (w == wave && hit[u]) {
                    const int pos = run + __popcll(mask[u] & below);   // < 1024
                    hit_k[pos] = k0 + (u * RA_WAVES + wave) * 64 + lane;
                    hit_v[pos] = vox[u];
                }
                run += counts[u * RA_WAVES + w];
            }
        }
        const int nh = run;   // the same in every wavefront
        __syncthreads();      // the hit list is complete; the counts may be overwritten
        for (int j0 = 0; j0 < nh; j0 += 64) {
            const int j = j0 + lane;
            const bool have = j < nh;
            const int v = have ? hit_v[j] : -1;
            const int k = have ? hit_k[j] : 0;
            bool act = have && ((v & (RA_WAVES - 1)) == wave);
            // the counter of the lane's voxel before this group: the same value in every lane of that voxel (only
            // this wavefront writes it, and not before the loop below is over).  A full list takes no more points
            // and its counter need not grow: the count word is capped anyway.
            const int base = act ? counter[v] : 0;
            act = act && base < cap;
            int rank = 0, size = 0;
            unsigned long long todo = __ballot(act);
            while (todo != 0ull) {   // one round per distinct voxel among the active lanes: ballots only, no memory
                const int leader = __ffsll((long long)todo) - 1;
                const int lv = __builtin_amdgcn_readlane(v, leader);
                const bool same = act && v == lv;
                const unsigned long long group = __ballot(same);
                if (same) {
                    rank = __popcll(group & below);
                    size = __popcll(group);
                }
                todo &= ~group;
            }
            if (act) {   // 0 <= v < nvox
                const int slot = base + rank;
                if (slot < cap) mine[(int64_t)v * max_pts + 1 + slot] = k;
                if (rank == size - 1) counter[v] = base + size;   // the voxel's highest lane
            }
        }
    }
    __syncthreads();
    for (int v = tid; v < nvox; v += RA_T) mine[(int64_t)v * max_pts] = min(counter[v], cap);
}

// ---------------------------------------------------------------- pooling ------------------------------------------------
// One lane per element of (N, V, C), consecutive lanes on consecutive channels: a point's feature row is one contiguous
// read over the lanes of a voxel, the list words are read from one address per voxel, the stores are coalesced.
// max: strictly greater than the best so far, from -inf (the reference's -1e50 as a float): the first of equal maxima
// wins, -inf and NaN never win; argmax is written for every element, pooled only where argmax != -1.
// avg: the float32 sum in slot order from +0 divided by (float)count, written only where count > 0.
constexpr int RP_T = 256;

template <int METHOD>
__global__ __launch_bounds__(RP_T) void roiaware_pool(int64_t total, int channels, int max_pts,
                                                     const float *__restrict__ feat, const int32_t *__restrict__ lists,
                                                     float *__restrict__ pooled, int32_t *__restrict__ argmax) {
    const int64_t e0 = (int64_t)blockIdx.x * RP_T;
    const int64_t e = e0 + threadIdx.x;
    if (e >= total) return;
    // (box, voxel) and channel of e: one 64-bit division per workgroup (uniform), a 32-bit one per lane
    const int64_t bv0 = e0 / channels;
    const int t = (int)(e0 - bv0 * channels) + (int)threadIdx.x;   // < channels + 256
    const int64_t bv = bv0 + t / channels;
    const int c = t % channels;
    const int32_t *l = lists + bv * max_pts;
    const int cnt = l[0];
    if (METHOD == 0) {
        float best = -INFINITY;
        int arg = -1;
        for (int k = 1; k <= cnt; ++k) {
            const int p = l[k];
            const float val = feat[(int64_t)p * channels + c];
            if (val > best) { best = val; arg = p; }
        }
        argmax[e] = arg;
        if (arg != -1) pooled[e] = best;
    } else {
        float sum = 0.f;
        for (int k = 1; k <= cnt; ++k) sum += feat[(int64_t)l[k] * channels + c];
        if (cnt > 0) pooled[e] = sum / (float)cnt;
    }
}

// ---------------------------------------------------------------- backward -----------------------------------------------
// A point lies in at most one voxel of a box, so the gradient of (point p, channel c) collects at most one term per
// box.  First the lists are turned round into a table T[p][b] = the voxel of box b that lists p, -1 for none
// ((npoints, N) int32, the caller's workspace, preset to -1 by a memset on the stream): one wavefront per 64 voxels
// reads their count words, then takes the non-empty ones in turn with its lanes across the slots.  The writes are
// collision-free.  Then one lane per (p, c) walks b ascending -- T's row is read from one address per point -- and adds
// in that order: the sum has one set of bits.  Indices read from the lists are checked against pts_num.
constexpr int RB_T = 256;

__global__ __launch_bounds__(RB_T) void roiaware_table(int64_t nbv, int nvox, int boxes_num, int pts_num, int max_pts,
                                                      const int32_t *__restrict__ lists, int32_t *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const int64_t first = ((int64_t)blockIdx.x * (RB_T / 64) + (threadIdx.x >> 6)) * 64;   // the wavefront's first voxel
    if (first >= nbv) return;
    const int64_t b0 = first / nvox;
    const int v0 = (int)(first - b0 * nvox);
    int cnt = 0;
    if (first + lane < nbv) cnt = min(max(lists[(first + lane) * max_pts], 0), max_pts - 1);
    unsigned long long todo = __ballot(cnt > 0);
    while (todo != 0ull) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int scnt = __shfl(cnt, src);
        const int tv = v0 + src;                 // < nvox + 64
        const int64_t b = b0 + tv / nvox;
        const int v = tv % nvox;
        const int32_t *l = lists + (first + src) * max_pts;
        for (int k = 1 + lane; k <= scnt; k += 64) {
            const int p = l[k];
            if ((unsigned)p < (unsigned)pts_num) table[(int64_t)p * boxes_num + b] = v;
        }
    }
}

template <int METHOD>
__global__ __launch_bounds__(RB_T) void roiaware_backward(int64_t total, int channels, int boxes_num, int nvox, int max_pts,
                                                         const int32_t *__restrict__ table,
                                                         const int32_t *__restrict__ lists,
                                                         const int32_t *__restrict__ argmax,
                                                         const float *__restrict__ grad_out, float *__restrict__ grad_in) {
    const int64_t e0 = (int64_t)blockIdx.x * RB_T;
    const int64_t e = e0 + threadIdx.x;
    if (e >= total) return;
    const int64_t p0 = e0 / channels;
    const int t = (int)(e0 - p0 * channels) + (int)threadIdx.x;
    const int64_t p = p0 + t / channels;
    const int c = t % channels;
    const int32_t *row = table + p * boxes_num;
    float g = grad_in[e];
    bool any = false;
    for (int b = 0; b < boxes_num; ++b) {
        const int v = row[b];
        if (v < 0) continue;
        const int64_t bv = (int64_t)b * nvox + v;
        if (METHOD == 0) {
            if ((int64_t)argmax[bv * channels + c] == p) {
                g += grad_out[bv * channels + c];
                any = true;
            }
        } else {
            const int cnt = lists[bv * max_pts];
            const float w = 1.0f / fmaxf((float)cnt, 1.0f);
            const float term = grad_out[bv * channels + c] * w;
            g += term;
            any = true;
        }
    }
    if (any) grad_in[e] = g;
}

int check_grid(int out_x, int out_y, int out_z) {
    return out_x >= 1 && out_x <= 256 && out_y >= 1 && out_y <= 256 && out_z >= 1 && out_z <= 256;
}

}  // namespace

extern "C" int modest_roiaware_pool3d_forward(int boxes_num, int pts_num, int channels, int max_pts_each_voxel, int out_x,
                                              int out_y, int out_z, const float *rois_dev, const float *pts_dev,
                                              const float *pts_feature_dev, int32_t *argmax_dev,
                                              int32_t *pts_idx_of_voxels_dev, float *pooled_features_dev, int pool_method,
                                              void *stream) {
    MODEST_REQUIRE(boxes_num >= 0 && pts_num >= 0 && channels >= 0, "negative size");
    MODEST_REQUIRE(pool_method == 0 || pool_method == 1, "pool_method is 0 (max) or 1 (avg)");
    MODEST_REQUIRE(max_pts_each_voxel >= 1, "max_pts_each_voxel counts the count word: at least 1");
    MODEST_REQUIRE(check_grid(out_x, out_y, out_z), "every out size must lie in 1..256");
    MODEST_REQUIRE((int64_t)out_x * out_y * out_z <= RA_MAX_VOXELS,
                   "more voxels per box than the LDS counters hold (13824)");
    MODEST_REQUIRE(pts_num <= 2147483647 - RA_CHUNK, "too many points");
    MODEST_REQUIRE(channels <= (1 << 30), "too many channels");
    if (boxes_num == 0) return MODEST_OK;
    const int nvox = out_x * out_y * out_z;
    MODEST_REQUIRE(rois_dev && pts_idx_of_voxels_dev, "NULL buffer");
    MODEST_REQUIRE(pts_num == 0 || pts_dev, "NULL buffer");
    const int64_t total = (int64_t)boxes_num * nvox * channels;
    MODEST_REQUIRE(total == 0 || (pooled_features_dev && (pool_method == 1 || argmax_dev) && (pts_num == 0 || pts_feature_dev)),
                   "NULL buffer");
    const int64_t blocks = (total + RP_T - 1) / RP_T;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    hipStream_t st = as_stream(stream);
    roiaware_collect<<<(unsigned)boxes_num, RA_T, (size_t)nvox * sizeof(int), st>>>(
        pts_num, max_pts_each_voxel, out_x, out_y, out_z, rois_dev, pts_dev, pts_idx_of_voxels_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    if (total == 0) return MODEST_OK;
    if (pool_method == 0)
        roiaware_pool<0><<<(unsigned)blocks, RP_T, 0, st>>>(total, channels, max_pts_each_voxel, pts_feature_dev,
                                                           pts_idx_of_voxels_dev, pooled_features_dev, argmax_dev);
    else
        roiaware_pool<1><<<(unsigned)blocks, RP_T, 0, st>>>(total, channels, max_pts_each_voxel, pts_feature_dev,
                                                           pts_idx_of_voxels_dev, pooled_features_dev, argmax_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int64_t modest_roiaware_pool3d_backward_workspace_bytes(int boxes_num, int pts_num) {
    if (boxes_num <= 0 || pts_num <= 0) return 0;
    return (int64_t)boxes_num * pts_num * (int64_t)sizeof(int32_t);
}

extern "C" int modest_roiaware_pool3d_backward(int boxes_num, int pts_num, int out_x, int out_y, int out_z, int channels,
                                               int max_pts_each_voxel, const int32_t *pts_idx_of_voxels_dev,
                                               const int32_t *argmax_dev, const float *grad_out_dev, float *grad_in_dev,
                                               int pool_method, void *workspace_dev, int64_t workspace_bytes,
                                               void *stream) {
    MODEST_REQUIRE(boxes_num >= 0 && pts_num >= 0 && channels >= 0, "negative size");
    MODEST_REQUIRE(pool_method == 0 || pool_method == 1, "pool_method is 0 (max) or 1 (avg)");
    MODEST_REQUIRE(max_pts_each_voxel >= 1, "max_pts_each_voxel counts the count word: at least 1");
    MODEST_REQUIRE(check_grid(out_x, out_y, out_z), "every out size must lie in 1..256");
    MODEST_REQUIRE(channels <= (1 << 30), "too many channels");
    if (boxes_num == 0 || pts_num == 0 || channels == 0) return MODEST_OK;
    const int64_t need = modest_roiaware_pool3d_backward_workspace_bytes(boxes_num, pts_num);
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace smaller than modest_roiaware_pool3d_backward_workspace_bytes");
    MODEST_REQUIRE(pts_idx_of_voxels_dev && grad_out_dev && grad_in_dev && (pool_method == 1 || argmax_dev), "NULL buffer");
    const int nvox = out_x * out_y * out_z;   // <= 2^24
    const int64_t nbv = (int64_t)boxes_num * nvox;
    const int64_t tblocks = (nbv + RB_T - 1) / RB_T;
    const int64_t total = (int64_t)pts_num * channels;
    const int64_t blocks = (total + RB_T - 1) / RB_T;
    MODEST_REQUIRE(tblocks <= GRID_MAX && blocks <= GRID_MAX, "grid too large");
    hipStream_t st = as_stream(stream);
    MODEST_HIP_CHECK(hipMemsetAsync(workspace_dev, 0xFF, (size_t)need, st));
    int32_t *table = static_cast<int32_t *>(workspace_dev);
    roiaware_table<<<(unsigned)tblocks, RB_T, 0, st>>>(nbv, nvox, boxes_num, pts_num, max_pts_each_voxel,
                                                      pts_idx_of_voxels_dev, table);
    MODEST_HIP_CHECK(hipGetLastError());
    if (pool_method == 0)
        roiaware_backward<0><<<(unsigned)blocks, RB_T, 0, st>>>(total, channels, boxes_num, nvox, max_pts_each_voxel, table,
                                                               pts_idx_of_voxels_dev, argmax_dev, grad_out_dev, grad_in_dev);
    else
        roiaware_backward<1><<<(unsigned)blocks, RB_T, 0, st>>>(total, channels, boxes_num, nvox, max_pts_each_voxel, table,
                                                               pts_idx_of_voxels_dev, argmax_dev, grad_out_dev, grad_in_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
