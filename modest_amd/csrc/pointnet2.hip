// PointNet++ set-abstraction ops of the detector (OpenPCDet pcdet/ops/pointnet2/pointnet2_batch/src/*.cu), hand-written
// for gfx950.  Nine entry points (include/modest_hip.h, "a22"): enqueue only, no synchronise, no context.
//
// What each result is (the contract):
//   * squared distances are (dx*dx + dy*dy) + dz*dz in float32, no contraction (the build's -ffp-contract=off);
//   * ball query: d2 < radius*radius strict, the FIRST nsample hits in index order, short rows padded with the first
//     hit, rows without a hit left as the caller gave them;
//   * three-NN: strict < against the running best three (kept in double like the reference, so that an infinite
//     distance still enters), unused slots 1e40 -> inf / index 0;
//   * furthest point sampling: the maximum of temp, ties decided by the reference's reduction tree: among the points at
//     the maximum the one whose bitreverse(k mod bs) is smallest, then the smallest k (bs = the reference's block size).
//     Here that is a 64-bit key (temp bits, ~rank) and a plain max, whatever the thread count or point-to-lane layout;
//   * gradients add into the buffer they are given; the order of the float32 additions is free (LDS atomics: two runs
//     may differ in the last bits).
// Every element offset is 64-bit.  An index outside [0, N) (the reference would read or write out of bounds) is
// skipped by the gradients and reads as 0 in the forward gathers.
// The ball walk with its placing and padding of the hits, and the tile walk and merge of three-NN, are pn2_search.h's,
// shared with the stacked layout (pointnet2_stack.hip); the kernels here resolve a cloud's pointers and store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "modest_hip.h"
#include "pn2_search.h"

namespace {

// ---------------------------------------------------------------- furthest point sampling -------------------------
// rank of point k in the reference's tie order: (bitreverse of k mod bs over L bits, k div bs); a smaller rank wins.
// L = log2 bs, S = bits of (n - 1) >> L; L + S <= 31, so ~rank >= 1 for every real point and key 0 marks "no point".
__device__ __forceinline__ unsigned fps_rank(unsigned k, int L, int S) {
    unsigned rev = L ? (__brev(k & ((1u << L) - 1u)) >> (32 - L)) : 0u;
    return (rev << S) | (k >> L);
}
__device__ __forceinline__ unsigned fps_unrank(unsigned r, int L, int S) {
    unsigned q = r & ((1u << S) - 1u), rev = r >> S;
    unsigned low = L ? (__brev(rev) >> (32 - L)) : 0u;
    return (q << L) | low;
}
__device__ __forceinline__ unsigned long long fps_key(float t, unsigned nrank) {
    return ((unsigned long long)__float_as_uint(t) << 32) | nrank;   // temp >= 0: its bits order like its value
}
// The 64-bit max across lanes by DPP moves (one vector instruction per half and step, no LDS crossbar): quad_perm
// [1,0,3,2] and [2,3,0,1] give every lane its quad's max, row_ror:4 and row_ror:8 its row's (16 lanes); the four row
// results are then read with v_readlane.  Every lane of the wavefront is active wherever these are called.
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
    int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long quad_max_u64(unsigned long long v) {
    v = umax64(v, dpp_u64<0xB1>(v));
    return umax64(v, dpp_u64<0x4E>(v));
}
__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long v) {
    v = quad_max_u64(v);
    v = umax64(v, dpp_u64<0x124>(v));
    return umax64(v, dpp_u64<0x128>(v));
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = row_max_u64(v);
    return umax64(umax64(readlane_u64(v, 0), readlane_u64(v, 16)), umax64(readlane_u64(v, 32), readlane_u64(v, 48)));
}
// the max of the WAVES per-wavefront results (WAVES = 4 or 16 consecutive slots, read as slot[lane & (WAVES - 1)])
template <int WAVES> __device__ __forceinline__ unsigned long long slots_max_u64(unsigned long long v) {
    static_assert(WAVES == 4 || WAVES == 16, "one quad or one row of lanes");
    return WAVES == 4 ? quad_max_u64(v) : row_max_u64(v);
}

// One workgroup of WAVES wavefronts per cloud, PPL points per lane: coordinates and temp stay in registers for all m - 1
// rounds, the cloud's coordinates also sit in LDS (the next round's centre is read from there, one broadcast read).
// A round: PPL distance updates per lane, a 64-bit max inside the wavefront (no LDS), one LDS exchange among the
// wavefronts (two alternating slots: one barrier per round), nothing at all when WAVES == 1.
template <int WAVES, int PPL>
__global__ __launch_bounds__(WAVES * 64) void pn2_fps_reg(int n, int m, int L, int S, const float *__restrict__ xyz_,
                                                          float *__restrict__ temp_, int32_t *__restrict__ idx_) {
    constexpr int T = WAVES * 64;
    __shared__ float sx[T * PPL * 3];
    __shared__ unsigned long long slot[2][WAVES > 1 ? WAVES : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const float *xyz = xyz_ + b * n * 3;
    float *temp = temp_ + b * n;
    int32_t *idx = idx_ + b * m;
    if (tid == 0) idx[0] = 0;
    if (m <= 1) return;
    for (int i = tid; i < 3 * n; i += T) sx[i] = xyz[i];
    float px[PPL], py[PPL], pz[PPL], t[PPL];
    unsigned nr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int k = j * T + tid;
        const bool ok = k < n;
        px[j] = ok ? xyz[(int64_t)k * 3 + 0] : 0.f;
        py[j] = ok ? xyz[(int64_t)k * 3 + 1] : 0.f;
        pz[j] = ok ? xyz[(int64_t)k * 3 + 2] : 0.f;
        t[j] = ok ? temp[k] : 0.f;
        nr[j] = ok ? ~fps_rank((unsigned)k, L, S) : 0u;
    }
    __syncthreads();
    int old = 0;
    for (int r = 1; r < m; ++r) {
        const float x1 = sx[old * 3 + 0], y1 = sx[old * 3 + 1], z1 = sx[old * 3 + 2];
        unsigned long long best = 0ull;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const float dx = px[j] - x1, dy = py[j] - y1, dz = pz[j] - z1;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const float t2 = fminf(d, t[j]);
            t[j] = t2;
            best = umax64(best, fps_key(t2, nr[j]));   // a lane's padding: temp 0 and ~rank 0 for ever, key 0
        }
        best = wave_max_u64(best);
        if constexpr (WAVES > 1) {
            if (lane == 0) slot[r & 1][wave] = best;
            __syncthreads();
            best = slots_max_u64<WAVES>(slot[r & 1][lane & (WAVES - 1)]);
        }
        old = (int)fps_unrank(~(unsigned)best, L, S);
        if (tid == 0) idx[r] = old;
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int k = j * T + tid;
        if (k < n) temp[k] = t[j];
    }
}

// Any N: temp and the coordinates stay in global memory (each lane re-reads its own points every round, as the reference
// does), the reduction is the same key max.  A lane touches only its own temp[k]; the winner's index travels through the
// two alternating LDS slots, so no round reads what the next one overwrites.
__global__ __launch_bounds__(1024) void pn2_fps_global(int n, int m, int L, int S, const float *__restrict__ xyz_,
                                                       float *__restrict__ temp_, int32_t *__restrict__ idx_) {
    constexpr int WAVES = 16, T = 1024;
    __shared__ unsigned long long slot[2][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const float *xyz = xyz_ + b * n * 3;
    float *temp = temp_ + b * n;
    int32_t *idx = idx_ + b * m;
    if (tid == 0) idx[0] = 0;
    if (m <= 1) return;
    int old = 0;
    for (int r = 1; r < m; ++r) {
        const float x1 = xyz[(int64_t)old * 3 + 0], y1 = xyz[(int64_t)old * 3 + 1], z1 = xyz[(int64_t)old * 3 + 2];
        unsigned long long best = 0ull;
        for (int k = tid; k < n; k += T) {
            const float dx = xyz[(int64_t)k * 3 + 0] - x1, dy = xyz[(int64_t)k * 3 + 1] - y1, dz = xyz[(int64_t)k * 3 + 2] - z1;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const float t2 = fminf(d, temp[k]);
            temp[k] = t2;
            best = umax64(best, fps_key(t2, ~fps_rank((unsigned)k, L, S)));
        }
        best = wave_max_u64(best);
        if (lane == 0) slot[r & 1][wave] = best;
        __syncthreads();
        best = slots_max_u64<WAVES>(slot[r & 1][lane & (WAVES - 1)]);
        old = (int)fps_unrank(~(unsigned)best, L, S);
        if (tid == 0) idx[r] = old;
    }
}

// ---------------------------------------------------------------- ball query ---------------------------------------
// A wavefront per centre; the walk, the order of the hits and the padding are pn2_search.h's.
__global__ __launch_bounds__(256) void pn2_ball_query(int64_t centres, int n, int m, float r2, int nsample,
                                                      const float *__restrict__ new_xyz, const float *__restrict__ xyz,
                                                      int32_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= centres) return;
    const int64_t b = w / m;
    const float cx = new_xyz[w * 3 + 0], cy = new_xyz[w * 3 + 1], cz = new_xyz[w * 3 + 2];
    const float *p = xyz + b * n * 3;
    int32_t *out = idx + w * nsample;
    const unsigned long long below = (1ull << lane) - 1ull;
    const Pn2Row row = pn2_ball_walk(p, n, cx, cy, cz, r2, lane, below, nsample, out);
    if (row.cnt > 0) pn2_pad_row(lane, row, nsample, out);   // a row without a hit stays as the caller gave it
}

// ---------------------------------------------------------------- three nearest neighbours ------------------------
// 64 unknown points of one cloud per workgroup, one per lane, against the cloud's m known points: one range for
// pn2_search.h's tile walk, every lane compares, and the merged result is stored as it is.
__global__ __launch_bounds__(256) void pn2_three_nn(int n, int m, int blocks_per_cloud, const float *__restrict__ unknown,
                                                    const float *__restrict__ known, float *__restrict__ dist2,
                                                    int32_t *__restrict__ idx) {
    __shared__ float sk[NN_TILE * 3];
    __shared__ float md[NN_PARTS - 1][3][64];
    __shared__ int mi[NN_PARTS - 1][3][64];
    const int lane = threadIdx.x & 63;
    const int64_t b = blockIdx.x / blocks_per_cloud;
    const int pt = (int)(blockIdx.x % blocks_per_cloud) * 64 + lane;
    const bool ok = pt < n;
    const int64_t u = (b * n + (ok ? pt : 0)) * 3;
    const float ux = unknown[u + 0], uy = unknown[u + 1], uz = unknown[u + 2];
    const NNBest best = nn_walk(known + b * m * 3, m, true, ux, uy, uz, sk, threadIdx.x >> 6, NN_NONE);
    NNResult r;
    if (nn_finish(best, ok, md, mi, r)) {
        dist2[u + 0] = r.d1; dist2[u + 1] = r.d2; dist2[u + 2] = r.d3;
        idx[u + 0] = r.i1; idx[u + 1] = r.i2; idx[u + 2] = r.i3;
    }
}

// ---------------------------------------------------------------- gathers (forward) --------------------------------
// out[b, c, e] = points[b, c, idx[b, e]], e < K: gather_points with K = m, group_points with K = npoints * nsample.
// A thread reads its index once and walks GA_CH channels; stores are coalesced along e.
constexpr int GA_CH = 8;
__global__ __launch_bounds__(256) void pn2_gather(int c, int n, int64_t K, int64_t eblocks, int cchunks,
                                                  const float *__restrict__ points, const int32_t *__restrict__ idx,
                                                  float *__restrict__ out) {
    const int64_t blk = blockIdx.x;
    const int64_t eb = blk % eblocks, rest = blk / eblocks;
    const int cc = (int)(rest % cchunks);
    const int64_t b = rest / cchunks;
    const int64_t e = eb * 256 + threadIdx.x;
    if (e >= K) return;
    const int i = idx[b * K + e];
    const bool ok = (unsigned)i < (unsigned)n;
    const int c1 = min(c, (cc + 1) * GA_CH);
    for (int ch = cc * GA_CH; ch < c1; ++ch) {
        const int64_t row = b * c + ch;
        out[row * K + e] = ok ? points[row * n + i] : 0.f;
    }
}

// out[b, c, p] = (w0 * points[b, c, i0] + w1 * points[b, c, i1]) + w2 * points[b, c, i2]
__global__ __launch_bounds__(256) void pn2_three_interpolate(int c, int m, int n, int64_t eblocks, int cchunks,
                                                             const float *__restrict__ points,
                                                             const int32_t *__restrict__ idx,
                                                             const float *__restrict__ weight, float *__restrict__ out) {
    const int64_t blk = blockIdx.x;
    const int64_t eb = blk % eblocks, rest = blk / eblocks;
    const int cc = (int)(rest % cchunks);
    const int64_t b = rest / cchunks;
    const int64_t e = eb * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t q = (b * n + e) * 3;
    const int i0 = idx[q], i1 = idx[q + 1], i2 = idx[q + 2];
    const float w0 = weight[q], w1 = weight[q + 1], w2 = weight[q + 2];
    const bool o0 = (unsigned)i0 < (unsigned)m, o1 = (unsigned)i1 < (unsigned)m, o2 = (unsigned)i2 < (unsigned)m;
    const int c1 = min(c, (cc + 1) * GA_CH);
    for (int ch = cc * GA_CH; ch < c1; ++ch) {
        const float *row = points + (b * c + ch) * m;
        const float p0 = o0 ? row[i0] : 0.f, p1 = o1 ? row[i1] : 0.f, p2 = o2 ? row[i2] : 0.f;
        out[(b * c + ch) * n + e] = (w0 * p0 + w1 * p1) + w2 * p2;
    }
}

// ---------------------------------------------------------------- the three gradients ------------------------------
// grad[b, c, idx[b, e]] += go[b, c, e / D] * (WEIGHTED ? w[b, e] : 1), e < K   (D = 3 for the interpolation, else 1).
// 64 lanes of such an add hit 64 different addresses of one (b, c) row, the slowest shape for global float atomics.  A
// workgroup therefore accumulates R whole rows in LDS (ds_add_f32), reading idx once for all R of them, and then adds
// the rows to the output with plain coalesced read-modify-writes: rows (b, c0 .. c0 + R) are one contiguous range that
// no other workgroup touches.  With too few (b, channel chunk) pairs to fill the device (the coordinates' C = 3) the
// terms are split over `ksplit` workgroups per pair, which then add their rows with global atomics, coalesced along
// the row.  An element no term reaches is not written at all.
template <int LDS_FLOATS, bool WEIGHTED>
__global__ __launch_bounds__(512) void pn2_scatter_rows(int c, int n, int64_t K, int R, int cchunks, int ksplit,
                                                        const float *__restrict__ go, const int32_t *__restrict__ idx,
                                                        const float *__restrict__ weight, float *__restrict__ grad) {
    __shared__ float acc[LDS_FLOATS];
    constexpr int D = WEIGHTED ? 3 : 1;
    const int ks = (int)(blockIdx.x % ksplit);
    const int cc = (int)((blockIdx.x / ksplit) % cchunks);
    const int64_t b = blockIdx.x / ksplit / cchunks;
    const int c0 = cc * R, rows = min(R, c - c0);
    const int total = rows * n;
    for (int i = threadIdx.x; i < total; i += 512) acc[i] = 0.f;
    __syncthreads();
    const int64_t Kg = K / D;
    const float *g0 = go + (b * c + c0) * Kg;
    const int64_t per = (K + ksplit - 1) / ksplit, e1 = min(K, (ks + 1) * per);
    for (int64_t e = ks * per + threadIdx.x; e < e1; e += 512) {
        const int i = idx[b * K + e];
        if ((unsigned)i >= (unsigned)n) continue;
        const int64_t eg = WEIGHTED ? e / 3 : e;
        const float w = WEIGHTED ? weight[b * K + e] : 1.f;
        for (int r = 0; r < rows; ++r) {
            const float g = g0[r * Kg + eg];
            atomicAdd(&acc[r * n + i], WEIGHTED ? g * w : g);
        }
    }
    __syncthreads();
    float *dst = grad + (b * c + c0) * n;
    for (int i = threadIdx.x; i < total; i += 512) {
        const float a = acc[i];
        if (a == 0.f) continue;
        if (ksplit > 1)
            atomicAdd(&dst[i], a);   // several workgroups share the rows: consecutive lanes, consecutive addresses
        else
            dst[i] += a;
    }
}

// rows longer than the LDS holds: global float atomics, a thread per term walking the channels
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void pn2_scatter_atomic(int c, int n, int64_t K, int64_t eblocks, int cchunks,
                                                          const float *__restrict__ go, const int32_t *__restrict__ idx,
                                                          const float *__restrict__ weight, float *__restrict__ grad) {
    constexpr int D = WEIGHTED ? 3 : 1;
    const int64_t blk = blockIdx.x;
    const int64_t eb = blk % eblocks, rest = blk / eblocks;
    const int cc = (int)(rest % cchunks);
    const int64_t b = rest / cchunks;
    const int64_t e = eb * 256 + threadIdx.x;
    if (e >= K) return;
    const int i = idx[b * K + e];
    if ((unsigned)i >= (unsigned)n) return;
    const int64_t Kg = K / D, eg = e / D;
    const float w = WEIGHTED ? weight[b * K + e] : 1.f;
    const int c1 = min(c, (cc + 1) * GA_CH);
    for (int ch = cc * GA_CH; ch < c1; ++ch) {
        const float g = go[(b * c + ch) * Kg + eg];
        atomicAdd(&grad[(b * c + ch) * n + i], WEIGHTED ? g * w : g);
    }
}

constexpr int SC_SMALL = 8192, SC_LARGE = 36864;   // 32 KB (several workgroups per CU) and 144 KB of the CU's 160 KB
constexpr int SC_MAX_ROWS = 16;
constexpr int SC_FILL = 256, SC_MIN_TERMS = 4096;

template <bool WEIGHTED>
int scatter_launch(int b, int c, int n, int64_t K, const float *go, const int32_t *idx, const float *weight, float *grad,
                   void *stream) {
    if (b == 0 || c == 0 || n == 0 || K == 0) return MODEST_OK;
    if (n <= SC_LARGE) {
        const int cap = n <= SC_SMALL ? SC_SMALL : SC_LARGE;
        const int R = std::min(std::min(SC_MAX_ROWS, cap / n), c);
        const int cchunks = (c + R - 1) / R;
        const int64_t pairs = (int64_t)b * cchunks;
        int ksplit = 1;   // at least SC_MIN_TERMS terms per workgroup, about one workgroup per CU
        if (pairs < SC_FILL) ksplit = (int)std::max<int64_t>(1, std::min<int64_t>((SC_FILL + pairs - 1) / pairs, K / SC_MIN_TERMS));
        const int64_t blocks = pairs * ksplit;
        MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
        if (cap == SC_SMALL)
            pn2_scatter_rows<SC_SMALL, WEIGHTED><<<(unsigned)blocks, 512, 0, as_stream(stream)>>>(c, n, K, R, cchunks, ksplit, go, idx, weight, grad);
        else
            pn2_scatter_rows<SC_LARGE, WEIGHTED><<<(unsigned)blocks, 512, 0, as_stream(stream)>>>(c, n, K, R, cchunks, ksplit, go, idx, weight, grad);
    } else {
        const int64_t eblocks = (K + 255) / 256;
        const int cchunks = (c + GA_CH - 1) / GA_CH;
        const int64_t blocks = (int64_t)b * cchunks * eblocks;
        MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
        pn2_scatter_atomic<WEIGHTED><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(c, n, K, eblocks, cchunks, go, idx, weight, grad);
    }
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

int gather_launch(int b, int c, int n, int64_t K, const float *points, const int32_t *idx, float *out, void *stream) {
    if (b == 0 || c == 0 || K == 0) return MODEST_OK;
    const int64_t eblocks = (K + 255) / 256;
    const int cchunks = (c + GA_CH - 1) / GA_CH;
    const int64_t blocks = (int64_t)b * cchunks * eblocks;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    pn2_gather<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(c, n, K, eblocks, cchunks, points, idx, out);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

}  // namespace

extern "C" int modest_pn2_furthest_point_sample(int b, int n, int m, const float *xyz_dev, float *temp_dev,
                                                int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && n >= 1 && m >= 0, "bad sizes");
    if (b == 0 || m == 0) return MODEST_OK;
    MODEST_REQUIRE(xyz_dev && temp_dev && idx_dev, "NULL buffer");
    // the reference's block size (opt_n_threads): the largest power of two <= n, at most 1024; it fixes the tie order
    int L = 0;
    while (L < 10 && (2 << L) <= n) ++L;
    int S = 0;
    while (((unsigned)(n - 1) >> L) >> S) ++S;
    hipStream_t st = as_stream(stream);
    if (n <= 512)
        pn2_fps_reg<1, 8><<<b, 64, 0, st>>>(n, m, L, S, xyz_dev, temp_dev, idx_dev);
    else if (n <= 1024)
        pn2_fps_reg<4, 4><<<b, 256, 0, st>>>(n, m, L, S, xyz_dev, temp_dev, idx_dev);
    else if (n <= 4096)
        pn2_fps_reg<16, 4><<<b, 1024, 0, st>>>(n, m, L, S, xyz_dev, temp_dev, idx_dev);
    else if (n <= 12288)
        pn2_fps_reg<16, 12><<<b, 1024, 0, st>>>(n, m, L, S, xyz_dev, temp_dev, idx_dev);
    else
        pn2_fps_global<<<b, 1024, 0, st>>>(n, m, L, S, xyz_dev, temp_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2_gather(int b, int c, int n, int m, const float *points_dev, const int32_t *idx_dev,
                                 float *out_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0, "negative size");
    return gather_launch(b, c, n, m, points_dev, idx_dev, out_dev, stream);
}

extern "C" int modest_pn2_gather_grad(int b, int c, int n, int m, const float *grad_out_dev, const int32_t *idx_dev,
                                      float *grad_points_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0, "negative size");
    return scatter_launch<false>(b, c, n, m, grad_out_dev, idx_dev, nullptr, grad_points_dev, stream);
}

extern "C" int modest_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz_dev,
                                     const float *xyz_dev, int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && n >= 0 && m >= 0 && nsample >= 0, "negative size");
    const int64_t centres = (int64_t)b * m;
    if (centres == 0 || nsample == 0 || n == 0) return MODEST_OK;
    const int64_t blocks = (centres + 3) / 4;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    const float r2 = radius * radius;
    pn2_ball_query<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(centres, n, m, r2, nsample, new_xyz_dev, xyz_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2_group(int b, int c, int n, int npoints, int nsample, const float *points_dev,
                                const int32_t *idx_dev, float *out_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0, "negative size");
    return gather_launch(b, c, n, (int64_t)npoints * nsample, points_dev, idx_dev, out_dev, stream);
}

extern "C" int modest_pn2_group_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out_dev,
                                     const int32_t *idx_dev, float *grad_points_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0, "negative size");
    return scatter_launch<false>(b, c, n, (int64_t)npoints * nsample, grad_out_dev, idx_dev, nullptr, grad_points_dev, stream);
}

extern "C" int modest_pn2_three_nn(int b, int n, int m, const float *unknown_dev, const float *known_dev,
                                   float *dist2_dev, int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && n >= 0 && m >= 0, "negative size");
    if (b == 0 || n == 0) return MODEST_OK;
    const int bpc = (n + 63) / 64;
    const int64_t blocks = (int64_t)b * bpc;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    pn2_three_nn<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(n, m, bpc, unknown_dev, known_dev, dist2_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2_three_interpolate(int b, int c, int m, int n, const float *points_dev, const int32_t *idx_dev,
                                            const float *weight_dev, float *out_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0, "negative size");
    if (b == 0 || c == 0 || n == 0) return MODEST_OK;
    const int64_t eblocks = ((int64_t)n + 255) / 256;
    const int cchunks = (c + GA_CH - 1) / GA_CH;
    const int64_t blocks = (int64_t)b * cchunks * eblocks;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    pn2_three_interpolate<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(c, m, n, eblocks, cchunks, points_dev, idx_dev, weight_dev, out_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out_dev,
                                                 const int32_t *idx_dev, const float *weight_dev,
                                                 float *grad_points_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0, "negative size");
    return scatter_launch<true>(b, c, m, (int64_t)n * 3, grad_out_dev, idx_dev, weight_dev, grad_points_dev, stream);
}
