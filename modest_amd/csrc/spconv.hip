// Sparse 3-D convolutions for SECOND's VoxelBackBone8x (the part of spconv 1.2 it constructs) on gfx950.
// Six entry points (include/modest_hip.h, "a25"); the contract is DESIGN.md section 7g:
//   * modest_spconv_rulebook_workspace_bytes / _plan / _fill -- output sites and the neighbour maps both ways
//   * modest_spconv_gather_gemm                               -- forward, and the feature gradient on the transposed map
//   * modest_spconv_wgrad_workspace_bytes / modest_spconv_wgrad -- weight and bias gradients
//
// Rulebook.  A site (b, z, y, x) becomes the 64-bit key ((b * D + z) * H + y) * W + x; no table over the grid exists.
//   1. keys of the input rows (a row outside the shape sets an error bit), stable LSD radix sort of (key, row) over the
//      bits in use (sort64.hip), equal neighbours in the sorted keys set the duplicate bit.
//   2. strided only: the candidate output key of every (input, offset) -- o = (i + p - k) / s where that is an integer
//      inside the output shape, the sentinel `cells` otherwise --, sorted; the first of every run of equal keys is an
//      output site, its rank in an exclusive scan its row: rows come out ascending in (b, z, y, x).
//   3. the last kernel writes the error bits and N_out to the caller's pinned words; plan synchronises once.
//   4. fill (enqueue only): nbr[k][o] = the input row at o * s - p + k, nbr_t[k][i] = the output row at (i + p - k) / s,
//      -1 where there is none.  Every axis is tested against its extent BEFORE the key is formed, so a neighbour across a
//      border never lands in the next row, slab or cloud.  A lookup is a binary search in sorted unique keys.
//   A submanifold convolution is the same with s = 1, p = k / 2 and the input sites as the outputs, in input order.
//
// Arithmetic.  out[o][c] = (((+0 + x[nbr_0(o)][0] * w[0][0][c]) + x[..][1] * w[0][1][c]) + ...) over k ascending, absent
// neighbours skipped, ci ascending; product and sum rounded separately (the build has -ffp-contract=off and no fmaf is
// written here), then + bias[c].  Every accumulator lives in one lane's register from start to end: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "common.h"
#include "modest_hip.h"
#include "sort64.h"

namespace {

constexpr int64_t SP_MAX_ROWS = 2147483647 - 4096;
constexpr int SP_KSIZE_MAX = 7;
constexpr int SP_CH_MAX = 128;
constexpr int SP_SCAN_T = 1024;   // rows per block of the head scan
constexpr int SP_HDR_WORDS = 64;   // [0] error bits
constexpr int SP_ERR_RANGE = 1, SP_ERR_DUP = 2;

struct SpGeom {
    int batch, kvol, subm;
    int in[3], out[3], k[3], s[3], p[3];   // axis order z, y, x
    int64_t cells_in, cells_out;           // batch * D * H * W: the sentinel key of either side
};

struct SpLayout {
    int64_t m, flag_blocks;
    size_t hdr, key_a, key_b, idx_a, idx_b, table, in_keys, in_idx, rank, bsum, bytes;
};

// a function of the input rows and the kernel volume only, never of the grid
inline SpLayout sp_layout(int64_t n_in, int kvol, int subm) {
    SpLayout L;
    L.m = subm ? n_in : n_in * kvol;   // rows of the larger of the two sorts
    L.flag_blocks = (L.m + SP_SCAN_T - 1) / SP_SCAN_T;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += arena_sz(bytes);
        return at;
    };
    L.hdr = take(sizeof(int32_t) * SP_HDR_WORDS);
    L.key_a = take(sizeof(uint64_t) * (size_t)L.m);
    L.key_b = take(sizeof(uint64_t) * (size_t)L.m);
    L.idx_a = take(sizeof(uint32_t) * (size_t)n_in);
    L.idx_b = take(sizeof(uint32_t) * (size_t)n_in);
    L.table = take(sizeof(uint32_t) * sort64_table_words(L.m));
    L.in_keys = take(sizeof(uint64_t) * (size_t)n_in);
    L.in_idx = take(sizeof(uint32_t) * (size_t)n_in);
    L.rank = take(sizeof(int32_t) * (size_t)L.m);
    L.bsum = take(sizeof(uint32_t) * ((size_t)L.flag_blocks + 1));
    L.bytes = off;
    return L;
}

// checks the geometry and fills g; the products are formed in steps that cannot overflow 64 bits
int sp_geom(int batch, const int32_t *shape3, const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3, int subm,
            SpGeom *g) {
    MODEST_REQUIRE(shape3 && kernel3 && stride3 && pad3, "NULL geometry");
    MODEST_REQUIRE(batch >= 1 && batch <= (1 << 20), "batch size out of range");
    g->batch = batch;
    g->subm = subm ? 1 : 0;
    g->kvol = 1;
    g->cells_in = g->cells_out = batch;
    for (int j = 0; j < 3; ++j) {
        MODEST_REQUIRE(shape3[j] >= 1 && shape3[j] <= (1 << 24), "spatial extent out of range");
        MODEST_REQUIRE(kernel3[j] >= 1 && kernel3[j] <= SP_KSIZE_MAX, "kernel size out of range (1 .. 7)");
        g->in[j] = shape3[j];
        g->k[j] = kernel3[j];
        if (subm) {
            MODEST_REQUIRE(kernel3[j] % 2 == 1, "a submanifold convolution needs odd kernel sizes");
            g->s[j] = 1;
            g->p[j] = kernel3[j] / 2;
            g->out[j] = shape3[j];
        } else {
            MODEST_REQUIRE(stride3[j] >= 1 && stride3[j] <= 64 && pad3[j] >= 0 && pad3[j] <= 64, "stride or padding out of range");
            g->s[j] = stride3[j];
            g->p[j] = pad3[j];
            const int span = shape3[j] + 2 * pad3[j] - kernel3[j];
            MODEST_REQUIRE(span >= 0, "an output extent <= 0");
            g->out[j] = span / stride3[j] + 1;
        }
        g->kvol *= g->k[j];
        MODEST_REQUIRE(g->cells_in <= ((int64_t)1 << 56) / g->in[j] && g->cells_out <= ((int64_t)1 << 56) / g->out[j],
                       "more than 2^56 cells");
        g->cells_in *= g->in[j];
        g->cells_out *= g->out[j];
    }
    return MODEST_OK;
}

__device__ __forceinline__ void sp_offset(const SpGeom &g, int k, int kk[3]) {
    kk[2] = k % g.k[2];
    const int zy = k / g.k[2];
    kk[1] = zy % g.k[1];
    kk[0] = zy / g.k[1];
}

// ---------------------------------------------------------------- keys --------------------------------------------------
__global__ __launch_bounds__(256) void sp_in_keys(const int32_t *__restrict__ ind, int n, SpGeom g, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ idx, int32_t *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = ind[i * 4], z = ind[i * 4 + 1], y = ind[i * 4 + 2], x = ind[i * 4 + 3];
    uint64_t key = (uint64_t)g.cells_in;
    if (b >= 0 && b < g.batch && z >= 0 && z < g.in[0] && y >= 0 && y < g.in[1] && x >= 0 && x < g.in[2])
        key = (uint64_t)((((int64_t)b * g.in[0] + z) * g.in[1] + y) * g.in[2] + x);
    else
        atomicOr(&hdr[0], SP_ERR_RANGE);
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void sp_dup_check(const uint64_t *__restrict__ sk, int n, uint64_t sentinel,
                                                    int32_t *__restrict__ hdr) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < 1 || p >= n) return;
    if (sk[p] == sk[p - 1] && sk[p] != sentinel) atomicOr(&hdr[0], SP_ERR_DUP);
}

// entry e = i * kvol + k: the key of the output site that reads input i at offset k, or the sentinel
__global__ __launch_bounds__(256) void sp_candidates(const int32_t *__restrict__ ind, int64_t m, SpGeom g,
                                                     uint64_t *__restrict__ cand) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int64_t i = e / g.kvol;
    int kk[3];
    sp_offset(g, (int)(e % g.kvol), kk);
    const int b = ind[i * 4];
    bool ok = b >= 0 && b < g.batch;
    int o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = ind[i * 4 + 1 + j];
        const int t = c + g.p[j] - kk[j];
        ok = ok && c >= 0 && c < g.in[j] && t >= 0 && t % g.s[j] == 0;
        o[j] = t >= 0 ? t / g.s[j] : 0;
        ok = ok && o[j] < g.out[j];
    }
    cand[e] = ok ? (uint64_t)((((int64_t)b * g.out[0] + o[0]) * g.out[1] + o[1]) * g.out[2] + o[2]) : (uint64_t)g.cells_out;
}

// ---------------------------------------------------------------- output sites ------------------------------------------
__device__ __forceinline__ bool sp_is_head(const uint64_t *__restrict__ sk, int64_t p, uint64_t sentinel) {
    const uint64_t key = sk[p];
    return key < sentinel && (p == 0 || sk[p - 1] != key);
}

__global__ __launch_bounds__(SP_SCAN_T) void sp_head_sums(const uint64_t *__restrict__ sk, int m, uint64_t sentinel,
                                                          uint32_t *__restrict__ bsum) {
    const int64_t p = (int64_t)blockIdx.x * SP_SCAN_T + threadIdx.x;
    const int c = __syncthreads_count(p < m && sp_is_head(sk, p, sentinel));
    if (threadIdx.x == 0) bsum[blockIdx.x] = (unsigned)c;
}

// rank[p] = heads before p; a head writes its key to out_keys[rank]
__global__ __launch_bounds__(SP_SCAN_T) void sp_head_ranks(const uint64_t *__restrict__ sk, int m, uint64_t sentinel,
                                                           const uint32_t *__restrict__ bsum, uint64_t *__restrict__ out_keys) {
    __shared__ unsigned ws[SP_SCAN_T / 64];
    const int64_t p = (int64_t)blockIdx.x * SP_SCAN_T + threadIdx.x;
    const bool f = p < m && sp_is_head(sk, p, sentinel);
    const unsigned r = sort64_block_rank(f, bsum + blockIdx.x, ws);
    if (f && r < (unsigned)m) out_keys[r] = sk[p];
}

__global__ void sp_finish(const int32_t *__restrict__ hdr, const uint32_t *__restrict__ total_p, int n_fixed,
                          int32_t *__restrict__ pinned) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int err = hdr[0];
        pinned[1] = err ? 0 : (total_p ? (int32_t)*total_p : n_fixed);
        pinned[0] = err;
    }
}

// ---------------------------------------------------------------- the maps ----------------------------------------------
// position of `key` in the ascending unique keys t[0 .. n), or -1
__device__ __forceinline__ int64_t sp_find(const uint64_t *__restrict__ t, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (t[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && t[lo] == key) ? lo : -1;
}

__device__ __forceinline__ void sp_decode(uint64_t key, const int ext[3], int &b, int c[3]) {
    c[2] = (int)(key % (uint64_t)ext[2]);
    key /= (uint64_t)ext[2];
    c[1] = (int)(key % (uint64_t)ext[1]);
    key /= (uint64_t)ext[1];
    c[0] = (int)(key % (uint64_t)ext[0]);
    b = (int)(key / (uint64_t)ext[0]);
}

__global__ __launch_bounds__(256) void sp_out_indices(const uint64_t *__restrict__ out_keys, int n_out, SpGeom g,
                                                      int32_t *__restrict__ out_ind) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_out) return;
    int b, c[3];
    sp_decode(out_keys[o], g.out, b, c);
    out_ind[o * 4] = b;
    out_ind[o * 4 + 1] = c[0];
    out_ind[o * 4 + 2] = c[1];
    out_ind[o * 4 + 3] = c[2];
}

// nbr[k][o]: grid (blocks over o, k).  The output coordinates come from the input rows (submanifold) or the output keys.
__global__ __launch_bounds__(256) void sp_fill_nbr(const int32_t *__restrict__ ind, const uint64_t *__restrict__ out_keys,
                                                   int n_out, SpGeom g, const uint64_t *__restrict__ in_keys,
                                                   const uint32_t *__restrict__ in_idx, int n_in, int32_t *__restrict__ nbr) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (o >= n_out) return;
    int b, c[3], kk[3];
    if (g.subm) {
        b = ind[o * 4];
        c[0] = ind[o * 4 + 1];
        c[1] = ind[o * 4 + 2];
        c[2] = ind[o * 4 + 3];
    } else {
        sp_decode(out_keys[o], g.out, b, c);
    }
    sp_offset(g, k, kk);
    bool ok = true;
    int q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        q[j] = c[j] * g.s[j] - g.p[j] + kk[j];
        ok = ok && q[j] >= 0 && q[j] < g.in[j];   // per axis, before the key exists
    }
    int32_t row = -1;
    if (ok) {
        const uint64_t key = (uint64_t)((((int64_t)b * g.in[0] + q[0]) * g.in[1] + q[1]) * g.in[2] + q[2]);
        const int64_t pos = sp_find(in_keys, n_in, key);
        if (pos >= 0) {
            const uint32_t r = in_idx[pos];
            if (r < (uint32_t)n_in) row = (int32_t)r;
        }
    }
    nbr[(int64_t)k * n_out + o] = row;
}

// nbr_t[k][i]: the output row that reads input i at offset k
__global__ __launch_bounds__(256) void sp_fill_nbr_t(const int32_t *__restrict__ ind, int n_in, SpGeom g,
                                                     const uint64_t *__restrict__ in_keys, const uint32_t *__restrict__ in_idx,
                                                     const uint64_t *__restrict__ out_keys, int n_out,
                                                     int32_t *__restrict__ nbr_t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n_in) return;
    int kk[3], o[3];
    sp_offset(g, k, kk);
    const int b = ind[i * 4];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int t = ind[i * 4 + 1 + j] + g.p[j] - kk[j];
        ok = ok && t >= 0 && t % g.s[j] == 0;
        o[j] = t >= 0 ? t / g.s[j] : 0;
        ok = ok && o[j] < g.out[j];
    }
    int32_t row = -1;
    if (ok) {
        const uint64_t key = (uint64_t)((((int64_t)b * g.out[0] + o[0]) * g.out[1] + o[1]) * g.out[2] + o[2]);
        if (g.subm) {
            const int64_t pos = sp_find(in_keys, n_in, key);
            if (pos >= 0) {
                const uint32_t r = in_idx[pos];
                if (r < (uint32_t)n_in) row = (int32_t)r;
            }
        } else {
            const int64_t pos = sp_find(out_keys, n_out, key);
            if (pos >= 0) row = (int32_t)pos;
        }
    }
    nbr_t[(int64_t)k * n_in + i] = row;
}

// ---------------------------------------------------------------- gather-GEMM -------------------------------------------
// out[r][n] = sum over k, then m ascending, of in[map[k][r]][m] * W_k[m][n], rows with map < 0 skipped, + bias[n].
// W_k[m][n] = w[(k * w_cin + m) * w_cout + n] (forward: m = ci, n = co) or, transposed, w[(k * w_cin + n) * w_cout + m]
// (feature gradient: m = co, n = ci).  A workgroup owns 64 output rows and all NP >= n_dim columns; a lane owns RPT rows
// x 4 columns in registers.  Per offset and per chunk of 32 input channels the weights and the gathered rows go through
// LDS (24.3 KB at NP = 128).
constexpr int SP_TM = 64, SP_CK = 32;

template <int NP>
__global__ __launch_bounds__(256) void sp_gather_gemm(const float *__restrict__ in, int n_in, int m_dim,
                                                      const float *__restrict__ w, int kvol, int w_cin, int w_cout, int trans,
                                                      const float *__restrict__ bias, const int32_t *__restrict__ map, int n_out,
                                                      int n_dim, float *__restrict__ out) {
    constexpr int CG = NP / 4, RG = 256 / CG, RPT = SP_TM / RG;
    __shared__ __attribute__((aligned(16))) float sW[SP_CK][NP];
    __shared__ float sX[SP_TM][SP_CK + 1];
    __shared__ int sRow[SP_TM];
    const int tid = threadIdx.x, cg = tid % CG, rg = tid / CG, c0 = cg * 4, r0 = rg * RPT;
    const int64_t o0 = (int64_t)blockIdx.x * SP_TM;
    float acc[RPT][4];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
    for (int k = 0; k < kvol; ++k) {
        __syncthreads();   // the rows of the previous offset have been read
        int row = -1;
        if (tid < SP_TM) {
            const int64_t o = o0 + tid;
            if (o < n_out) row = map[(int64_t)k * n_out + o];
            if (row < 0 || row >= n_in) row = -1;
            sRow[tid] = row;
        }
        if (!__syncthreads_or(row >= 0)) continue;   // no row of this tile has a neighbour at k
        unsigned present = 0;
#pragma unroll
        for (int r = 0; r < RPT; ++r) present |= (sRow[r0 + r] >= 0 ? 1u : 0u) << r;
        for (int m0 = 0; m0 < m_dim; m0 += SP_CK) {
            const int mc = m_dim - m0 < SP_CK ? m_dim - m0 : SP_CK;
            __syncthreads();   // the previous chunk has been consumed
            if (trans) {
                for (int e = tid; e < SP_CK * NP; e += 256) {
                    const int n = e / SP_CK, mm = e % SP_CK;
                    sW[mm][n] = (mm < mc && n < n_dim) ? w[((int64_t)k * w_cin + n) * w_cout + m0 + mm] : 0.f;
                }
            } else {
                for (int e = tid; e < SP_CK * NP; e += 256) {
                    const int mm = e / NP, n = e % NP;
                    sW[mm][n] = (mm < mc && n < n_dim) ? w[((int64_t)k * w_cin + m0 + mm) * w_cout + n] : 0.f;
                }
            }
            for (int e = tid; e < SP_TM * SP_CK; e += 256) {
                const int r = e / SP_CK, mm = e % SP_CK;
                const int src = sRow[r];
                sX[r][mm] = (src >= 0 && mm < mc) ? in[(int64_t)src * m_dim + m0 + mm] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int mm = 0; mm < mc; ++mm) {
                const float4 wv = *reinterpret_cast<const float4 *>(&sW[mm][c0]);
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    if ((present >> r) & 1u) {
                        const float xv = sX[r0 + r][mm];
                        acc[r][0] = acc[r][0] + xv * wv.x;
                        acc[r][1] = acc[r][1] + xv * wv.y;
                        acc[r][2] = acc[r][2] + xv * wv.z;
                        acc[r][3] = acc[r][3] + xv * wv.w;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t o = o0 + r0 + r;
        if (o < n_out) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = c0 + j;
                if (n < n_dim) out[o * n_dim + n] = bias ? acc[r][j] + bias[n] : acc[r][j];
            }
        }
    }
}

// ---------------------------------------------------------------- weight and bias gradients -----------------------------
// The output rows are cut into S equal segments, S a function of n_out alone.  partial[s][k][ci][co] is the sum over the
// rows of segment s in ascending order, one accumulator per lane; the second kernel adds the S partials in ascending s.
constexpr int SP_WG_SEG_MAX = 32, SP_WG_SEG_ROWS = 1024, SP_WG_RB = 32;

inline int sp_wgrad_segments(int64_t n_out) {
    const int64_t s = (n_out + SP_WG_SEG_ROWS - 1) / SP_WG_SEG_ROWS;
    return (int)(s < 1 ? 1 : (s > SP_WG_SEG_MAX ? SP_WG_SEG_MAX : s));
}

template <int T>   // a T x T tile of (ci, co); a lane owns (T / 16)^2 of it
__global__ __launch_bounds__(256) void sp_wgrad_partial(const float *__restrict__ x, int n_in, int cin,
                                                        const float *__restrict__ dy, int n_out, int cout,
                                                        const int32_t *__restrict__ nbr, int kvol, int seg_rows, int tiles_co,
                                                        float *__restrict__ partial) {
    constexpr int E = T / 16;
    __shared__ float sX[SP_WG_RB][T + 1];
    __shared__ float sY[SP_WG_RB][T + 1];
    __shared__ int sRow[SP_WG_RB];
    const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
    const int ci0 = (blockIdx.x / tiles_co) * T, co0 = (blockIdx.x % tiles_co) * T;
    const int k = blockIdx.y, s = blockIdx.z;
    const int64_t begin = (int64_t)s * seg_rows;
    const int64_t end = begin + seg_rows < n_out ? begin + seg_rows : n_out;
    float acc[E][E];
#pragma unroll
    for (int a = 0; a < E; ++a)
#pragma unroll
        for (int b = 0; b < E; ++b) acc[a][b] = 0.f;
    for (int64_t base = begin; base < end; base += SP_WG_RB) {
        __syncthreads();
        int row = -1;
        if (tid < SP_WG_RB) {
            const int64_t o = base + tid;
            if (o < end) row = nbr[(int64_t)k * n_out + o];
            if (row < 0 || row >= n_in) row = -1;
            sRow[tid] = row;
        }
        if (!__syncthreads_or(row >= 0)) continue;
        for (int e = tid; e < SP_WG_RB * T; e += 256) {
            const int r = e / T, c = e % T;
            const int src = sRow[r];
            const int64_t o = base + r;
            sX[r][c] = (src >= 0 && ci0 + c < cin) ? x[(int64_t)src * cin + ci0 + c] : 0.f;
            sY[r][c] = (src >= 0 && co0 + c < cout) ? dy[o * cout + co0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < SP_WG_RB; ++r) {
            float xa[E], yb[E];
#pragma unroll
            for (int a = 0; a < E; ++a) xa[a] = sX[r][ty * E + a];
#pragma unroll
            for (int b = 0; b < E; ++b) yb[b] = sY[r][tx * E + b];
#pragma unroll
            for (int a = 0; a < E; ++a)
#pragma unroll
                for (int b = 0; b < E; ++b) acc[a][b] = acc[a][b] + xa[a] * yb[b];
        }
    }
#pragma unroll
    for (int a = 0; a < E; ++a)
#pragma unroll
        for (int b = 0; b < E; ++b) {
            const int ci = ci0 + ty * E + a, co = co0 + tx * E + b;
            if (ci < cin && co < cout) partial[(((int64_t)s * kvol + k) * cin + ci) * cout + co] = acc[a][b];
        }
}

__global__ __launch_bounds__(128) void sp_bias_partial(const float *__restrict__ dy, int n_out, int cout, int seg_rows,
                                                       float *__restrict__ partial) {
    const int co = threadIdx.x, s = blockIdx.x;
    if (co >= cout) return;
    const int64_t begin = (int64_t)s * seg_rows;
    const int64_t end = begin + seg_rows < n_out ? begin + seg_rows : n_out;
    float acc = 0.f;
    for (int64_t o = begin; o < end; ++o) acc = acc + dy[o * cout + co];
    partial[(int64_t)s * cout + co] = acc;
}

__global__ __launch_bounds__(256) void sp_partial_sum(const float *__restrict__ partial, int segments, int64_t count,
                                                      float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float acc = 0.f;
    for (int s = 0; s < segments; ++s) acc = acc + partial[(int64_t)s * count + e];
    out[e] = acc;
}

int sp_check_rows(int64_t n_in, int kvol) {
    MODEST_REQUIRE(n_in >= 0 && n_in <= SP_MAX_ROWS && n_in * (int64_t)kvol <= SP_MAX_ROWS,
                   "input rows times kernel volume out of range");
    return MODEST_OK;
}

}  // namespace

extern "C" int64_t modest_spconv_rulebook_workspace_bytes(int64_t n_in, int kvol, int subm) {
    MODEST_REQUIRE(kvol >= 1 && kvol <= SP_KSIZE_MAX * SP_KSIZE_MAX * SP_KSIZE_MAX, "kernel volume out of range");
    if (sp_check_rows(n_in, kvol) != MODEST_OK) return MODEST_ERR_ARG;
    return (int64_t)sp_layout(n_in, kvol, subm).bytes;
}

extern "C" int modest_spconv_rulebook_plan(const int32_t *indices_dev, int64_t n_in, int batch_size, const int32_t *shape3_host,
                                           const int32_t *kernel3_host, const int32_t *stride3_host, const int32_t *pad3_host,
                                           int subm, void *workspace_dev, int64_t workspace_bytes, int32_t *counts_pinned_host,
                                           void *stream) {
    SpGeom g;
    if (int rc = sp_geom(batch_size, shape3_host, kernel3_host, stride3_host, pad3_host, subm, &g)) return rc;
    if (int rc = sp_check_rows(n_in, g.kvol)) return rc;
    MODEST_REQUIRE(counts_pinned_host, "NULL counts");
    if (n_in == 0) {
        counts_pinned_host[0] = counts_pinned_host[1] = 0;
        return MODEST_OK;
    }
    const SpLayout L = sp_layout(n_in, g.kvol, g.subm);
    MODEST_REQUIRE(indices_dev && workspace_dev, "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)L.bytes, "workspace smaller than modest_spconv_rulebook_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "workspace must be 256-byte aligned");
    const hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    int32_t *hdr = reinterpret_cast<int32_t *>(ws + L.hdr);
    uint64_t *key[2] = {reinterpret_cast<uint64_t *>(ws + L.key_a), reinterpret_cast<uint64_t *>(ws + L.key_b)};
    uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + L.idx_a), reinterpret_cast<uint32_t *>(ws + L.idx_b)};
    uint32_t *table = reinterpret_cast<uint32_t *>(ws + L.table), *bsum = reinterpret_cast<uint32_t *>(ws + L.bsum);
    uint64_t *in_keys = reinterpret_cast<uint64_t *>(ws + L.in_keys);
    uint32_t *in_idx = reinterpret_cast<uint32_t *>(ws + L.in_idx);
    const int n = (int)n_in;
    const unsigned row_blocks = (unsigned)((n_in + 255) / 256);
    MODEST_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(int32_t) * SP_HDR_WORDS, st));
    sp_in_keys<<<row_blocks, 256, 0, st>>>(indices_dev, n, g, key[0], idx[0], hdr);
    const int fin = sort64(key, idx, n, sort64_bit_length((uint64_t)g.cells_in), table, st);
    MODEST_HIP_CHECK(hipMemcpyAsync(in_keys, key[fin], sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    MODEST_HIP_CHECK(hipMemcpyAsync(in_idx, idx[fin], sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    sp_dup_check<<<row_blocks, 256, 0, st>>>(in_keys, n, (uint64_t)g.cells_in, hdr);
    if (g.subm) {
        sp_finish<<<1, 64, 0, st>>>(hdr, nullptr, n, counts_pinned_host);
    } else {
        const int m = (int)L.m;
        sp_candidates<<<(unsigned)((L.m + 255) / 256), 256, 0, st>>>(indices_dev, L.m, g, key[0]);
        const int cf = sort64(key, nullptr, m, sort64_bit_length((uint64_t)g.cells_out), table, st);
        sp_head_sums<<<(unsigned)L.flag_blocks, SP_SCAN_T, 0, st>>>(key[cf], m, (uint64_t)g.cells_out, bsum);
        sort64_scan(bsum, L.flag_blocks, st);
        // the output keys land in the sort's other buffer: ascending, unique, N_out of them
        sp_head_ranks<<<(unsigned)L.flag_blocks, SP_SCAN_T, 0, st>>>(key[cf], m, (uint64_t)g.cells_out, bsum, key[cf ^ 1]);
        sp_finish<<<1, 64, 0, st>>>(hdr, bsum + L.flag_blocks, 0, counts_pinned_host);
    }
    MODEST_HIP_CHECK(hipGetLastError());
    MODEST_HIP_CHECK(hipStreamSynchronize(st));
    const int err = counts_pinned_host[0];
    MODEST_REQUIRE(!(err & SP_ERR_RANGE), "an index row lies outside the batch or the spatial shape");
    MODEST_REQUIRE(!(err & SP_ERR_DUP), "two index rows name the same site (duplicate rows)");
    return MODEST_OK;
}

extern "C" int modest_spconv_rulebook_fill(const int32_t *indices_dev, int64_t n_in, int batch_size, const int32_t *shape3_host,
                                           const int32_t *kernel3_host, const int32_t *stride3_host, const int32_t *pad3_host,
                                           int subm, const void *workspace_dev, int64_t workspace_bytes, int64_t n_out,
                                           int32_t *out_indices_dev, int32_t *nbr_dev, int32_t *nbr_t_dev, void *stream) {
    SpGeom g;
    if (int rc = sp_geom(batch_size, shape3_host, kernel3_host, stride3_host, pad3_host, subm, &g)) return rc;
    if (int rc = sp_check_rows(n_in, g.kvol)) return rc;
    MODEST_REQUIRE(n_out >= 0 && n_out <= n_in * (int64_t)g.kvol && (!g.subm || n_out == n_in),
                   "an output count that no plan call can have returned");
    if (n_in == 0 || n_out == 0) return MODEST_OK;
    const SpLayout L = sp_layout(n_in, g.kvol, g.subm);
    MODEST_REQUIRE(indices_dev && workspace_dev && nbr_dev && nbr_t_dev && (g.subm || out_indices_dev), "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)L.bytes, "workspace smaller than modest_spconv_rulebook_workspace_bytes");
    const hipStream_t st = as_stream(stream);
    const char *ws = static_cast<const char *>(workspace_dev);
    const uint64_t *in_keys = reinterpret_cast<const uint64_t *>(ws + L.in_keys);
    const uint32_t *in_idx = reinterpret_cast<const uint32_t *>(ws + L.in_idx);
    // where plan left the output keys: the buffer the candidate sort did not end in
    const int cf = sort64_result(sort64_bit_length((uint64_t)g.cells_out));
    const uint64_t *out_keys = g.subm ? nullptr : reinterpret_cast<const uint64_t *>(ws + (cf ? L.key_a : L.key_b));
    const int ni = (int)n_in, no = (int)n_out;
    if (!g.subm) sp_out_indices<<<(unsigned)((n_out + 255) / 256), 256, 0, st>>>(out_keys, no, g, out_indices_dev);
    sp_fill_nbr<<<dim3((unsigned)((n_out + 255) / 256), (unsigned)g.kvol), 256, 0, st>>>(indices_dev, out_keys, no, g, in_keys,
                                                                                       in_idx, ni, nbr_dev);
    sp_fill_nbr_t<<<dim3((unsigned)((n_in + 255) / 256), (unsigned)g.kvol), 256, 0, st>>>(indices_dev, ni, g, in_keys, in_idx,
                                                                                        out_keys, no, nbr_t_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_spconv_gather_gemm(const float *in_dev, int64_t n_in, int in_channels, const float *weight_dev, int kvol,
                                         int w_cin, int w_cout, int transposed, const float *bias_dev, const int32_t *map_dev,
                                         int64_t n_out, float *out_dev, void *stream) {
    MODEST_REQUIRE(kvol >= 1 && kvol <= SP_KSIZE_MAX * SP_KSIZE_MAX * SP_KSIZE_MAX, "kernel volume out of range");
    MODEST_REQUIRE(w_cin >= 1 && w_cin <= SP_CH_MAX && w_cout >= 1 && w_cout <= SP_CH_MAX, "channels out of range (1 .. 128)");
    MODEST_REQUIRE(in_channels == (transposed ? w_cout : w_cin), "the input width does not match the weight");
    MODEST_REQUIRE(n_in >= 0 && n_in <= SP_MAX_ROWS && n_out >= 0 && n_out <= SP_MAX_ROWS, "row count out of range");
    if (n_out == 0) return MODEST_OK;
    MODEST_REQUIRE(weight_dev && map_dev && out_dev && (n_in == 0 || in_dev), "NULL buffer");
    const int n_dim = transposed ? w_cin : w_cout;
    const unsigned blocks = (unsigned)((n_out + SP_TM - 1) / SP_TM);
    const hipStream_t st = as_stream(stream);
#define SP_GEMM(NP)                                                                                                          \
    sp_gather_gemm<NP><<<blocks, 256, 0, st>>>(in_dev, (int)n_in, in_channels, weight_dev, kvol, w_cin, w_cout, transposed,  \
                                               bias_dev, map_dev, (int)n_out, n_dim, out_dev)
    if (n_dim <= 16) SP_GEMM(16);
    else if (n_dim <= 32) SP_GEMM(32);
    else if (n_dim <= 64) SP_GEMM(64);
    else SP_GEMM(128);
#undef SP_GEMM
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int64_t modest_spconv_wgrad_workspace_bytes(int64_t n_out, int kvol, int c_in, int c_out) {
    MODEST_REQUIRE(kvol >= 1 && kvol <= SP_KSIZE_MAX * SP_KSIZE_MAX * SP_KSIZE_MAX, "kernel volume out of range");
    MODEST_REQUIRE(c_in >= 1 && c_in <= SP_CH_MAX && c_out >= 1 && c_out <= SP_CH_MAX, "channels out of range (1 .. 128)");
    MODEST_REQUIRE(n_out >= 0 && n_out <= SP_MAX_ROWS, "row count out of range");
    const size_t s = (size_t)sp_wgrad_segments(n_out);
    return (int64_t)(arena_sz(sizeof(float) * s * (size_t)kvol * c_in * c_out) + arena_sz(sizeof(float) * s * c_out));
}

extern "C" int modest_spconv_wgrad(const float *x_dev, int64_t n_in, int c_in, const float *dy_dev, int64_t n_out, int c_out,
                                   const int32_t *nbr_dev, int kvol, void *workspace_dev, int64_t workspace_bytes,
                                   float *dweight_dev, float *dbias_dev, void *stream) {
    const int64_t need = modest_spconv_wgrad_workspace_bytes(n_out, kvol, c_in, c_out);
    if (need < 0) return (int)need;
    MODEST_REQUIRE(n_in >= 0 && n_in <= SP_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(dweight_dev, "NULL buffer");
    const hipStream_t st = as_stream(stream);
    const int64_t count = (int64_t)kvol * c_in * c_out;
    if (n_out == 0) {
        MODEST_HIP_CHECK(hipMemsetAsync(dweight_dev, 0, sizeof(float) * (size_t)count, st));
        if (dbias_dev) MODEST_HIP_CHECK(hipMemsetAsync(dbias_dev, 0, sizeof(float) * (size_t)c_out, st));
        return MODEST_OK;
    }
    MODEST_REQUIRE(dy_dev && nbr_dev && workspace_dev && (n_in == 0 || x_dev), "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= need, "workspace smaller than modest_spconv_wgrad_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "workspace must be 256-byte aligned");
    const int segs = sp_wgrad_segments(n_out);
    const int seg_rows = (int)((n_out + segs - 1) / segs);
    float *partial = static_cast<float *>(workspace_dev);
    float *bpartial = reinterpret_cast<float *>(static_cast<char *>(workspace_dev) + arena_sz(sizeof(float) * (size_t)segs * count));
    const int widest = c_in > c_out ? c_in : c_out;
#define SP_WGRAD(T)                                                                                                          \
    do {                                                                                                                     \
        const int tci = (c_in + T - 1) / T, tco = (c_out + T - 1) / T;                                                       \
        sp_wgrad_partial<T><<<dim3((unsigned)(tci * tco), (unsigned)kvol, (unsigned)segs), 256, 0, st>>>(                    \
            x_dev, (int)n_in, c_in, dy_dev, (int)n_out, c_out, nbr_dev, kvol, seg_rows, tco, partial);                       \
    } while (0)
    if (widest <= 16) SP_WGRAD(16);
    else if (widest <= 32) SP_WGRAD(32);
    else SP_WGRAD(64);
#undef SP_WGRAD
    sp_partial_sum<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(partial, segs, count, dweight_dev);
    if (dbias_dev) {
        sp_bias_partial<<<(unsigned)segs, 128, 0, st>>>(dy_dev, (int)n_out, c_out, seg_rows, bpartial);
        sp_partial_sum<<<1, 256, 0, st>>>(bpartial, segs, c_out, dbias_dev);
    }
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
