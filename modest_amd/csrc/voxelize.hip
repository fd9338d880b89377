// Point-to-voxel grouping (spconv 1.2 hard voxelisation, first come first served) for PointPillars, on the host and on gfx950.
// Four entry points (include/modest_hip.h, "a24"); the contract is DESIGN.md section 7f:
//   * modest_voxelize_host            -- one cloud, sequential, pure host code (DataLoader workers): no HIP call
//   * modest_voxelize_workspace_bytes -- scratch of the device path, a function of the row count and the batch capacity only
//   * modest_voxelize_plan            -- a collated batch on the device up to the per-cloud voxel counts (one synchronise)
//   * modest_voxelize_fill            -- writes the four outputs (enqueue only)
//
// The cell of a point, on both paths: c_j = floorf((p_j - lo_j) / vs_j) in float32 (one rounding for the difference, one
// correctly rounded division, no reciprocal), kept iff 0 <= c_j < (float)grid_j on the FLOAT for all three axes (NaN and
// +-inf fail, -0.0 is cell 0), converted to integer only then.
//
// The device path has no table over the grid and nothing in it depends on the order in which atomics land:
//   1. key(i) = (b << bits_cell) | cell, or (batch_cap << bits_cell) for a dropped point; the same kernel finds the first
//      row of every cloud and reports a batch column that is not a non-decreasing sequence of integers in [0, batch_cap).
//   2. stable LSD radix sort of (key, i), 8 bits per pass over the bits in use only (sort64.hip has the scheme).
//   3. the first row of a run of equal keys is the cell's first point (the sort is stable): flag[i] = 1 there.
//   4. exclusive scan of the flags in ROW order = the number of cells opened before row i.  Taken at a cell's first point
//      it is the cell's voxel number over the batch, minus the value at the cloud's first row the number within the cloud;
//      numbers >= max_voxels are rejected with all their points.  V_b = min(cells of cloud b, max_voxels).
//   5. fill: one wavefront per opened cell; slot = position in the run, kept if < max_num_points; the wavefront writes
//      the whole voxel row (padding included), its coordinates, its count and its row of point indices.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "common.h"
#include "modest_hip.h"
#include "sort64.h"

namespace {

constexpr int64_t VX_MAX_CELLS = 2147483647;
constexpr int64_t VX_MAX_ROWS = 2147483647 - 4096;
constexpr int VX_BATCH_MAX = 4096;
constexpr int VX_SCAN_T = 1024;   // rows per block of the flag scan
constexpr int VX_HDR_WORDS = 64;   // [0] error bits, [1] clouds seen (last batch index + 1)
constexpr int VX_ERR_ORDER = 1, VX_ERR_BATCH = 2;
constexpr int VX_FILL_T = 256;

struct VxGeom {
    float lo[3], vs[3], gf[3];
    int g[3];
};

// the carve of the workspace: a function of the row count and the batch capacity, never of the grid
struct VxLayout {
    int64_t flag_blocks;
    size_t hdr, start, rbase, obase, key_a, key_b, idx_a, idx_b, table, rank, bsum, headpos, bytes;
};

inline VxLayout vx_layout(int64_t n, int batch_cap) {
    VxLayout L;
    L.flag_blocks = (n + VX_SCAN_T - 1) / VX_SCAN_T;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += arena_sz(bytes);
        return at;
    };
    L.hdr = take(sizeof(int32_t) * VX_HDR_WORDS);
    L.start = take(sizeof(int32_t) * ((size_t)batch_cap + 2));
    L.rbase = take(sizeof(int32_t) * ((size_t)batch_cap + 2));
    L.obase = take(sizeof(int32_t) * ((size_t)batch_cap + 2));
    L.key_a = take(sizeof(uint64_t) * (size_t)n);
    L.key_b = take(sizeof(uint64_t) * (size_t)n);
    L.idx_a = take(sizeof(uint32_t) * (size_t)n);
    L.idx_b = take(sizeof(uint32_t) * (size_t)n);
    L.table = take(sizeof(uint32_t) * sort64_table_words(n));
    L.rank = take(sizeof(int32_t) * (size_t)n);
    L.bsum = take(sizeof(uint32_t) * ((size_t)L.flag_blocks + 1));
    L.headpos = take(sizeof(int32_t) * (size_t)n);
    L.bytes = off;
    return L;
}

// bits of a cell number, bits of the whole key ((batch_cap << bits_cell) is the key of a dropped point)
struct VxBits {
    int cell, all;
};
inline VxBits vx_bits(int64_t cells, int batch_cap) {
    VxBits b;
    b.cell = sort64_bit_length((uint64_t)(cells - 1));
    b.all = b.cell + sort64_bit_length((uint64_t)batch_cap);
    return b;
}

// the shared argument checks; *cells_out = cells per cloud
int vx_check_geom(const float *lo3, const float *vs3, const int32_t *grid3, int64_t *cells_out) {
    MODEST_REQUIRE(lo3 && vs3 && grid3, "NULL geometry");
    MODEST_REQUIRE(grid3[0] >= 1 && grid3[1] >= 1 && grid3[2] >= 1, "a grid of no cells");
    // 2^31 - 1 cells at the most: the product is formed in steps that cannot overflow 64 bits
    const int64_t xy = (int64_t)grid3[0] * grid3[1];
    MODEST_REQUIRE(xy <= VX_MAX_CELLS && xy * (int64_t)grid3[2] <= VX_MAX_CELLS, "more than 2^31 - 1 cells per cloud");
    *cells_out = xy * (int64_t)grid3[2];
    return MODEST_OK;
}

VxGeom vx_geom(const float *lo3, const float *vs3, const int32_t *grid3) {
    VxGeom g;
    for (int j = 0; j < 3; ++j) {
        g.lo[j] = lo3[j];
        g.vs[j] = vs3[j];
        g.g[j] = grid3[j];
        g.gf[j] = (float)grid3[j];
    }
    return g;
}

__device__ __forceinline__ int vx_batch_index(float bf, int batch_cap) {
    return (bf >= 0.f && bf < (float)batch_cap && bf == floorf(bf)) ? (int)bf : -2;   // NaN fails the first test
}

// ---------------------------------------------------------------- 1. keys, cloud starts, order check -------------------
__global__ __launch_bounds__(256) void vx_keys(const float *__restrict__ pts, int n, int stride, VxGeom g, int batch_cap,
                                               int bits_cell, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                               int32_t *__restrict__ start, int32_t *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *r = pts + i * stride;
    const int bi = vx_batch_index(r[0], batch_cap);
    if (bi < 0) {
        atomicOr(&hdr[0], VX_ERR_BATCH);
    } else {
        const int prev = i > 0 ? vx_batch_index(pts[(i - 1) * stride], batch_cap) : -1;
        if (prev >= -1) {   // (an invalid predecessor reports itself)
            if (bi < prev) atomicOr(&hdr[0], VX_ERR_ORDER);
            for (int b = prev + 1; b <= bi; ++b) start[b] = (int32_t)i;   // clouds prev+1 .. bi-1 are empty
        }
        if (i == n - 1) {
            for (int b = bi + 1; b <= batch_cap; ++b) start[b] = n;
            hdr[1] = bi + 1;
        }
    }
    bool in = bi >= 0;
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c[j] = floorf((r[1 + j] - g.lo[j]) / g.vs[j]);
        in = in && (c[j] >= 0.f && c[j] < g.gf[j]);
    }
    uint64_t key = (uint64_t)batch_cap << bits_cell;
    if (in) {
        const int64_t cell = ((int64_t)c[2] * g.g[1] + (int64_t)c[1]) * g.g[0] + (int64_t)c[0];
        key = ((uint64_t)bi << bits_cell) | (uint64_t)cell;
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// ---------------------------------------------------------------- 3./4. first points, voxel numbers --------------------
__device__ __forceinline__ bool vx_is_head(const uint64_t *__restrict__ sk, int64_t p, int batch_cap, int bits_cell) {
    const uint64_t key = sk[p];
    if ((int)(key >> bits_cell) >= batch_cap) return false;   // dropped
    return p == 0 || sk[p - 1] != key;
}

__global__ __launch_bounds__(256) void vx_flags(const uint64_t *__restrict__ sk, const uint32_t *__restrict__ si, int n,
                                                int batch_cap, int bits_cell, int32_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = si[p];
    if (i < (uint32_t)n) flag[i] = vx_is_head(sk, p, batch_cap, bits_cell) ? 1 : 0;   // si is a permutation: every row written
}

__global__ __launch_bounds__(VX_SCAN_T) void vx_flag_sums(const int32_t *__restrict__ flag, int n, uint32_t *__restrict__ bsum) {
    const int64_t i = (int64_t)blockIdx.x * VX_SCAN_T + threadIdx.x;
    const int c = __syncthreads_count(i < n && flag[i] != 0);
    if (threadIdx.x == 0) bsum[blockIdx.x] = (unsigned)c;
}

// flag -> exclusive rank, in place (a thread reads its own word before the barrier and writes it after)
__global__ __launch_bounds__(VX_SCAN_T) void vx_ranks(int32_t *__restrict__ flag_rank, int n, const uint32_t *__restrict__ bsum) {
    __shared__ unsigned ws[VX_SCAN_T / 64];
    const int64_t i = (int64_t)blockIdx.x * VX_SCAN_T + threadIdx.x;
    const unsigned r = sort64_block_rank(i < n && flag_rank[i] != 0, bsum + blockIdx.x, ws);
    if (i < n) flag_rank[i] = (int32_t)r;
}

__global__ __launch_bounds__(256) void vx_headpos(const uint64_t *__restrict__ sk, const uint32_t *__restrict__ si, int n,
                                                  int batch_cap, int bits_cell, const int32_t *__restrict__ rank,
                                                  int32_t *__restrict__ headpos) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n || !vx_is_head(sk, p, batch_cap, bits_cell)) return;
    const uint32_t i = si[p];
    if (i >= (uint32_t)n) return;
    const int32_t r = rank[i];
    if (r >= 0 && r < n) headpos[r] = (int32_t)p;
}

// one workgroup: the voxel number at every cloud's first row, the counts V_b and the output bases; the answer goes
// straight into the caller's pinned words: [0] error bits, [1] clouds seen, [2] cells opened, [3] sum of V_b, [4 + b] V_b
__global__ __launch_bounds__(256) void vx_plan(const int32_t *__restrict__ start, const int32_t *__restrict__ rank,
                                               const uint32_t *__restrict__ total_p, int n, int batch_cap, int m,
                                               int32_t *__restrict__ rbase, int32_t *__restrict__ obase,
                                               const int32_t *__restrict__ hdr, int32_t *__restrict__ pinned) {
    const int err = hdr[0];
    if (err) {   // (uniform over the workgroup) no cloud start can be trusted
        if (threadIdx.x == 0) {
            pinned[1] = pinned[2] = pinned[3] = 0;
            pinned[0] = err;
        }
        return;
    }
    const int total = (int)*total_p;
    for (int b = threadIdx.x; b <= batch_cap; b += 256) {
        const int s = start[b];
        rbase[b] = (s >= 0 && s < n) ? rank[s] : total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int b = 0; b < batch_cap; ++b) {
            const int u = rbase[b + 1] - rbase[b];
            const int v = u < 0 ? 0 : (u < m ? u : m);
            obase[b] = acc;
            pinned[4 + b] = v;
            acc += v;
        }
        obase[batch_cap] = acc;
        pinned[0] = 0;
        pinned[1] = hdr[1];
        pinned[2] = total;
        pinned[3] = acc;
    }
}

// ---------------------------------------------------------------- 5. fill ----------------------------------------------
__global__ __launch_bounds__(VX_FILL_T) void vx_fill(const uint32_t *__restrict__ pts, int n, int c, int batch_cap, int bits_cell,
                                                     int gx, int gy, int p_max, int m, const uint64_t *__restrict__ sk,
                                                     const uint32_t *__restrict__ si, const int32_t *__restrict__ headpos,
                                                     const int32_t *__restrict__ rbase, const int32_t *__restrict__ obase,
                                                     int opened, int64_t total_voxels, uint32_t *__restrict__ voxels,
                                                     int32_t *__restrict__ coords, int32_t *__restrict__ num,
                                                     int32_t *__restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (VX_FILL_T / 64) + (threadIdx.x >> 6);
    if (r >= opened) return;   // (whole wavefronts leave together: r is per wavefront)
    const int64_t p = headpos[r];
    if (p < 0 || p >= n) return;
    const uint64_t key = sk[p];
    const int b = (int)(key >> bits_cell);
    if (b < 0 || b >= batch_cap) return;
    const int64_t local = r - rbase[b];
    if (local < 0 || local >= m) return;   // the cloud's voxels are full: the cell and all its points are dropped
    const int64_t row = (int64_t)obase[b] + local;
    if (row >= total_voxels) return;
    // the run of this key from p on, at most p_max long
    int cnt = 0;
    for (int s0 = 0; s0 < p_max; s0 += 64) {
        const int64_t q = p + s0 + lane;
        const bool ok = s0 + lane < p_max && q < n && sk[q] == key;
        const unsigned long long bal = __ballot(ok);
        cnt += __popcll(bal);
        if (bal != ~0ull) break;
    }
    if (lane == 0) {
        const uint64_t cell = key & ((1ull << bits_cell) - 1ull);
        const uint64_t zy = cell / (uint64_t)gx;
        coords[row * 4 + 0] = b;
        coords[row * 4 + 1] = (int32_t)(zy / (uint64_t)gy);
        coords[row * 4 + 2] = (int32_t)(zy % (uint64_t)gy);
        coords[row * 4 + 3] = (int32_t)(cell % (uint64_t)gx);
        num[row] = cnt;
    }
    const int stride = 1 + c;
    for (int s = lane; s < p_max; s += 64) mask[row * p_max + s] = s < cnt ? (int32_t)si[p + s] : -1;
    const int64_t words = (int64_t)p_max * c;
    uint32_t *out = voxels + row * words;
    int s = lane / c, col = lane % c;
    const int ds = 64 / c, dcol = 64 % c;
    for (int64_t e = lane; e < words; e += 64) {   // raw 32-bit words: NaN payloads survive
        out[e] = s < cnt ? pts[(int64_t)si[p + s] * stride + 1 + col] : 0u;
        s += ds;
        col += dcol;
        if (col >= c) { col -= c; ++s; }
    }
}

}  // namespace

extern "C" int64_t modest_voxelize_workspace_bytes(int64_t n_rows, int batch_cap, const int32_t *grid3_host) {
    int64_t cells = 0;
    const int32_t one[3] = {1, 1, 1};
    const float zero[3] = {0.f, 0.f, 0.f};
    if (vx_check_geom(zero, zero, grid3_host ? grid3_host : one, &cells) != MODEST_OK) return MODEST_ERR_ARG;
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= VX_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(batch_cap >= 1 && batch_cap <= VX_BATCH_MAX, "batch capacity out of range (1 .. 4096)");
    return (int64_t)vx_layout(n_rows, batch_cap).bytes;
}

extern "C" int modest_voxelize_plan(const float *points_dev, int64_t n_rows, int c, int batch_cap, const float *lo3_host,
                                    const float *vs3_host, const int32_t *grid3_host, int max_num_points, int max_voxels,
                                    void *workspace_dev, int64_t workspace_bytes, int32_t *counts_pinned_host, void *stream) {
    int64_t cells = 0;
    if (int rc = vx_check_geom(lo3_host, vs3_host, grid3_host, &cells)) return rc;
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= VX_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(c >= 3 && c <= 4096, "a row is the batch index and at least x, y, z");
    MODEST_REQUIRE(batch_cap >= 1 && batch_cap <= VX_BATCH_MAX, "batch capacity out of range (1 .. 4096)");
    MODEST_REQUIRE(max_num_points >= 1 && max_voxels >= 1, "max_num_points and max_voxels must be positive");
    MODEST_REQUIRE(counts_pinned_host, "NULL counts");
    if (n_rows == 0) {
        memset(counts_pinned_host, 0, sizeof(int32_t) * (4 + (size_t)batch_cap));
        return MODEST_OK;
    }
    const VxLayout L = vx_layout(n_rows, batch_cap);
    MODEST_REQUIRE(points_dev && workspace_dev, "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)L.bytes, "workspace smaller than modest_voxelize_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "workspace must be 256-byte aligned");
    const VxBits bits = vx_bits(cells, batch_cap);
    const VxGeom g = vx_geom(lo3_host, vs3_host, grid3_host);
    const hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    int32_t *hdr = reinterpret_cast<int32_t *>(ws + L.hdr), *start = reinterpret_cast<int32_t *>(ws + L.start);
    int32_t *rbase = reinterpret_cast<int32_t *>(ws + L.rbase), *obase = reinterpret_cast<int32_t *>(ws + L.obase);
    uint64_t *key[2] = {reinterpret_cast<uint64_t *>(ws + L.key_a), reinterpret_cast<uint64_t *>(ws + L.key_b)};
    uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + L.idx_a), reinterpret_cast<uint32_t *>(ws + L.idx_b)};
    uint32_t *table = reinterpret_cast<uint32_t *>(ws + L.table), *bsum = reinterpret_cast<uint32_t *>(ws + L.bsum);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + L.rank), *headpos = reinterpret_cast<int32_t *>(ws + L.headpos);
    const int n = (int)n_rows;
    const unsigned row_blocks = (unsigned)((n_rows + 255) / 256);
    MODEST_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(int32_t) * VX_HDR_WORDS, st));
    vx_keys<<<row_blocks, 256, 0, st>>>(points_dev, n, 1 + c, g, batch_cap, bits.cell, key[0], idx[0], start, hdr);
    const int fin = sort64(key, idx, n, bits.all, table, st);
    vx_flags<<<row_blocks, 256, 0, st>>>(key[fin], idx[fin], n, batch_cap, bits.cell, rank);
    vx_flag_sums<<<(unsigned)L.flag_blocks, VX_SCAN_T, 0, st>>>(rank, n, bsum);
    sort64_scan(bsum, L.flag_blocks, st);
    vx_ranks<<<(unsigned)L.flag_blocks, VX_SCAN_T, 0, st>>>(rank, n, bsum);
    vx_headpos<<<row_blocks, 256, 0, st>>>(key[fin], idx[fin], n, batch_cap, bits.cell, rank, headpos);
    vx_plan<<<1, 256, 0, st>>>(start, rank, bsum + L.flag_blocks, n, batch_cap, max_voxels, rbase, obase, hdr, counts_pinned_host);
    MODEST_HIP_CHECK(hipGetLastError());
    MODEST_HIP_CHECK(hipStreamSynchronize(st));
    const int err = counts_pinned_host[0];
    MODEST_REQUIRE(!(err & VX_ERR_BATCH), "the batch column holds a value that is not an integer in [0, batch capacity)");
    MODEST_REQUIRE(!(err & VX_ERR_ORDER), "the batch column is not in non-decreasing order");
    return MODEST_OK;
}

extern "C" int modest_voxelize_fill(const float *points_dev, int64_t n_rows, int c, int batch_cap, const int32_t *grid3_host,
                                    int max_num_points, int max_voxels, const void *workspace_dev, int64_t workspace_bytes,
                                    int32_t cells_opened, int64_t total_voxels, float *voxels_dev, int32_t *coords_dev,
                                    int32_t *num_points_dev, int32_t *point_mask_dev, void *stream) {
    int64_t cells = 0;
    const float zero[3] = {0.f, 0.f, 0.f};
    if (int rc = vx_check_geom(zero, zero, grid3_host, &cells)) return rc;
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= VX_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(c >= 3 && c <= 4096, "a row is the batch index and at least x, y, z");
    MODEST_REQUIRE(batch_cap >= 1 && batch_cap <= VX_BATCH_MAX, "batch capacity out of range (1 .. 4096)");
    MODEST_REQUIRE(max_num_points >= 1 && max_voxels >= 1, "max_num_points and max_voxels must be positive");
    MODEST_REQUIRE(cells_opened >= 0 && cells_opened <= n_rows && total_voxels >= 0 && total_voxels <= cells_opened,
                   "counts that no plan call can have returned");
    if (total_voxels == 0) return MODEST_OK;
    const VxLayout L = vx_layout(n_rows, batch_cap);
    MODEST_REQUIRE(points_dev && workspace_dev && voxels_dev && coords_dev && num_points_dev && point_mask_dev, "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)L.bytes, "workspace smaller than modest_voxelize_workspace_bytes");
    const VxBits bits = vx_bits(cells, batch_cap);
    const char *ws = static_cast<const char *>(workspace_dev);
    const int fin = sort64_result(bits.all);
    const uint64_t *sk = reinterpret_cast<const uint64_t *>(ws + (fin ? L.key_b : L.key_a));
    const uint32_t *si = reinterpret_cast<const uint32_t *>(ws + (fin ? L.idx_b : L.idx_a));
    const int per = VX_FILL_T / 64;
    vx_fill<<<(unsigned)((cells_opened + per - 1) / per), VX_FILL_T, 0, as_stream(stream)>>>(
        reinterpret_cast<const uint32_t *>(points_dev), (int)n_rows, c, batch_cap, bits.cell, grid3_host[0], grid3_host[1],
        max_num_points, max_voxels, sk, si, reinterpret_cast<const int32_t *>(ws + L.headpos),
        reinterpret_cast<const int32_t *>(ws + L.rbase), reinterpret_cast<const int32_t *>(ws + L.obase), cells_opened,
        total_voxels, reinterpret_cast<uint32_t *>(voxels_dev), coords_dev, num_points_dev, point_mask_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

// ---------------------------------------------------------------- the host path ----------------------------------------
// The sequential walk itself.  table[cells]: the voxel number of every cell, -1 = not opened; all -1 on entry, and on
// return again (only the opened cells are reset), so a generator allocates it once.  Rows are written as they open:
// the caller's arrays may be uninitialised, rows [0, V) are complete on return.  No HIP call.
extern "C" int64_t modest_voxelize_host(const float *points, int64_t n, int c, const float *lo3, const float *vs3,
                                        const int32_t *grid3, int max_num_points, int max_voxels, int32_t *table,
                                        float *voxels, int32_t *coords, int32_t *num_points, int32_t *point_mask) {
    int64_t cells = 0;
    if (vx_check_geom(lo3, vs3, grid3, &cells) != MODEST_OK) return MODEST_ERR_ARG;
    MODEST_REQUIRE(n >= 0 && n <= 2147483647 && c >= 3, "rows of at least x, y, z; at most 2^31 - 1 of them");
    MODEST_REQUIRE(max_num_points >= 1 && max_voxels >= 1, "max_num_points and max_voxels must be positive");
    MODEST_REQUIRE(table && voxels && coords && num_points && point_mask && (n == 0 || points), "NULL buffer");
    const VxGeom g = vx_geom(lo3, vs3, grid3);
    const int64_t P = max_num_points, row_words = P * c;
    int32_t v_count = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float *r = points + i * c;
        float cj[3];
        bool in = true;
        for (int j = 0; j < 3; ++j) {
            cj[j] = floorf((r[j] - g.lo[j]) / g.vs[j]);
            in = in && (cj[j] >= 0.f && cj[j] < g.gf[j]);
        }
        if (!in) continue;
        const int32_t x = (int32_t)cj[0], y = (int32_t)cj[1], z = (int32_t)cj[2];
        const int64_t cell = ((int64_t)z * g.g[1] + y) * g.g[0] + x;
        int32_t v = table[cell];
        if (v < 0) {
            if (v_count >= max_voxels) continue;   // the walk goes on: later points of open cells still enter
            v = table[cell] = v_count++;
            coords[(int64_t)v * 3 + 0] = z;
            coords[(int64_t)v * 3 + 1] = y;
            coords[(int64_t)v * 3 + 2] = x;
            num_points[v] = 0;
            memset(voxels + v * row_words, 0, sizeof(float) * (size_t)row_words);
            for (int64_t s = 0; s < P; ++s) point_mask[v * P + s] = -1;
        }
        const int32_t s = num_points[v];
        if (s >= max_num_points) continue;
        memcpy(voxels + v * row_words + (int64_t)s * c, r, sizeof(float) * (size_t)c);   // raw words
        point_mask[v * P + s] = (int32_t)i;
        num_points[v] = s + 1;
    }
    for (int32_t v = 0; v < v_count; ++v)
        table[((int64_t)coords[(int64_t)v * 3] * g.g[1] + coords[(int64_t)v * 3 + 1]) * g.g[0] + coords[(int64_t)v * 3 + 2]] = -1;
    return v_count;
}
