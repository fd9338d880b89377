// Stacked-batch PointNet++ ops of the detector (OpenPCDet pcdet/ops/pointnet2/pointnet2_stack/src/*.cu), hand-written
// for gfx950.  Seven entry points (include/modest_hip.h, "a26"): enqueue only, no synchronise, no context.  Furthest
// point sampling has none of its own: the stack extension's kernel is the batch one (modest_pn2_furthest_point_sample).
//
// The layout: all scans of a batch are rows of ONE (N1 + N2 + ..., C) tensor, the per-scan row counts sit in a DEVICE
// tensor of B int32.  Row p belongs to the first scan b with p < cnt[0] + ... + cnt[b]; rows past the total belong to scan
// B - 1 (the reference's loop); negative counts count as 0.  The rows of the other tensor for that scan are
// [start_b, start_b + cnt_b), clipped to the tensor's real row count.  No count is ever read on the host: a wavefront
// finds its scan with a prefix sum of the counts across its lanes (find_scan), 64 scans per step.
//
// What each result is (the contract):
//   * squared distances are (dx*dx + dy*dy) + dz*dz in float32, no contraction (the build's -ffp-contract=off);
//   * ball query: d2 < radius*radius strict, the FIRST nsample hits in index order as scan-local indices, short rows
//     padded with the first hit, a row without a hit gets idx[0] = -1 and is otherwise left as given;
//   * voxel query: cells in dz, dy, dx order, a cell is rejected only if d2 > radius*radius (equality is a hit), global
//     row indices, the same padding and the same -1; a batch index outside [0, B) and a table entry >= the row count
//     of xyz (the reference reads out of bounds there) are skipped;
//   * three-NN: the three smallest (distance, index) pairs within the row's scan, global indices, unused slots inf and
//     start_b;
//   * group / interpolate: an index outside its range reads as 0, the gradients skip it; gradients add into the buffer
//     they are given with global float atomics (two runs may differ in the last bits), an element no term reaches is
//     not written.
// Every element offset is 64-bit.
// The ball walk, the placing and padding of the hits (both queries) and the tile walk and merge of three-NN are
// pn2_search.h's, shared with the batch layout (pointnet2.hip); the kernels here find a row's scan, and own the -1 of a
// row without a hit and the scan's start added to a three-NN index.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "modest_hip.h"
#include "pn2_search.h"

namespace {

// ---------------------------------------------------------------- the scan of a row --------------------------------
__device__ __forceinline__ int64_t cnt_at(const int32_t *cnt, int k) { return (int64_t)max(cnt[k], 0); }

__device__ __forceinline__ int64_t wave_inclusive_sum(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// scan b of row p, the first row of scan b in the row's own tensor (qstart) and in the other tensor (xstart).
// Called by every lane of a wavefront with the same p; b_total >= 1.
struct ScanPos {
    int b;
    int64_t qstart, xstart;
};
__device__ __forceinline__ ScanPos find_scan(int64_t p, int b_total, const int32_t *__restrict__ cntq,
                                             const int32_t *__restrict__ cntx) {
    const int lane = threadIdx.x & 63;
    ScanPos r = {0, 0, 0};
    int64_t qbase = 0, xbase = 0;
    for (int k0 = 0; k0 < b_total; k0 += 64) {
        const int k = k0 + lane;
        const int64_t cq = k < b_total ? cnt_at(cntq, k) : 0, cx = k < b_total ? cnt_at(cntx, k) : 0;
        const int64_t iq = wave_inclusive_sum(cq, lane), ix = wave_inclusive_sum(cx, lane);
        const bool here = k < b_total && (p < qbase + iq || k == b_total - 1);
        const unsigned long long m = __ballot(here);
        if (m) {
            const int j = __ffsll((long long)m) - 1;
            r.b = k0 + j;
            r.qstart = qbase + __shfl(iq - cq, j);
            r.xstart = xbase + __shfl(ix - cx, j);
            break;
        }
        qbase += __shfl(iq, 63);
        xbase += __shfl(ix, 63);
    }
    return r;
}

// ---------------------------------------------------------------- ball query ---------------------------------------
// A wavefront per centre: pn2_search.h's walk over the points of the centre's scan, so the indices are scan-local.
// Each wavefront resolves its own centre's scan, so a workgroup whose four centres straddle two scans needs no care.
__global__ __launch_bounds__(256) void pn2s_ball_query(int b_total, int64_t m, int64_t n_rows, float r2, int nsample,
                                                       const float *__restrict__ new_xyz,
                                                       const int32_t *__restrict__ new_cnt,
                                                       const float *__restrict__ xyz, const int32_t *__restrict__ xyz_cnt,
                                                       int32_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= m) return;
    const ScanPos sp = find_scan(w, b_total, new_cnt, xyz_cnt);
    const int64_t lo = min(sp.xstart, n_rows);
    const int n = (int)min(cnt_at(xyz_cnt, sp.b), n_rows - lo);
    const float cx = new_xyz[w * 3 + 0], cy = new_xyz[w * 3 + 1], cz = new_xyz[w * 3 + 2];
    const float *p = xyz + lo * 3;
    int32_t *out = idx + w * nsample;
    const unsigned long long below = (1ull << lane) - 1ull;
    const Pn2Row row = pn2_ball_walk(p, n, cx, cy, cz, r2, lane, below, nsample, out);
    if (row.cnt > 0) {
        pn2_pad_row(lane, row, nsample, out);
    } else if (lane == 0) {
        out[0] = -1;
    }
}

// ---------------------------------------------------------------- voxel query --------------------------------------
// A wavefront per query.  The (2rz+1)(2ry+1)(2rx+1) box is first clipped to the grid (the cells cut off are the ones the
// reference skips, so the visiting order of the rest is unchanged); lanes take 64 consecutive cells of the clipped box in
// dz, dy, dx order, and pn2_search.h's placing of the hits keeps the accepted ones in the serial order; the value a
// lane writes is the row its cell holds, not its position.
__global__ __launch_bounds__(256) void pn2s_voxel_query(int64_t m, int b_total, int r1, int r2_, int r3, int nsample,
                                                        float rad2, int rz, int ry, int rx, int64_t n_rows,
                                                        const float *__restrict__ new_xyz, const float *__restrict__ xyz,
                                                        const int32_t *__restrict__ coords,
                                                        const int32_t *__restrict__ table, int32_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= m) return;
    const float qx = new_xyz[w * 3 + 0], qy = new_xyz[w * 3 + 1], qz = new_xyz[w * 3 + 2];
    const int bi = coords[w * 4 + 0];
    const int64_t cz = coords[w * 4 + 1], cy = coords[w * 4 + 2], cx = coords[w * 4 + 3];
    int32_t *out = idx + w * nsample;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t z0 = max(cz - rz, (int64_t)0), z1 = min(cz + rz, (int64_t)r1 - 1);
    const int64_t y0 = max(cy - ry, (int64_t)0), y1 = min(cy + ry, (int64_t)r2_ - 1);
    const int64_t x0 = max(cx - rx, (int64_t)0), x1 = min(cx + rx, (int64_t)r3 - 1);
    Pn2Row row = PN2_NO_HIT;
    if ((unsigned)bi < (unsigned)b_total && z0 <= z1 && y0 <= y1 && x0 <= x1) {
        const int ny = (int)(y1 - y0 + 1), nx = (int)(x1 - x0 + 1);
        const int cells = (int)(z1 - z0 + 1) * ny * nx;   // <= the product the entry point bounded by INT_MAX
        for (int64_t t0 = 0; t0 < cells && row.cnt < nsample; t0 += 64 * PN2_UNROLL) {
            bool hit[PN2_UNROLL];
            int nb[PN2_UNROLL];
#pragma unroll
            for (int u = 0; u < PN2_UNROLL; ++u) {
                const int64_t t = t0 + u * 64 + lane;
                hit[u] = false;
                nb[u] = -1;
                if (t < cells) {
                    const int tt = (int)t, x = tt % nx, yz = tt / nx, y = yz % ny, z = yz / ny;
                    const int64_t off = (((int64_t)bi * r1 + (z0 + z)) * r2_ + (y0 + y)) * r3 + (x0 + x);
                    const int i = table[off];
                    if (i >= 0 && i < n_rows) {
                        const float px = xyz[(int64_t)i * 3 + 0], py = xyz[(int64_t)i * 3 + 1], pz = xyz[(int64_t)i * 3 + 2];
                        const float d2 = ((px - qx) * (px - qx) + (py - qy) * (py - qy)) + (pz - qz) * (pz - qz);
                        hit[u] = !(d2 > rad2);
                        nb[u] = i;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < PN2_UNROLL; ++u) {
                const int v = nb[u];
                row = pn2_place_hits(hit[u], v, [v](int j) { return __shfl(v, j); }, below, nsample, row, out);
            }
        }
    }
    if (row.cnt > 0) {
        pn2_pad_row(lane, row, nsample, out);
    } else if (lane == 0) {
        out[0] = -1;
    }
}

// ---------------------------------------------------------------- three nearest neighbours ------------------------
// 64 unknown rows per workgroup, one per lane, on pn2_search.h's tile walk and merge.  The 64 rows may lie in several
// scans: the workgroup finds the scan of its first row and then walks the scans in order until its last row is behind it,
// one range of known rows per scan; in each only the lanes whose row belongs to the scan compare.  A row belongs to
// exactly one scan, so its best three are from that scan's known rows alone, counted from the scan's first known row:
// my_start makes them global.  The loop conditions around the walk are the same in every lane (the walk has barriers).
__global__ __launch_bounds__(256) void pn2s_three_nn(int b_total, int64_t n, int64_t m_rows,
                                                     const float *__restrict__ unknown,
                                                     const int32_t *__restrict__ unknown_cnt,
                                                     const float *__restrict__ known,
                                                     const int32_t *__restrict__ known_cnt, float *__restrict__ dist2,
                                                     int32_t *__restrict__ idx) {
    __shared__ float sk[NN_TILE * 3];
    __shared__ float md[NN_PARTS - 1][3][64];
    __shared__ int mi[NN_PARTS - 1][3][64];
    const int lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * 64, pt = row0 + lane, last_row = min(n - 1, row0 + 63);
    const bool ok = pt < n;
    const int64_t u = (ok ? pt : row0) * 3;
    const float ux = unknown[u + 0], uy = unknown[u + 1], uz = unknown[u + 2];
    NNBest best = NN_NONE;
    int64_t my_start = 0;
    const ScanPos sp = find_scan(row0, b_total, unknown_cnt, known_cnt);
    int64_t qs = sp.qstart, xs = sp.xstart;
    for (int b = sp.b; b < b_total && qs <= last_row; ++b) {
        const int64_t cq = cnt_at(unknown_cnt, b), cx = cnt_at(known_cnt, b);
        const bool last = b == b_total - 1;
        const bool mine = ok && pt >= qs && (last || pt < qs + cq);
        if (last || (cq > 0 && qs + cq > row0)) {   // the scan holds rows of this workgroup (the same answer in every lane)
            if (mine) my_start = xs;
            const int64_t lo = min(xs, m_rows), kn = min(cx, m_rows - lo);
            best = nn_walk(known + lo * 3, kn, mine, ux, uy, uz, sk, threadIdx.x >> 6, best);
        }
        qs += cq;
        xs += cx;
    }
    NNResult r;
    if (nn_finish(best, ok, md, mi, r)) {
        dist2[u + 0] = r.d1; dist2[u + 1] = r.d2; dist2[u + 2] = r.d3;
        idx[u + 0] = (int32_t)(my_start + r.i1);
        idx[u + 1] = (int32_t)(my_start + r.i2);
        idx[u + 2] = (int32_t)(my_start + r.i3);
    }
}

// ---------------------------------------------------------------- grouping: a transpose ----------------------------
// features (N, C) rows in, out (M, C, nsample): one wavefront (a workgroup of 64) per query row.  A tile of up to
// GP_CH channels x GP_ST samples passes through LDS: it is filled sample by sample, lanes along C (the feature rows are
// read coalesced), and written out along (C, nsample), the order out is stored in (coalesced; with nsample <= GP_ST the
// whole tile is one contiguous range).  The gradient is the same walk backwards: grad_out is read coalesced into the
// tile, and the adds go out as global float atomics with lanes along C.
constexpr int GP_CH = 64, GP_ST = 32, GP_LD = GP_ST + 1;
template <bool GRAD>
__global__ __launch_bounds__(64) void pn2s_group(int b_total, int c_total, int nsample, int64_t n_rows,
                                                 const float *__restrict__ src, const int32_t *__restrict__ feat_cnt,
                                                 const int32_t *__restrict__ idx, const int32_t *__restrict__ idx_cnt,
                                                 float *__restrict__ dst) {
    // forward: src = features (N, C), dst = out (M, C, nsample); gradient: src = grad_out, dst = grad_features
    __shared__ float tile[GP_CH * GP_LD];
    __shared__ int sidx[GP_ST];
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const ScanPos sp = find_scan(p, b_total, idx_cnt, feat_cnt);
    const int64_t lo = min(sp.xstart, n_rows);
    const int64_t n = min(cnt_at(feat_cnt, sp.b), n_rows - lo);
    const float *feat = GRAD ? nullptr : src + lo * c_total;
    float *gfeat = GRAD ? dst + lo * c_total : nullptr;
    const int64_t grouped = p * c_total * nsample;   // the row's (C, nsample) block
    for (int s0 = 0; s0 < nsample; s0 += GP_ST) {
        const int nsc = min(GP_ST, nsample - s0);
        __syncthreads();
        if (lane < nsc) sidx[lane] = idx[p * nsample + s0 + lane];
        for (int c0 = 0; c0 < c_total; c0 += GP_CH) {
            const int chn = min(GP_CH, c_total - c0), total = nsc * chn;
            __syncthreads();
            if (GRAD) {
                for (int e = lane; e < total; e += 64) {
                    const int c = e / nsc, s = e - c * nsc;
                    tile[c * GP_LD + s] = src[grouped + (int64_t)(c0 + c) * nsample + s0 + s];
                }
            } else {
                for (int j = lane; j < total; j += 64) {
                    const int s = j / chn, c = j - s * chn, i = sidx[s];
                    tile[c * GP_LD + s] = (i >= 0 && i < n) ? feat[(int64_t)i * c_total + c0 + c] : 0.f;
                }
            }
            __syncthreads();
            if (GRAD) {
                for (int j = lane; j < total; j += 64) {
                    const int s = j / chn, c = j - s * chn, i = sidx[s];
                    if (i >= 0 && i < n) atomicAdd(&gfeat[(int64_t)i * c_total + c0 + c], tile[c * GP_LD + s]);
                }
            } else {
                for (int e = lane; e < total; e += 64) {
                    const int c = e / nsc, s = e - c * nsc;
                    dst[grouped + (int64_t)(c0 + c) * nsample + s0 + s] = tile[c * GP_LD + s];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- three-interpolate --------------------------------
// out (N, C) = (w0 * f[i0] + w1 * f[i1]) + w2 * f[i2], features (M, C): a thread per output element, lanes along C, so
// the three feature rows are read and the output row is written coalesced; a row's three (idx, weight) pairs are read by
// its C lanes from one address each.  The gradient is the same walk with three global float atomics per element, again
// lanes along C.
template <bool GRAD>
__global__ __launch_bounds__(256) void pn2s_three_interpolate(int64_t total, int c_total, int64_t m_rows,
                                                              const float *__restrict__ src,
                                                              const int32_t *__restrict__ idx,
                                                              const float *__restrict__ weight, float *__restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t p = e / c_total;
    const int c = (int)(e - p * c_total);
    const int i0 = idx[p * 3], i1 = idx[p * 3 + 1], i2 = idx[p * 3 + 2];
    const float w0 = weight[p * 3], w1 = weight[p * 3 + 1], w2 = weight[p * 3 + 2];
    const bool o0 = i0 >= 0 && i0 < m_rows, o1 = i1 >= 0 && i1 < m_rows, o2 = i2 >= 0 && i2 < m_rows;
    if (GRAD) {
        const float g = src[e];
        if (o0) atomicAdd(&dst[(int64_t)i0 * c_total + c], g * w0);
        if (o1) atomicAdd(&dst[(int64_t)i1 * c_total + c], g * w1);
        if (o2) atomicAdd(&dst[(int64_t)i2 * c_total + c], g * w2);
    } else {
        const float f0 = o0 ? src[(int64_t)i0 * c_total + c] : 0.f, f1 = o1 ? src[(int64_t)i1 * c_total + c] : 0.f,
                    f2 = o2 ? src[(int64_t)i2 * c_total + c] : 0.f;
        dst[e] = (w0 * f0 + w1 * f1) + w2 * f2;
    }
}

template <bool GRAD>
int group_launch(int b, int m, int c, int nsample, int n, const float *src, const int32_t *feat_cnt, const int32_t *idx,
                 const int32_t *idx_cnt, float *dst, void *stream) {
    if (m == 0 || c == 0 || nsample == 0) return MODEST_OK;
    MODEST_REQUIRE(b >= 1, "rows without a scan");
    MODEST_REQUIRE(src && feat_cnt && idx && idx_cnt && dst, "NULL buffer");
    pn2s_group<GRAD><<<(unsigned)m, 64, 0, as_stream(stream)>>>(b, c, nsample, n, src, feat_cnt, idx, idx_cnt, dst);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

template <bool GRAD>
int interpolate_launch(int n, int c, int m, const float *src, const int32_t *idx, const float *weight, float *dst,
                       void *stream) {
    if (n == 0 || c == 0) return MODEST_OK;
    MODEST_REQUIRE(src && idx && weight && dst, "NULL buffer");
    const int64_t total = (int64_t)n * c, blocks = (total + 255) / 256;
    MODEST_REQUIRE(blocks <= GRID_MAX, "grid too large");
    pn2s_three_interpolate<GRAD><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(total, c, m, src, idx, weight, dst);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

}  // namespace

extern "C" int modest_pn2s_ball_query(int b, int m, float radius, int nsample, const float *new_xyz_dev,
                                      const int32_t *new_xyz_batch_cnt_dev, const float *xyz_dev,
                                      const int32_t *xyz_batch_cnt_dev, int n, int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && n >= 0 && nsample >= 0, "negative size");
    if (m == 0 || nsample == 0) return MODEST_OK;
    MODEST_REQUIRE(b >= 1, "rows without a scan");
    MODEST_REQUIRE(new_xyz_dev && new_xyz_batch_cnt_dev && xyz_batch_cnt_dev && idx_dev && (xyz_dev || n == 0), "NULL buffer");
    const float r2 = radius * radius;
    pn2s_ball_query<<<(unsigned)((m + 3) / 4), 256, 0, as_stream(stream)>>>(b, m, n, r2, nsample, new_xyz_dev, new_xyz_batch_cnt_dev,
                                                                            xyz_dev, xyz_batch_cnt_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2s_voxel_query(int b, int m, int r1, int r2, int r3, int nsample, float radius, int z_range,
                                       int y_range, int x_range, const float *new_xyz_dev, const float *xyz_dev, int n,
                                       const int32_t *new_coords_dev, const int32_t *point_indices_dev,
                                       int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && n >= 0 && nsample >= 0 && r1 >= 0 && r2 >= 0 && r3 >= 0, "negative size");
    MODEST_REQUIRE(z_range >= 0 && y_range >= 0 && x_range >= 0, "negative range");
    if (m == 0 || nsample == 0) return MODEST_OK;
    MODEST_REQUIRE(new_xyz_dev && new_coords_dev && idx_dev, "NULL buffer");
    const int64_t table = (int64_t)b * r1 * r2 * r3;
    MODEST_REQUIRE((point_indices_dev || table == 0) && (xyz_dev || n == 0), "NULL buffer");
    // the cells of a query's box inside the grid: at most min(2 range + 1, R) per axis
    const int64_t bz = std::min<int64_t>(2 * (int64_t)z_range + 1, r1), by = std::min<int64_t>(2 * (int64_t)y_range + 1, r2),
                  bx = std::min<int64_t>(2 * (int64_t)x_range + 1, r3);
    MODEST_REQUIRE(bz * by <= INT_MAX && bz * by * bx <= INT_MAX, "more than 2^31 - 1 cells per query");
    const float rad2 = radius * radius;
    pn2s_voxel_query<<<(unsigned)((m + 3) / 4), 256, 0, as_stream(stream)>>>(m, b, r1, r2, r3, nsample, rad2, z_range, y_range, x_range, n,
                                                                             new_xyz_dev, xyz_dev, new_coords_dev,
                                                                             point_indices_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2s_three_nn(int b, int n, int m, const float *unknown_dev, const int32_t *unknown_batch_cnt_dev,
                                    const float *known_dev, const int32_t *known_batch_cnt_dev, float *dist2_dev,
                                    int32_t *idx_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && n >= 0 && m >= 0, "negative size");
    if (n == 0) return MODEST_OK;
    MODEST_REQUIRE(b >= 1, "rows without a scan");
    MODEST_REQUIRE(unknown_dev && unknown_batch_cnt_dev && known_batch_cnt_dev && dist2_dev && idx_dev && (known_dev || m == 0),
                   "NULL buffer");
    pn2s_three_nn<<<(unsigned)((n + 63) / 64), 256, 0, as_stream(stream)>>>(b, n, m, unknown_dev, unknown_batch_cnt_dev, known_dev,
                                                                            known_batch_cnt_dev, dist2_dev, idx_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pn2s_group(int b, int m, int c, int nsample, int n, const float *features_dev,
                                 const int32_t *features_batch_cnt_dev, const int32_t *idx_dev,
                                 const int32_t *idx_batch_cnt_dev, float *out_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && c >= 0 && nsample >= 0 && n >= 0, "negative size");
    if (m == 0 || c == 0 || nsample == 0) return MODEST_OK;
    MODEST_REQUIRE(features_dev || n == 0, "NULL buffer");
    // with no feature rows every index reads as 0: any non-NULL pointer serves, nothing is read through it
    return group_launch<false>(b, m, c, nsample, n, features_dev ? features_dev : out_dev, features_batch_cnt_dev, idx_dev,
                               idx_batch_cnt_dev, out_dev, stream);
}

extern "C" int modest_pn2s_group_grad(int b, int m, int c, int n, int nsample, const float *grad_out_dev,
                                      const int32_t *idx_dev, const int32_t *idx_batch_cnt_dev,
                                      const int32_t *features_batch_cnt_dev, float *grad_features_dev, void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && c >= 0 && nsample >= 0 && n >= 0, "negative size");
    if (n == 0) return MODEST_OK;   // no destination row: every term is skipped
    return group_launch<true>(b, m, c, nsample, n, grad_out_dev, features_batch_cnt_dev, idx_dev, idx_batch_cnt_dev,
                              grad_features_dev, stream);
}

extern "C" int modest_pn2s_three_interpolate(int n, int c, int m, const float *features_dev, const int32_t *idx_dev,
                                             const float *weight_dev, float *out_dev, void *stream) {
    MODEST_REQUIRE(n >= 0 && c >= 0 && m >= 0, "negative size");
    MODEST_REQUIRE(features_dev || m == 0 || n == 0 || c == 0, "NULL buffer");
    return interpolate_launch<false>(n, c, m, features_dev ? features_dev : out_dev, idx_dev, weight_dev, out_dev, stream);
}

extern "C" int modest_pn2s_three_interpolate_grad(int n, int c, int m, const float *grad_out_dev, const int32_t *idx_dev,
                                                  const float *weight_dev, float *grad_features_dev, void *stream) {
    MODEST_REQUIRE(n >= 0 && c >= 0 && m >= 0, "negative size");
    if (m == 0) return MODEST_OK;   // no destination row: every term is skipped
    return interpolate_launch<true>(n, c, m, grad_out_dev, idx_dev, weight_dev, grad_features_dev, stream);
}
