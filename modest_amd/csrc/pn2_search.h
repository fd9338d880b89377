// The neighbour searches of pointnet2.hip (batch layout) and pointnet2_stack.hip (stacked layout,
// 7h), the code both bit-for-bit contracts rest on: the order of the hits of a ball / voxel query, the tie order and the
// infinity handling of three-NN.  Device functions only, each inlined into the kernel that calls it; no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

// ---------------------------------------------------------------- hits of a query row, in index order --------------
// A wavefront per row; `below` is the lane's (1 << lane) - 1.  A row's state is the same in every lane and is handed on
// by value (through references to it the compiler moves it to vector registers).
struct Pn2Row { int cnt, first; };   // hits so far; the first hit, -1 before there is one
constexpr Pn2Row PN2_NO_HIT = {0, -1};

// One step of 64 candidates, a lane each: the hits take the places cnt, cnt + 1, ... of out in lane order, as far as
// they are below nsample.  first_of(j) is the value of lane j, asked once, for the row's first hit.  (`hit` by
// reference: a step's flags then stay the bytes their array holds, as when the step is written out in the kernel.)
template <class FirstOf>
__device__ __forceinline__ Pn2Row pn2_place_hits(const bool &hit, int value, FirstOf first_of, unsigned long long below,
                                                 int nsample, Pn2Row row, int32_t *out) {
    const unsigned long long mask = __ballot(hit);
    if (mask && row.cnt < nsample) {
        if (row.first < 0) row.first = first_of(__ffsll((long long)mask) - 1);
        const int pos = row.cnt + __popcll(mask & below);
        if (hit && pos < nsample) out[pos] = value;
        row.cnt += __popcll(mask);
    }
    return row;
}

// A short row is filled up with its first hit.  What a row without a hit gets is the caller's: there the layouts differ.
__device__ __forceinline__ void pn2_pad_row(int lane, Pn2Row row, int nsample, int32_t *out) {
    for (int l = row.cnt + lane; l < nsample; l += 64) out[l] = row.first;
}

// The ball around (cx, cy, cz) over the n points at p: 64 consecutive points per step, PN2_UNROLL steps in flight,
// d2 < r2 strict, the walk ends once nsample hits are placed.  The values written are positions in p.
constexpr int PN2_UNROLL = 4;
__device__ __forceinline__ Pn2Row pn2_ball_walk(const float *p, int n, float cx, float cy, float cz, float r2, int lane,
                                                unsigned long long below, int nsample, int32_t *out) {
    Pn2Row row = PN2_NO_HIT;
    for (int k0 = 0; k0 < n && row.cnt < nsample; k0 += 64 * PN2_UNROLL) {
        bool hit[PN2_UNROLL];
#pragma unroll
        for (int u = 0; u < PN2_UNROLL; ++u) {
            const int k = k0 + u * 64 + lane;
            hit[u] = false;
            if (k < n) {
                const float x = p[(int64_t)k * 3 + 0], y = p[(int64_t)k * 3 + 1], z = p[(int64_t)k * 3 + 2];
                const float d2 = ((cx - x) * (cx - x) + (cy - y) * (cy - y)) + (cz - z) * (cz - z);
                hit[u] = d2 < r2;
            }
        }
#pragma unroll
        for (int u = 0; u < PN2_UNROLL; ++u)
            row = pn2_place_hits(hit[u], k0 + u * 64 + lane, [k0, u](int j) { return k0 + u * 64 + j; }, below, nsample,
                                 row, out);
    }
    return row;
}

// ---------------------------------------------------------------- three nearest neighbours ------------------------
// A workgroup of four wavefronts for 64 unknown points, one per lane.  The known points pass through LDS in tiles and
// each wavefront walks its quarter of every tile in index order (all lanes read one address: a broadcast), keeping its
// own best three with the reference's strict <, in double like the reference, so that an infinite distance still
// enters.  The reference's result is the three smallest (distance, index) pairs in lexicographic order, so the four
// lists merge exactly by that order; a slot never filled travels as (inf, INT_MAX), behind any real pair, and leaves
// as the reference's initial values (1e40 -> inf, index 0).
constexpr int NN_TILE = 1024, NN_PARTS = 4, NN_SEG = NN_TILE / NN_PARTS;
__device__ __forceinline__ bool nn_less(float a, int ia, float b, int ib) { return a < b || (a == b && ia < ib); }

struct NNBest { double d1, d2, d3; int i1, i2, i3; };   // a lane's running best three in its wavefront
constexpr NNBest NN_NONE = {1e40, 1e40, 1e40, 0, 0, 0};
struct NNResult { float d1, d2, d3; int i1, i2, i3; };

// The tiles of one range of kn known points at kp, indices counted from the range's start; only lanes with `mine`
// compare.  Called by the whole workgroup with the same kp and kn (two barriers per tile); sk holds NN_TILE * 3 floats,
// part is the caller's threadIdx.x >> 6.  K is the caller's own type for a row count, int (batch) or int64_t (stacked);
// that, and the list in scalars declared as below, keep each kernel the loop it had when it held this code itself.
template <typename K>
__device__ __forceinline__ NNBest nn_walk(const float *kp, K kn, bool mine, float ux, float uy, float uz, float *sk,
                                          int part, NNBest b) {
    double best1 = b.d1, best2 = b.d2, best3 = b.d3;
    int i1 = b.i1, i2 = b.i2, i3 = b.i3;
    for (K k0 = 0; k0 < kn; k0 += NN_TILE) {
        const int cnt = (int)min((K)NN_TILE, kn - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 3; i += 256) sk[i] = kp[(int64_t)k0 * 3 + i];
        __syncthreads();
        if (mine) {
            const int s0 = part * NN_SEG, s1 = min(cnt, s0 + NN_SEG);
#pragma unroll 8
            for (int k = s0; k < s1; ++k) {
                const float x = sk[k * 3 + 0], y = sk[k * 3 + 1], z = sk[k * 3 + 2];
                const float d = ((ux - x) * (ux - x) + (uy - y) * (uy - y)) + (uz - z) * (uz - z);
                if (d < best1) {
                    best3 = best2; i3 = i2;
                    best2 = best1; i2 = i1;
                    best1 = d; i1 = (int)k0 + k;
                } else if (d < best2) {
                    best3 = best2; i3 = i2;
                    best2 = d; i2 = (int)k0 + k;
                } else if (d < best3) {
                    best3 = d; i3 = (int)k0 + k;
                }
            }
        }
    }
    return {best1, best2, best3, i1, i2, i3};
}

// The four wavefronts' lists of a lane merged by (distance, index), through md / mi.  Called by the whole workgroup (one
// barrier).  True in the lanes that hold the result, those of wavefront 0 whose row exists (`ok`); a slot never filled
// is (inf, index 0) in it.
__device__ __forceinline__ bool nn_finish(NNBest b, bool ok, float (*md)[3][64], int (*mi)[3][64], NNResult &r) {
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    float d1 = (float)b.d1, d2 = (float)b.d2, d3 = (float)b.d3;
    int i1 = b.i1, i2 = b.i2, i3 = b.i3;
    if (b.d1 == 1e40) i1 = INT_MAX;
    if (b.d2 == 1e40) i2 = INT_MAX;
    if (b.d3 == 1e40) i3 = INT_MAX;
    if (part > 0) {
        md[part - 1][0][lane] = d1; md[part - 1][1][lane] = d2; md[part - 1][2][lane] = d3;
        mi[part - 1][0][lane] = i1; mi[part - 1][1][lane] = i2; mi[part - 1][2][lane] = i3;
    }
    __syncthreads();
    const bool mine = part == 0 && ok;
    if (mine) {
#pragma unroll
        for (int q = 0; q < (NN_PARTS - 1) * 3; ++q) {
            const float d = md[q / 3][q % 3][lane];
            const int i = mi[q / 3][q % 3][lane];
            const bool l1 = nn_less(d, i, d1, i1), l2 = nn_less(d, i, d2, i2), l3 = nn_less(d, i, d3, i3);
            d3 = l2 ? d2 : (l3 ? d : d3); i3 = l2 ? i2 : (l3 ? i : i3);
            d2 = l1 ? d1 : (l2 ? d : d2); i2 = l1 ? i1 : (l2 ? i : i2);
            d1 = l1 ? d : d1; i1 = l1 ? i : i1;
        }
        r = {d1, d2, d3, i1 == INT_MAX ? 0 : i1, i2 == INT_MAX ? 0 : i2, i3 == INT_MAX ? 0 : i3};
    }
    return mine;
}
