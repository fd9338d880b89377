// What the RoI proposal layer (csrc/proposals.hip) and the post-processing (csrc/post_process.hip,
// section 7o) share: the score and sort key of a row, the sample of a row, the workspace of the sort, and the walk of one
// sample's candidates by a workgroup -- walk_segment, the body of prop_walk and of post_walk, so that both make the same
// decisions in the same order.  Include from a translation unit built with -ffp-contract=off, after common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iou_bev.h"
#include "sort64.h"

namespace {

constexpr int WK_WAVES = 4;                  // wavefronts of a walk workgroup: each owns a PolyLds (18 KB)
constexpr int WK_T = 64 * WK_WAVES;
constexpr int WK_CHUNK = 64;                 // candidates per step: one suppression word per row
constexpr int WK_POST_MAX = 1024;            // kept list held in LDS (44 B a box)
constexpr int WK_REC = 11;                   // box (7) + cos h, sin h, cos(-h), sin(-h)
constexpr int WK_MAX_BATCH = 65535;          // 16 sample bits above the 32 score bits of a key
// LDS of a walk kernel (prop_walk, post_walk): 4 * 18432 (PolyLds) + 1024 * 44 + 1024 * 4 (kept) + 64 * 44 + 64 * 4 (chunk) + 64 * 8 + 4 * 8 + 16
//                 = 126.5 KB of the CU's 160 KB; a fifth PolyLds would fit, a sixth would not.

enum { BIDX_NONE = 0, BIDX_F32 = 1, BIDX_I64 = 2, BIDX_I32 = 3 };

// max over the k class values of a row and its column: the lowest column among equal maxima, a NaN above every number
// (the first NaN wins)
__device__ __forceinline__ float row_max(const float *__restrict__ c, int k, int &label) {
    float best = c[0];
    int at = 0;
    for (int j = 1; j < k; ++j) {
        const float v = c[j];
        if (v > best || (v != v && best == best)) {
            best = v;
            at = j;
        }
    }
    label = at;
    return best;
}

// 32 bits whose ascending unsigned order is the descending order of the scores: NaN first, then +inf ... -inf; -0 == +0
__device__ __forceinline__ uint32_t descending_bits(float s) {
    if (s != s) return 0u;
    if (s == 0.f) s = 0.f;   // -0 -> +0
    const uint32_t u = __float_as_uint(s);
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;             // +inf -> 0x007fffff: above the NaN's 0
}

// the sample of row i: dense by position, stacked by batch_index; b where the value names no sample (behind every segment)
__device__ __forceinline__ int64_t row_sample(int64_t i, int b, int64_t rows_per_sample, const void *__restrict__ bidx, int kind) {
    int64_t sample = b;
    if (kind == BIDX_NONE) {
        sample = i / rows_per_sample;
    } else if (kind == BIDX_F32) {
        const float v = static_cast<const float *>(bidx)[i];
        if (v >= 0.f && v < (float)b) {   // NaN fails both
            const int t = (int)v;
            if ((float)t == v) sample = t;
        }
    } else {
        const int64_t v = kind == BIDX_I64 ? static_cast<const int64_t *>(bidx)[i] : (int64_t) static_cast<const int32_t *>(bidx)[i];
        if (v >= 0 && v < b) sample = v;
    }
    return sample;
}

struct WalkParams {
    int64_t n;                    // rows
    const uint64_t *key;          // sorted
    const uint32_t *idx;          // their rows
    const float *box, *cls;
    int box_cols, cls_cols;
    int pre, post;
    float thresh;
    float *rois, *scores;
    int64_t *labels;
};

// first position whose key is >= v
__device__ __forceinline__ int64_t lower_bound(const uint64_t *__restrict__ key, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Walked {
    int nk;                       // survivors: the same in every lane
    const uint32_t *krow;         // their rows, in LDS, in keep order
};

// The walk of sample s, by a whole workgroup of WK_T lanes: the body of prop_walk and post_walk.  It owns the workgroup's LDS
// and ends behind a barrier, the kept rows complete.
template <bool ROTATED>
__device__ __forceinline__ Walked walk_segment(const WalkParams &p, int s) {
    __shared__ PolyLds s_poly[WK_WAVES];
    __shared__ float s_k[WK_POST_MAX][WK_REC];        // the kept list
    __shared__ uint32_t s_krow[WK_POST_MAX];          // ... and its rows
    __shared__ float s_c[WK_CHUNK][WK_REC];           // the chunk
    __shared__ uint32_t s_crow[WK_CHUNK];
    __shared__ unsigned long long s_mat[WK_CHUNK];    // bit j of word i: candidate i suppresses candidate j > i
    __shared__ unsigned long long s_sup[WK_WAVES];    // bit j: a kept box of wavefront w's share suppresses candidate j
    __shared__ int64_t s_seg[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) {
        s_seg[0] = lower_bound(p.key, p.n, (uint64_t)s << 32);
        s_seg[1] = lower_bound(p.key, p.n, ((uint64_t)s + 1) << 32);
    }
    __syncthreads();
    const int64_t first = s_seg[0];
    const int64_t rows = s_seg[1] - first;
    const int cnt = (int)(rows < (int64_t)p.pre ? rows : (int64_t)p.pre);
    PolyLds &L = s_poly[w];
    int nk = 0;   // kept so far: the same in every lane
    for (int c0 = 0; c0 < cnt && nk < p.post; c0 += WK_CHUNK) {
        const int m = min(WK_CHUNK, cnt - c0);
        if (tid < m) {
            const uint32_t row = p.idx[first + c0 + tid];
            const float *src = p.box + (size_t)row * p.box_cols;
            float bx[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) bx[q] = src[q];
            const float4 t = ROTATED ? device_trig(bx[6]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < 7; ++q) s_c[tid][q] = bx[q];
            s_c[tid][7] = t.x; s_c[tid][8] = t.y; s_c[tid][9] = t.z; s_c[tid][10] = t.w;
            s_crow[tid] = row;
        }
        __syncthreads();
        // the lane's candidate
        float cb[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) cb[q] = s_c[lane][q];
        const float4 tcb = make_float4(s_c[lane][7], s_c[lane][8], s_c[lane][9], s_c[lane][10]);
        // (A) against the kept list: wavefront w takes kept boxes w, w + WK_WAVES, ...
        bool sup = lane >= m;
        for (int k = w; k < nk; k += WK_WAVES) {
            if (__all(sup)) break;
            if (!sup) {
                float a[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) a[q] = s_k[k][q];
                const float4 ta = make_float4(s_k[k][7], s_k[k][8], s_k[k][9], s_k[k][10]);
                const float v = ROTATED ? iou_bev(a, cb, ta, tcb, L) : iou_normal(a, cb);
                if (v > p.thresh) sup = true;
            }
        }
        const unsigned long long supw = __ballot(sup);
        if (lane == 0) s_sup[w] = supw;
        __syncthreads();
        unsigned long long dead = 0;   // suppressed by the kept list, or past the chunk's end
#pragma unroll
        for (int q = 0; q < WK_WAVES; ++q) dead |= s_sup[q];
        // (B) the live candidates among themselves: wavefront w takes rows w, w + WK_WAVES, ...
        for (int i = w; i < m; i += WK_WAVES) {
            if ((dead >> i) & 1ull) continue;   // never kept: its word is never read
            bool hit = false;
            if (lane > i && !((dead >> lane) & 1ull)) {
                float a[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) a[q] = s_c[i][q];
                const float4 ta = make_float4(s_c[i][7], s_c[i][8], s_c[i][9], s_c[i][10]);
                const float v = ROTATED ? iou_bev(a, cb, ta, tcb, L) : iou_normal(a, cb);
                hit = v > p.thresh;
            }
            const unsigned long long word = __ballot(hit);
            if (lane == 0) s_mat[i] = word;
        }
        __syncthreads();
        // (C) in order: a live candidate is kept and its word kills later ones; the POST-th survivor ends the walk
        unsigned long long alive = ~dead, keepm = 0;
        int c = nk;
        while (alive != 0 && c < p.post) {
            const int i = __ffsll((long long)alive) - 1;
            keepm |= 1ull << i;
            ++c;
            alive &= ~s_mat[i];
            alive &= ~(1ull << i);
        }
        if (w == 0 && ((keepm >> lane) & 1ull)) {
            const int pos = nk + __popcll(keepm & ((1ull << lane) - 1ull));
#pragma unroll
            for (int q = 0; q < WK_REC; ++q) s_k[pos][q] = s_c[lane][q];
            s_krow[pos] = s_crow[lane];
        }
        nk = c;
        __syncthreads();   // the kept list is complete, the chunk has been read
    }
    __syncthreads();
    Walked out;
    out.nk = nk;
    out.krow = s_krow;
    return out;
}

struct Layout {
    size_t key[2], idx[2], table, total;
};

Layout layout(int64_t n) {
    Layout L;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += arena_sz(bytes);
        return at;
    };
    const size_t rows = (size_t)(n > 0 ? n : 1);
    L.key[0] = take(8 * rows);
    L.key[1] = take(8 * rows);
    L.idx[0] = take(4 * rows);
    L.idx[1] = take(4 * rows);
    L.table = take(4 * sort64_table_words((int64_t)rows));
    L.total = off;
    return L;
}

}  // namespace
