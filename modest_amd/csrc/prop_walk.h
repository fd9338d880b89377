// What the RoI proposal layer (csrc/proposals.hip) and the post-processing (csrc/post_process.hip,
// section 7o) share: the argument checks of the two entry points (WALK_REQUIRE_*), the keys kernel (rank_keys: the score and
// sort key of a row, the sample of a row), the host front that ranks the rows (walk_params, rank_rows: the workspace of the
// sort, the keys, the sort), and the walk of one sample's candidates by a workgroup -- walk_segment, the body of prop_walk
// and of post_walk, so that both make the same decisions in the same order.  The tails of the two walk kernels are their
// files' own.  Include from a translation unit built with -ffp-contract=off, after common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iou_bev.h"
#include "sort64.h"
#include "loss_terms.h"

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

// The checks modest_proposals and modest_post_process make of the arguments they share, under the names both give them.
// Macros, not a function: MODEST_REQUIRE reports the entry point it stands in and the condition as it is written here.
#define WALK_REQUIRE_SIZES()                                                                                                   \
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= 2147483647LL, "between 0 and 2^31 - 1 rows");                                      \
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= WK_MAX_BATCH, "batch_size at most 65535 (16 sample bits of the sort key)"); \
    MODEST_REQUIRE(post_maxsize >= 0 && post_maxsize <= WK_POST_MAX, "NMS_POST_MAXSIZE at most 1024 (the kept list held in LDS)"); \
    MODEST_REQUIRE(pre_maxsize >= 0, "NMS_PRE_MAXSIZE is negative");                                                           \
    MODEST_REQUIRE(box_cols >= 7 && box_cols <= 4096 && cls_cols >= 1 && cls_cols <= 4096, "7 + C box columns and K >= 1 class columns, 4096 at most")
#define WALK_REQUIRE_BATCH_INDEX()                                                                                             \
    MODEST_REQUIRE(batch_index_kind >= BIDX_NONE && batch_index_kind <= BIDX_I32, "batch_index kind: 0 none, 1 float32, 2 int64, 3 int32"); \
    MODEST_REQUIRE(batch_index_kind == BIDX_NONE ? batch_index_dev == nullptr : (batch_index_dev != nullptr || n_rows == 0),   \
                   "batch_index and its kind disagree");                                                                       \
    if (batch_index_kind == BIDX_NONE)                                                                                         \
    MODEST_REQUIRE(rows_per_sample >= 0 && rows_per_sample * batch_size == n_rows, "dense form: n_rows = batch_size * rows_per_sample")

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

// One lane per row: its score, its sample and the 64-bit key  sample << 32 | descending(score) , whose ascending order is the
// samples one after the other, each by descending score with NaN first.  SCORED (the post-processing): the score is the
// sigmoid of the class maximum (the double function rounded once) unless `normalized`, and with `has_thresh` a row that
// fails  score >= thresh  (a NaN fails) is in no sample: it gets sample b and sorts behind every segment.  Not SCORED (the
// proposal layer): the class maximum as it is, and the three arguments are not read.
template <bool SCORED>
__global__ __launch_bounds__(256) void rank_keys(int64_t n, int b, int64_t rows_per_sample, const float *__restrict__ cls,
                                                 int k, const void *__restrict__ bidx, int kind, int normalized,
                                                 int has_thresh, float thresh, uint64_t *__restrict__ key,
                                                 uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int label;
    float s = row_max(cls + i * k, k, label);
    if (SCORED && !normalized) s = modest::loss::sigmoid_f32(s);
    int64_t sample = row_sample(i, b, rows_per_sample, bidx, kind);
    if (SCORED && has_thresh && !(s >= thresh)) sample = b;
    key[i] = ((uint64_t)sample << 32) | descending_bits(s);
    idx[i] = (uint32_t)i;
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

// the fields both walks read, the rows not yet ranked
WalkParams walk_params(int64_t n_rows, const float *box, int box_cols, const float *cls, int cls_cols, int pre, int post,
                       float thresh, float *rois, float *scores, int64_t *labels) {
    WalkParams p;
    p.n = n_rows;
    p.key = nullptr;
    p.idx = nullptr;
    p.box = box;
    p.cls = cls;
    p.box_cols = box_cols;
    p.cls_cols = cls_cols;
    p.pre = pre;
    p.post = post;
    p.thresh = thresh;
    p.rois = rois;
    p.scores = scores;
    p.labels = labels;
    return p;
}

// The p.n > 0 rows ranked: key[2] / idx[2] / table laid over the workspace (layout(p.n) bytes, 8-byte aligned: the caller has
// checked both), rank_keys<SCORED>, sort64 over the 32 score bits and the bits of `sample_max`, the largest value the sample
// field can hold (it decides the number of radix passes); p.key / p.idx are the sorted side.  -> MODEST_OK or an error code
template <bool SCORED>
int rank_rows(WalkParams &p, int batch_size, int64_t rows_per_sample, const void *batch_index_dev, int batch_index_kind,
              int normalized, int has_thresh, float thresh, int sample_max, void *workspace_dev, hipStream_t st) {
    const Layout L = layout(p.n);
    char *ws = static_cast<char *>(workspace_dev);
    uint64_t *key[2] = {reinterpret_cast<uint64_t *>(ws + L.key[0]), reinterpret_cast<uint64_t *>(ws + L.key[1])};
    uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + L.idx[0]), reinterpret_cast<uint32_t *>(ws + L.idx[1])};
    uint32_t *table = reinterpret_cast<uint32_t *>(ws + L.table);
    rank_keys<SCORED><<<(unsigned)((p.n + 255) / 256), 256, 0, st>>>(p.n, batch_size, rows_per_sample, p.cls, p.cls_cols,
                                                                   batch_index_dev, batch_index_kind, normalized, has_thresh,
                                                                   thresh, key[0], idx[0]);
    MODEST_HIP_CHECK(hipGetLastError());
    const int fin = sort64(key, idx, (int)p.n, 32 + sort64_bit_length((uint64_t)sample_max), table, st);
    p.key = key[fin];
    p.idx = idx[fin];
    return MODEST_OK;
}

}  // namespace
