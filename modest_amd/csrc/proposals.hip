// RoI proposal layer of OpenPCDet's two-stage detectors (RoIHeadTemplate.proposal_layer,
// pcdet/models/roi_heads/roi_head_template.py:45-99, over class_agnostic_nms, model_utils/model_nms_utils.py:6-25, with
// MULTI_CLASSES_NMS off), hand-written for gfx950.  One entry point (include/modest_hip.h, "a31") selects the proposals of
// a whole batch, dense or stacked: enqueue only, no context, no device allocation, no synchronise, nothing read back, no
// (n, n / 64) suppression mask; every element of the three outputs is written.  DESIGN.md section 7m.
//
//   prop_keys   one lane per row: max / argmax over the class columns (lowest class among equal maxima, NaN above every
//               number), the row's sample (dense: row / rows per sample; stacked: batch_index, a value that names no sample
//               in [0, B) sorts behind every sample), and the 64-bit key  sample << 32 | descending(score)  whose
//               ascending order is descending score with NaN first and -0 == +0;
//   sort64      stable: equal scores keep ascending row order, samples become segments (csrc/sort64.h);
//   prop_walk   one workgroup per sample.  It finds its segment by two binary searches and walks the first
//               min(PRE, rows) candidates 64 at a time in score order: (A) the chunk against the kept list, the list dealt
//               round-robin to the wavefronts, a lane per candidate; (B) the chunk's live candidates among themselves, a
//               suppression word per row; (C) the 64 x 64 bits resolved in order, the survivors appended to the kept list
//               (box + trig in LDS) until the POST-th, which ends the walk wherever in the chunk it falls.  The tail
//               gathers the survivors' 7 + C columns, scores and labels and writes the padding.
// A pair is tested as iou(earlier, later) > thresh by the device functions of nms_tiles (csrc/iou_bev.h), so a decision
// is the one nms_gpu / nms_normal_gpu make on the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "iou_bev.h"
#include "sort64.h"

namespace {

constexpr int PW_WAVES = 4;                  // wavefronts of a walk workgroup: each owns a PolyLds (18 KB)
constexpr int PW_T = 64 * PW_WAVES;
constexpr int PW_CHUNK = 64;                 // candidates per step: one suppression word per row
constexpr int PW_POST_MAX = 1024;            // kept list held in LDS (44 B a box)
constexpr int PW_REC = 11;                   // box (7) + cos h, sin h, cos(-h), sin(-h)
constexpr int PROP_MAX_BATCH = 65535;        // 16 sample bits above the 32 score bits of a key
// LDS of prop_walk: 4 * 18432 (PolyLds) + 1024 * 44 + 1024 * 4 (kept) + 64 * 44 + 64 * 4 (chunk) + 64 * 8 + 4 * 8 + 16
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

__global__ __launch_bounds__(256) void prop_keys(int64_t n, int b, int64_t rows_per_sample, const float *__restrict__ cls,
                                                 int k, const void *__restrict__ bidx, int kind,
                                                 uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int label;
    const float s = row_max(cls + i * k, k, label);
    int64_t sample = b;      // names no sample: behind every segment
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

template <bool ROTATED>
__global__ __launch_bounds__(PW_T) void prop_walk(WalkParams p) {
    __shared__ PolyLds s_poly[PW_WAVES];
    __shared__ float s_k[PW_POST_MAX][PW_REC];        // the kept list
    __shared__ uint32_t s_krow[PW_POST_MAX];          // ... and its rows
    __shared__ float s_c[PW_CHUNK][PW_REC];           // the chunk
    __shared__ uint32_t s_crow[PW_CHUNK];
    __shared__ unsigned long long s_mat[PW_CHUNK];    // bit j of word i: candidate i suppresses candidate j > i
    __shared__ unsigned long long s_sup[PW_WAVES];    // bit j: a kept box of wavefront w's share suppresses candidate j
    __shared__ int64_t s_seg[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = blockIdx.x;
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
    for (int c0 = 0; c0 < cnt && nk < p.post; c0 += PW_CHUNK) {
        const int m = min(PW_CHUNK, cnt - c0);
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
        // (A) against the kept list: wavefront w takes kept boxes w, w + PW_WAVES, ...
        bool sup = lane >= m;
        for (int k = w; k < nk; k += PW_WAVES) {
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
        for (int q = 0; q < PW_WAVES; ++q) dead |= s_sup[q];
        // (B) the live candidates among themselves: wavefront w takes rows w, w + PW_WAVES, ...
        for (int i = w; i < m; i += PW_WAVES) {
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
            for (int q = 0; q < PW_REC; ++q) s_k[pos][q] = s_c[lane][q];
            s_krow[pos] = s_crow[lane];
        }
        nk = c;
        __syncthreads();   // the kept list is complete, the chunk has been read
    }
    __syncthreads();
    // the survivors' columns, scores and labels; the padding
    const int cols = p.box_cols;
    float *rois = p.rois + (size_t)s * p.post * cols;
    for (int t = tid; t < p.post * cols; t += PW_T) {
        const int pos = t / cols, col = t - pos * cols;
        rois[t] = pos < nk ? p.box[(size_t)s_krow[pos] * cols + col] : 0.f;
    }
    for (int pos = tid; pos < p.post; pos += PW_T) {
        float sc = 0.f;
        int label = 0;
        if (pos < nk) sc = row_max(p.cls + (size_t)s_krow[pos] * p.cls_cols, p.cls_cols, label);
        p.scores[(size_t)s * p.post + pos] = sc;
        p.labels[(size_t)s * p.post + pos] = (int64_t)label + 1;
    }
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

extern "C" int64_t modest_proposals_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows > 2147483647LL) {
        modest_set_error("modest_proposals_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 (the row count of a call)");
        return MODEST_ERR_ARG;
    }
    return (int64_t)layout(n_rows).total;
}

extern "C" int modest_proposals(int64_t n_rows, int batch_size, int64_t rows_per_sample, const float *box_dev, int box_cols,
                                const float *cls_dev, int cls_cols, const void *batch_index_dev, int batch_index_kind,
                                int pre_maxsize, int post_maxsize, float thresh, int rotated, float *rois_dev,
                                float *roi_scores_dev, int64_t *roi_labels_dev, void *workspace_dev, int64_t workspace_bytes,
                                void *stream) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= 2147483647LL, "between 0 and 2^31 - 1 rows");
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= PROP_MAX_BATCH, "batch_size at most 65535 (16 sample bits of the sort key)");
    MODEST_REQUIRE(post_maxsize >= 0 && post_maxsize <= PW_POST_MAX, "NMS_POST_MAXSIZE at most 1024 (the kept list held in LDS)");
    MODEST_REQUIRE(pre_maxsize >= 0, "NMS_PRE_MAXSIZE is negative");
    MODEST_REQUIRE(box_cols >= 7 && box_cols <= 4096 && cls_cols >= 1 && cls_cols <= 4096, "7 + C box columns and K >= 1 class columns, 4096 at most");
    MODEST_REQUIRE(batch_index_kind >= BIDX_NONE && batch_index_kind <= BIDX_I32, "batch_index kind: 0 none, 1 float32, 2 int64, 3 int32");
    MODEST_REQUIRE(batch_index_kind == BIDX_NONE ? batch_index_dev == nullptr : (batch_index_dev != nullptr || n_rows == 0),
                   "batch_index and its kind disagree");
    if (batch_index_kind == BIDX_NONE)
        MODEST_REQUIRE(rows_per_sample >= 0 && rows_per_sample * batch_size == n_rows, "dense form: n_rows = batch_size * rows_per_sample");
    if (batch_size == 0 || post_maxsize == 0) return MODEST_OK;   // empty outputs
    MODEST_REQUIRE(rois_dev && roi_scores_dev && roi_labels_dev, "NULL output");
    hipStream_t st = as_stream(stream);
    WalkParams p;
    p.n = n_rows;
    p.key = nullptr;
    p.idx = nullptr;
    if (n_rows > 0) {
        MODEST_REQUIRE(box_dev && cls_dev, "NULL buffer");
        const Layout L = layout(n_rows);
        MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)L.total, "workspace smaller than modest_proposals_workspace_bytes");
        MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
        char *ws = static_cast<char *>(workspace_dev);
        uint64_t *key[2] = {reinterpret_cast<uint64_t *>(ws + L.key[0]), reinterpret_cast<uint64_t *>(ws + L.key[1])};
        uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + L.idx[0]), reinterpret_cast<uint32_t *>(ws + L.idx[1])};
        uint32_t *table = reinterpret_cast<uint32_t *>(ws + L.table);
        prop_keys<<<(unsigned)((n_rows + 255) / 256), 256, 0, st>>>(n_rows, batch_size, rows_per_sample, cls_dev, cls_cols,
                                                                  batch_index_dev, batch_index_kind, key[0], idx[0]);
        MODEST_HIP_CHECK(hipGetLastError());
        // the sample field holds batch_size itself in the stacked form (a row of no sample)
        const int bits = 32 + sort64_bit_length((uint64_t)(batch_index_kind == BIDX_NONE ? batch_size - 1 : batch_size));
        const int fin = sort64(key, idx, (int)n_rows, bits, table, st);
        p.key = key[fin];
        p.idx = idx[fin];
    }
    p.box = box_dev;
    p.cls = cls_dev;
    p.box_cols = box_cols;
    p.cls_cols = cls_cols;
    p.pre = pre_maxsize;
    p.post = post_maxsize;
    p.thresh = thresh;
    p.rois = rois_dev;
    p.scores = roi_scores_dev;
    p.labels = roi_labels_dev;
    if (rotated)
        prop_walk<true><<<(unsigned)batch_size, PW_T, 0, st>>>(p);
    else
        prop_walk<false><<<(unsigned)batch_size, PW_T, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
