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
// The keys' helpers, the workspace layout and the walk itself (walk_segment) are in csrc/prop_walk.h, shared with
// csrc/post_process.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "iou_bev.h"
#include "sort64.h"
#include "prop_walk.h"

namespace {

// the figures of the walk, which csrc/prop_walk.h holds for both of its users
constexpr int PW_WAVES = 4;                  // wavefronts of a walk workgroup: each owns a PolyLds (18 KB)
constexpr int PW_T = 64 * PW_WAVES;
constexpr int PW_CHUNK = 64;                 // candidates per step: one suppression word per row
constexpr int PW_POST_MAX = 1024;            // kept list held in LDS (44 B a box)
constexpr int PROP_MAX_BATCH = 65535;        // 16 sample bits above the 32 score bits of a key
static_assert(PW_WAVES == WK_WAVES && PW_T == WK_T && PW_CHUNK == WK_CHUNK && PW_POST_MAX == WK_POST_MAX &&
                  PROP_MAX_BATCH == WK_MAX_BATCH, "csrc/prop_walk.h walks by other figures");

__global__ __launch_bounds__(256) void prop_keys(int64_t n, int b, int64_t rows_per_sample, const float *__restrict__ cls,
                                                 int k, const void *__restrict__ bidx, int kind,
                                                 uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int label;
    const float s = row_max(cls + i * k, k, label);
    const int64_t sample = row_sample(i, b, rows_per_sample, bidx, kind);
    key[i] = ((uint64_t)sample << 32) | descending_bits(s);
    idx[i] = (uint32_t)i;
}

template <bool ROTATED>
__global__ __launch_bounds__(PW_T) void prop_walk(WalkParams p) {
    const int tid = threadIdx.x, s = blockIdx.x;
    const Walked k = walk_segment<ROTATED>(p, s);
    const int nk = k.nk;
    const uint32_t *s_krow = k.krow;
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
