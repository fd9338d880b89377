// RoI proposal layer of OpenPCDet's two-stage detectors (RoIHeadTemplate.proposal_layer,
// pcdet/models/roi_heads/roi_head_template.py:45-99, over class_agnostic_nms, model_utils/model_nms_utils.py:6-25, with
// MULTI_CLASSES_NMS off), hand-written for gfx950.  One entry point (include/modest_hip.h, "a31") selects the proposals of
// a whole batch, dense or stacked: enqueue only, no context, no device allocation, no synchronise, nothing read back, no
// (n, n / 64) suppression mask; every element of the three outputs is written.  DESIGN.md section 7m.
//
//   rank_keys   (csrc/prop_walk.h, not SCORED) one lane per row: max / argmax over the class columns (lowest class among
//               equal maxima, NaN above every number), the row's sample (dense: row / rows per sample; stacked: batch_index,
//               a value that names no sample in [0, B) sorts behind every sample), and the 64-bit key
//               sample << 32 | descending(score)  whose ascending order is descending score with NaN first and -0 == +0;
//   sort64      stable: equal scores keep ascending row order, samples become segments (csrc/sort64.h);
//   prop_walk   one workgroup per sample.  It finds its segment by two binary searches and walks the first
//               min(PRE, rows) candidates 64 at a time in score order: (A) the chunk against the kept list, the list dealt
//               round-robin to the wavefronts, a lane per candidate; (B) the chunk's live candidates among themselves, a
//               suppression word per row; (C) the 64 x 64 bits resolved in order, the survivors appended to the kept list
//               (box + trig in LDS) until the POST-th, which ends the walk wherever in the chunk it falls.  The tail
//               gathers the survivors' 7 + C columns, scores and labels and writes the padding.
// A pair is tested as iou(earlier, later) > thresh by the device functions of nms_tiles (csrc/iou_bev.h), so a decision
// is the one nms_gpu / nms_normal_gpu make on the same order.
// The shared argument checks, the keys kernel, the host front that ranks the rows (the workspace layout, the keys, the sort)
// and the walk itself (walk_segment) are in csrc/prop_walk.h, shared with csrc/post_process.hip; the walk's figures (WK_*:
// 4 wavefronts, chunks of 64, at most 1024 survivors and 65535 samples) are there too.  This file keeps prop_walk's tail.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "iou_bev.h"
#include "sort64.h"
#include "prop_walk.h"

namespace {

template <bool ROTATED>
__global__ __launch_bounds__(WK_T) void prop_walk(WalkParams p) {
    const int tid = threadIdx.x, s = blockIdx.x;
    const Walked k = walk_segment<ROTATED>(p, s);
    const int nk = k.nk;
    const uint32_t *s_krow = k.krow;
    // the survivors' columns, scores and labels; the padding
    const int cols = p.box_cols;
    float *rois = p.rois + (size_t)s * p.post * cols;
    for (int t = tid; t < p.post * cols; t += WK_T) {
        const int pos = t / cols, col = t - pos * cols;
        rois[t] = pos < nk ? p.box[(size_t)s_krow[pos] * cols + col] : 0.f;
    }
    for (int pos = tid; pos < p.post; pos += WK_T) {
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
    WALK_REQUIRE_SIZES();
    WALK_REQUIRE_BATCH_INDEX();
    if (batch_size == 0 || post_maxsize == 0) return MODEST_OK;   // empty outputs
    MODEST_REQUIRE(rois_dev && roi_scores_dev && roi_labels_dev, "NULL output");
    hipStream_t st = as_stream(stream);
    WalkParams p = walk_params(n_rows, box_dev, box_cols, cls_dev, cls_cols, pre_maxsize, post_maxsize, thresh, rois_dev,
                               roi_scores_dev, roi_labels_dev);
    if (n_rows > 0) {
        MODEST_REQUIRE(box_dev && cls_dev, "NULL buffer");
        const Layout L = layout(n_rows);
        MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)L.total, "workspace smaller than modest_proposals_workspace_bytes");
        MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
        // the sample field holds batch_size itself in the stacked form (a row of no sample)
        const int rc = rank_rows<false>(p, batch_size, rows_per_sample, batch_index_dev, batch_index_kind, 0, 0, 0.f,
                                        batch_index_kind == BIDX_NONE ? batch_size - 1 : batch_size, workspace_dev, st);
        if (rc != MODEST_OK) return rc;
    }
    if (rotated)
        prop_walk<true><<<(unsigned)batch_size, WK_T, 0, st>>>(p);
    else
        prop_walk<false><<<(unsigned)batch_size, WK_T, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
