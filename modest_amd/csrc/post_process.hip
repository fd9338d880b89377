// Post-processing of a detector's test-time forward (Detector3DTemplate.post_processing,
// pcdet/models/detectors/detector3d_template.py:175-325, over class_agnostic_nms, model_utils/model_nms_utils.py:6-25, and
// generate_recall_record, with MULTI_CLASSES_NMS off), hand-written for gfx950.  One entry point (include/modest_hip.h,
// "a33") takes a whole batch, dense or stacked: no context, no device allocation, one stream synchronise at the end, nothing
// read back but the caller's small pinned table, which the kernels write.  DESIGN.md section 7o.  The shared argument
// checks, the keys kernel (rank_keys, here SCORED: the sigmoid of a logit, the double function rounded once, and the score
// threshold: a row that fails  score >= thresh  (a NaN fails) gets sample B and sorts behind every segment), the host front
// that ranks the rows and the walk (walk_segment, the body of prop_walk too) are those of the RoI proposal layer
// (csrc/prop_walk.h); this file adds:
//   post_walk     walk_segment, then the n survivors' 7 + C columns, scores and labels into the front of the sample's padded
//               row, and n into the workspace and the caller's pinned table;
//   post_recall   one workgroup per sample and box list, only with gts: the trim of rt_match, a lane per valid gt (64 at a
//               time, in each of the four wavefronts), the box list (the sample's final boxes, or all of its rows and its
//               rois) staged in LDS PR_TILE at a time and shared out to the wavefronts, the 3-D IoU by csrc/iou3d_steps.h,
//               torch's max (a NaN stays), the gts above each threshold counted into the pinned table.
// modest_post_process then synchronises the stream: its one host wait.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "prop_walk.h"
#include "iou3d_steps.h"
#include "loss_terms.h"

namespace {

using modest::loss::sigmoid_f32;   // torch.sigmoid's value by the project's rule for log / cos / sin: the double function, rounded once

// ------------------------------------------------------------------------------------------------ post-processing ("a33")
constexpr int PR_WAVES = 4;                  // wavefronts of a recall workgroup: each owns a PolyLds
constexpr int PR_T = 64 * PR_WAVES;          // 64 gts at a time, a lane each in every wavefront; the wavefronts share the boxes
constexpr int PR_TILE = 64;                  // boxes of a list staged in LDS at a time (modest_post_process_tile)
constexpr int PR_REC = 14;                   // box (7) + cos h, sin h, cos(-h), sin(-h) + top, bottom, volume
constexpr int PR_MAX_THRESH = 16;            // RECALL_THRESH_LIST: the thresholds travel in the kernel's arguments
// LDS of post_recall: 4 * 18432 (PolyLds) + 64 * 14 * 4 (tile) + 2 * 4 * 64 * 4 (the wavefronts' maxima) + 16 * 4 + 4 = 79 428 B.

struct PostParams {
    WalkParams w;                 // w.rois / w.scores / w.labels: the padded (B, post, .) outputs
    int normalized, raw_out;
    const int64_t *given;         // labels by row, or NULL: argmax + 1
    int32_t *nb;                  // (B) survivors, workspace
    int32_t *table;               // (B, stride) pinned host words: survivors, gts, rcnn per threshold, roi per threshold
    int stride;
};

template <bool ROTATED>
__global__ __launch_bounds__(WK_T) void post_walk(PostParams p) {
    const int tid = threadIdx.x, s = blockIdx.x;
    const Walked k = walk_segment<ROTATED>(p.w, s);
    const int nk = k.nk;
    // the survivors' columns, scores and labels into the front of the sample's row; the padding is not written
    const int cols = p.w.box_cols;
    float *boxes = p.w.rois + (size_t)s * p.w.post * cols;
    for (int t = tid; t < nk * cols; t += WK_T) {
        const int pos = t / cols, col = t - pos * cols;
        boxes[t] = p.w.box[(size_t)k.krow[pos] * cols + col];
    }
    for (int pos = tid; pos < nk; pos += WK_T) {
        const uint32_t row = k.krow[pos];
        int label;
        float sc = row_max(p.w.cls + (size_t)row * p.w.cls_cols, p.w.cls_cols, label);
        if (!p.normalized && !p.raw_out) sc = sigmoid_f32(sc);
        p.w.scores[(size_t)s * p.w.post + pos] = sc;
        p.w.labels[(size_t)s * p.w.post + pos] = p.given ? p.given[row] : (int64_t)label + 1;
    }
    if (tid == 0) {
        p.nb[s] = nk;
        p.table[(size_t)s * p.stride] = nk;
    }
}

struct RecallParams {
    int g, gt_cols;               // gt rows per sample, 7 + C + 1
    const float *gt;              // (B, g, gt_cols) by strides, in elements
    int64_t gs0, gs1, gs2;
    int nlist;                    // 1: rcnn; 2: rcnn and roi
    const float *list[2];         // (B, per, cols) contiguous
    int cols[2], per[2];
    int from_nb[2];               // the sample's rows: nb[b] (its final boxes) or per
    const int32_t *nb;
    int t;
    float thr[PR_MAX_THRESH];
    int32_t *table;
    int stride;
};

__global__ __launch_bounds__(PR_T) void post_recall(RecallParams p) {
    __shared__ PolyLds s_poly[PR_WAVES];
    __shared__ float s_box[PR_TILE][PR_REC];
    __shared__ float s_best[PR_WAVES][64];
    __shared__ int s_state[PR_WAVES][64];             // 0: no box seen, 1: a number, 2: a NaN among them
    __shared__ int s_cnt[PR_MAX_THRESH];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x, l = blockIdx.y;         // sample, list
    const float *gt = p.gt + (int64_t)b * p.gs0;
    // trim, as rt_match: the last row whose sum is not == 0 (a NaN sum is not), row 0 at the least; no row, no gt
    if (tid == 0) s_last = 0;
    if (tid < PR_MAX_THRESH) s_cnt[tid] = 0;
    __syncthreads();
    int last = 0;
    for (int j = tid; j < p.g; j += PR_T) {
        const float *row = gt + (int64_t)j * p.gs1;
        float s = row[0];
        for (int c = 1; c < p.gt_cols; ++c) s = s + row[(int64_t)c * p.gs2];
        if (!(s == 0.f)) last = j;
    }
    if (last > 0) atomicMax(&s_last, last);
    __syncthreads();
    const int nvalid = p.g > 0 ? s_last + 1 : 0;
    PolyLds &L = s_poly[w];
    const int rows = p.from_nb[l] ? min(p.nb[b], p.per[l]) : p.per[l];   // the walk stops at post
    const int cols = p.cols[l];
    const float *list = p.list[l] + (size_t)b * p.per[l] * cols;
    // 64 gts at a time, a lane each in EVERY wavefront; the wavefronts share out the boxes of a tile
    for (int g0 = 0; g0 < nvalid && rows > 0; g0 += 64) {
        const int gi = g0 + lane;
        const bool live = gi < nvalid;
        float bb[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float *row = gt + (int64_t)gi * p.gs1;
#pragma unroll
            for (int q = 0; q < 7; ++q) bb[q] = row[(int64_t)q * p.gs2];
        }
        const float4 tb = device_trig(bb[6]);
        float best = 0.f;      // the largest number so far
        int state = 0;
        for (int t0 = 0; t0 < rows; t0 += PR_TILE) {
            const int m = min(PR_TILE, rows - t0);
            __syncthreads();   // the tile before has been read
            if (tid < m) {
                const float *src = list + (size_t)(t0 + tid) * cols;
                float a[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) a[q] = src[q];
                const float4 t = device_trig(a[6]);
                const Iou3dSide sa = iou3d_side(a);
#pragma unroll
                for (int q = 0; q < 7; ++q) s_box[tid][q] = a[q];
                s_box[tid][7] = t.x; s_box[tid][8] = t.y; s_box[tid][9] = t.z; s_box[tid][10] = t.w;
                s_box[tid][11] = sa.top; s_box[tid][12] = sa.bot; s_box[tid][13] = sa.vol;
            }
            __syncthreads();
            if (live) {
                for (int k = w; k < m; k += PR_WAVES) {
                    float a[7];
#pragma unroll
                    for (int q = 0; q < 7; ++q) a[q] = s_box[k][q];
                    const float4 ta = make_float4(s_box[k][7], s_box[k][8], s_box[k][9], s_box[k][10]);
                    Iou3dSide sa;
                    sa.top = s_box[k][11]; sa.bot = s_box[k][12]; sa.vol = s_box[k][13];
                    const float v = iou3d_from_bev(sa, bb, box_overlap(a, bb, ta, tb, L));   // csrc/iou3d_steps.h
                    if (v != v) state = 2;
                    else if (state == 0 || v > best) best = v;
                    if (state == 0) state = 1;
                }
            }
        }
        s_best[w][lane] = best;
        s_state[w][lane] = state;
        __syncthreads();
        if (w == 0) {          // torch's max over the list: a NaN anywhere stays, and is not recalled
            float top = 0.f;
            int st = 0;
#pragma unroll
            for (int q = 0; q < PR_WAVES; ++q) {
                const int sq = s_state[q][lane];
                const float vq = s_best[q][lane];
                if (sq != 0 && (st == 0 || vq > top)) top = vq;
                st = max(st, sq);
            }
            for (int q = 0; q < p.t; ++q) {
                const unsigned long long word = __ballot(live && st == 1 && top > p.thr[q]);
                if (lane == 0) s_cnt[q] += __popcll(word);   // one writer
            }
        }
        // s_best is written again only behind the barriers of the next 64 gts' first tile (rows > 0 here)
    }
    __syncthreads();
    int32_t *out = p.table + (size_t)b * p.stride;
    if (l == 0 && tid == 0) out[1] = nvalid;
    if (tid < p.t) {
        out[2 + l * p.t + tid] = s_cnt[tid];
        if (p.nlist == 1) out[2 + p.t + tid] = 0;     // no rois: no roi is recalled
    }
}

size_t post_total(int64_t n, int b) { return layout(n).total + arena_sz(4 * (size_t)(b > 0 ? b : 1)); }

}  // namespace

extern "C" int modest_post_process_tile(void) { return PR_TILE; }

extern "C" int modest_post_process_max_thresholds(void) { return PR_MAX_THRESH; }

extern "C" int64_t modest_post_process_workspace_bytes(int64_t n_rows, int batch_size) {
    if (n_rows < 0 || n_rows > 2147483647LL || batch_size < 0 || batch_size > WK_MAX_BATCH) {
        modest_set_error("modest_post_process_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 and 0 <= batch_size <= 65535");
        return MODEST_ERR_ARG;
    }
    return (int64_t)post_total(n_rows, batch_size);
}

extern "C" int modest_post_process(int64_t n_rows, int batch_size, int64_t rows_per_sample, const float *box_dev, int box_cols,
                                   const float *cls_dev, int cls_cols, const void *batch_index_dev, int batch_index_kind,
                                   int normalized, int has_score_thresh, float score_thresh, int output_raw_score,
                                   const int64_t *labels_dev, int pre_maxsize, int post_maxsize, float nms_thresh, int rotated,
                                   int with_gt, int n_gt, const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_n,
                                   int64_t gt_stride_c, int n_rois, const float *rois_dev, int roi_cols, int n_thresh,
                                   const float *recall_thresh_host, float *pred_boxes_dev, float *pred_scores_dev,
                                   int64_t *pred_labels_dev, int32_t *table_pinned_host, void *workspace_dev,
                                   int64_t workspace_bytes, void *stream) {
    WALK_REQUIRE_SIZES();
    MODEST_REQUIRE(n_thresh >= 0 && n_thresh <= PR_MAX_THRESH, "RECALL_THRESH_LIST of at most 16 thresholds (they travel in the kernel's arguments)");
    WALK_REQUIRE_BATCH_INDEX();
    if (batch_index_kind != BIDX_NONE)
        MODEST_REQUIRE(labels_dev == nullptr && n_rois < 0, "given labels and rois need the dense form");
    MODEST_REQUIRE(n_rois >= -1, "n_rois: -1 without rois");
    MODEST_REQUIRE(with_gt || n_rois < 0, "rois without gts");
    if (with_gt) {
        MODEST_REQUIRE(n_gt >= 0 && (int64_t)batch_size * n_gt <= 2147483647LL, "at most 2^31 - 1 gt rows in a call");
        MODEST_REQUIRE(n_gt == 0 || batch_size == 0 || gt_dev, "NULL gt_boxes");
        MODEST_REQUIRE(n_thresh == 0 || recall_thresh_host, "NULL thresholds");
        if (n_rois >= 0) {
            MODEST_REQUIRE((int64_t)batch_size * n_rois <= 2147483647LL, "at most 2^31 - 1 roi rows in a call");
            MODEST_REQUIRE(roi_cols >= 7 && roi_cols <= 4096, "7 + C roi columns, 4096 at most");
            MODEST_REQUIRE(n_rois == 0 || batch_size == 0 || rois_dev, "NULL rois");
        }
    }
    if (batch_size == 0) return MODEST_OK;
    MODEST_REQUIRE(table_pinned_host, "NULL table");
    MODEST_REQUIRE(post_maxsize == 0 || (pred_boxes_dev && pred_scores_dev && pred_labels_dev), "NULL output");
    MODEST_REQUIRE(n_rows == 0 || (box_dev && cls_dev), "NULL buffer");
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)post_total(n_rows, batch_size),
                   "workspace smaller than modest_post_process_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
    hipStream_t st = as_stream(stream);
    PostParams p;
    p.w = walk_params(n_rows, box_dev, box_cols, cls_dev, cls_cols, pre_maxsize, post_maxsize, nms_thresh, pred_boxes_dev,
                      pred_scores_dev, pred_labels_dev);
    if (n_rows > 0) {
        // the sample field holds batch_size itself for a row below the threshold or of no sample
        const int rc = rank_rows<true>(p.w, batch_size, rows_per_sample, batch_index_dev, batch_index_kind, normalized,
                                       has_score_thresh, score_thresh, batch_size, workspace_dev, st);
        if (rc != MODEST_OK) return rc;
    }
    p.normalized = normalized;
    p.raw_out = output_raw_score;
    p.given = labels_dev;
    p.nb = reinterpret_cast<int32_t *>(static_cast<char *>(workspace_dev) + layout(n_rows).total);
    p.table = table_pinned_host;
    p.stride = 2 + 2 * n_thresh;
    if (rotated)
        post_walk<true><<<(unsigned)batch_size, WK_T, 0, st>>>(p);
    else
        post_walk<false><<<(unsigned)batch_size, WK_T, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    if (with_gt) {
        RecallParams r;
        r.g = n_gt;
        r.gt_cols = box_cols + 1;
        r.gt = gt_dev;
        r.gs0 = gt_stride_b;
        r.gs1 = gt_stride_n;
        r.gs2 = gt_stride_c;
        r.nb = p.nb;
        if (n_rois >= 0) {   // the reference then takes ALL of the sample's rows for "rcnn", and the rois for "roi"
            r.nlist = 2;
            r.list[0] = box_dev;  r.cols[0] = box_cols;  r.per[0] = (int)rows_per_sample;  r.from_nb[0] = 0;
            r.list[1] = rois_dev; r.cols[1] = roi_cols;  r.per[1] = n_rois;                r.from_nb[1] = 0;
        } else {
            r.nlist = 1;
            r.list[0] = pred_boxes_dev; r.cols[0] = box_cols; r.per[0] = post_maxsize; r.from_nb[0] = 1;
            r.list[1] = nullptr;        r.cols[1] = 7;        r.per[1] = 0;            r.from_nb[1] = 0;
        }
        r.t = n_thresh;
        for (int q = 0; q < PR_MAX_THRESH; ++q) r.thr[q] = q < n_thresh ? recall_thresh_host[q] : 0.f;
        r.table = table_pinned_host;
        r.stride = p.stride;
        post_recall<<<dim3((unsigned)batch_size, (unsigned)r.nlist), PR_T, 0, st>>>(r);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    MODEST_HIP_CHECK(hipStreamSynchronize(st));
    return MODEST_OK;
}
