// RoI target assignment of OpenPCDet's two-stage detectors (RoIHeadTemplate.assign_targets,
// pcdet/models/roi_heads/roi_head_template.py:101-131, over ProposalTargetLayer.forward,
// roi_heads/target_assigner/proposal_target_layer.py), hand-written for gfx950.  Two entry points (include/modest_hip.h,
// "a32"), split as modest_voxelize_plan / _fill are, because the reference draws its samples from the HOST generators
// with the list lengths as arguments: the three counts of every sample have to reach the host once.  No context, no
// device allocation; the caller supplies the workspace.  DESIGN.md section 7n.
//
//   rt_match    one workgroup per sample, one launch: (1) trim -- the last gt row whose f32 sum in column order is not
//               == 0; (2) match -- the valid gts and their trig staged in LDS RT_TILE at a time, a lane per roi, the 3-D
//               IoU in the reference's f32 operations and order over box_overlap of csrc/iou_bev.h (the BEV overlap of
//               boxes_overlap_bev_gpu), the maximum and its gt row (the lowest row among equal maxima, the first NaN above
//               every number), with by_class only the gts of the roi's label; (3) classify and compact -- the fg / hard /
//               easy lists in ascending roi order by ballots and a prefix over the wavefronts' totals; the three counts go
//               to the workspace and straight into the caller's pinned words.  modest_roi_targets_match then synchronises
//               the stream: its one host wait.
//   rt_sample   a lane per output slot: the pick (list, position) resolved through the workspace to a roi row and its gt
//               row, the gathered columns, the labels and the canonical transform.  A pick outside its list writes a zero
//               slot; nothing is read out of bounds.  Enqueue only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "iou_bev.h"
#include "iou3d_steps.h"

namespace {

constexpr int RT_WAVES = 8;                  // wavefronts of a match workgroup: each owns a PolyLds (18 432 B)
constexpr int RT_T = 64 * RT_WAVES;
constexpr int RT_TILE = 64;                  // gts staged in LDS at a time (modest_roi_targets_gt_tile)
constexpr int RT_REC = 12;                   // box (7) + cos h, sin h, cos(-h), sin(-h) + label
constexpr int RT_MAX_BATCH = 65535;          // grid.x of both kernels' sample dimension
constexpr int RT_MAX_COLS = 4096;
// LDS of rt_match: 8 * 18432 (PolyLds) + 64 * 12 * 4 (gt tile) + 3 * 8 * 4 (list totals) + 4 = 150 628 B of the CU's 160 KB.

enum { LIST_FG = 0, LIST_HARD = 1, LIST_EASY = 2 };
enum { SCORE_CLS = 0, SCORE_ROI_IOU = 1 };

struct Layout {
    size_t counts, iou, assign, list[3], total;
};

Layout layout(int64_t b, int64_t r) {
    Layout L;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += arena_sz(bytes);
        return at;
    };
    const size_t rows = (size_t)(b * r > 0 ? b * r : 1);
    L.counts = take(4 * 3 * (size_t)(b > 0 ? b : 1));
    L.iou = take(4 * rows);
    L.assign = take(4 * rows);
    for (int l = 0; l < 3; ++l) L.list[l] = take(4 * rows);
    L.total = off;
    return L;
}

struct MatchParams {
    int r, g, gt_cols;                 // rois and gt rows per sample, 7 + C + 1
    const float *rois;                 // (B, r, roi_cols)
    int roi_cols;
    const int64_t *labels;             // (B, r)
    const float *gt;                   // (B, g, gt_cols) by strides, in elements
    int64_t gs0, gs1, gs2;
    float fg_thresh, bg_lo, reg_fg;    // min(REG_FG, CLS_FG), CLS_BG_THRESH_LO, REG_FG_THRESH
    int by_class;
    float *iou;                        // workspace
    int32_t *assign, *list[3], *counts;
    int32_t *pinned;                   // (B, 3) host words
};

__global__ __launch_bounds__(RT_T) void rt_match(MatchParams p) {
    __shared__ PolyLds s_poly[RT_WAVES];
    __shared__ float s_gt[RT_TILE][RT_REC];
    __shared__ int s_tot[3][RT_WAVES];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const float *gt = p.gt + (int64_t)b * p.gs0;
    // (1) trim: the last row whose sum is not == 0 (a NaN sum is not), row 0 at the least
    if (tid == 0) s_last = 0;
    __syncthreads();
    int last = 0;
    for (int j = tid; j < p.g; j += RT_T) {
        const float *row = gt + (int64_t)j * p.gs1;
        float s = row[0];
        for (int c = 1; c < p.gt_cols; ++c) s = s + row[(int64_t)c * p.gs2];
        if (!(s == 0.f)) last = j;
    }
    if (last > 0) atomicMax(&s_last, last);
    __syncthreads();
    const int nvalid = s_last + 1;   // with g == 0: one box of zeros, never read from memory
    PolyLds &L = s_poly[w];
    int run[3] = {0, 0, 0};          // list lengths so far: the same in every lane
    for (int r0 = 0; r0 < p.r; r0 += RT_T) {
        const int r = r0 + tid;
        const bool live = r < p.r;
        float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int64_t label = 0;
        if (live) {
            const float *src = p.rois + ((size_t)b * p.r + r) * p.roi_cols;
#pragma unroll
            for (int q = 0; q < 7; ++q) a[q] = src[q];
            label = p.labels[(size_t)b * p.r + r];
        }
        const float4 ta = device_trig(a[6]);
        const Iou3dSide sa = iou3d_side(a);
        // (2) match
        float best = 0.f;
        int at = 0;
        bool any = false;
        for (int g0 = 0; g0 < nvalid; g0 += RT_TILE) {
            const int m = min(RT_TILE, nvalid - g0);
            __syncthreads();   // the tile before has been read
            if (tid < m) {
                float bx[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                float lab = 0.f;
                if (p.g > 0) {
                    const float *row = gt + (int64_t)(g0 + tid) * p.gs1;
#pragma unroll
                    for (int q = 0; q < 7; ++q) bx[q] = row[(int64_t)q * p.gs2];
                    lab = row[(int64_t)(p.gt_cols - 1) * p.gs2];
                }
                const float4 t = device_trig(bx[6]);
#pragma unroll
                for (int q = 0; q < 7; ++q) s_gt[tid][q] = bx[q];
                s_gt[tid][7] = t.x; s_gt[tid][8] = t.y; s_gt[tid][9] = t.z; s_gt[tid][10] = t.w;
                s_gt[tid][11] = lab;
            }
            __syncthreads();
            if (live) {
                for (int k = 0; k < m; ++k) {
                    if (p.by_class && (int64_t)s_gt[k][11] != label) continue;
                    float bb[7];
#pragma unroll
                    for (int q = 0; q < 7; ++q) bb[q] = s_gt[k][q];
                    const float4 tb = make_float4(s_gt[k][7], s_gt[k][8], s_gt[k][9], s_gt[k][10]);
                    const float v = iou3d_from_bev(sa, bb, box_overlap(a, bb, ta, tb, L));   // csrc/iou3d_steps.h
                    if (!any || v > best || (v != v && best == best)) {
                        best = v;
                        at = g0 + k;
                        any = true;
                    }
                }
            }
        }
        if (live) {
            p.iou[(size_t)b * p.r + r] = best;
            p.assign[(size_t)b * p.r + r] = at;
        }
        // (3) classify and compact: ascending roi order
        const bool flag[3] = {live && best >= p.fg_thresh, live && best < p.reg_fg && best >= p.bg_lo, live && best < p.bg_lo};
        int pre[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const unsigned long long word = __ballot(flag[l]);
            pre[l] = __popcll(word & ((1ull << lane) - 1ull));
            if (lane == 0) s_tot[l][w] = __popcll(word);
        }
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            int before = 0, all = 0;
#pragma unroll
            for (int q = 0; q < RT_WAVES; ++q) {
                const int t = s_tot[l][q];
                before += q < w ? t : 0;
                all += t;
            }
            if (flag[l]) p.list[l][(size_t)b * p.r + run[l] + before + pre[l]] = r;
            run[l] += all;
        }
        // s_tot is written again only after the barriers of the next chunk's first tile
    }
    if (tid < 3) {
        p.counts[b * 3 + tid] = run[tid];
        p.pinned[b * 3 + tid] = run[tid];
    }
}

struct SampleParams {
    int r, g, m;
    int roi_cols, gt_cols;
    const int32_t *picks;              // (B, m, 2): list, position
    const float *iou;                  // workspace of the match call
    const int32_t *assign, *list[3], *counts;
    const float *rois_in, *scores_in;
    const int64_t *labels_in;
    const float *gt;
    int64_t gs0, gs1, gs2;
    float reg_fg, cls_fg, cls_bg, den;   // den: CLS_FG - CLS_BG, the double difference rounded once
    int score_type;
    float *rois, *scores, *gt_iou, *gt_src, *gt_can;
    int64_t *labels, *reg_valid;
    void *cls_labels;                  // int64 (cls) or float32 (roi_iou)
};

// torch's remainder of two float32: fmod, then the divisor's sign
__device__ __forceinline__ float rem_f32(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.f && ((b < 0.f) != (m < 0.f))) m = m + b;
    return m;
}

__global__ __launch_bounds__(256) void rt_sample(SampleParams p) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (slot >= p.m) return;
    const size_t o = (size_t)b * p.m + slot;
    const int list = p.picks[o * 2], pos = p.picks[o * 2 + 1];
    bool ok = list >= 0 && list < 3 && pos >= 0;
    int r = 0, g = 0;
    float iou = 0.f;
    if (ok) ok = pos < p.counts[b * 3 + list] && p.counts[b * 3 + list] <= p.r;
    if (ok) {
        r = (list == LIST_FG ? p.list[0] : list == LIST_HARD ? p.list[1] : p.list[2])[(size_t)b * p.r + pos];
        ok = r >= 0 && r < p.r;
    }
    if (ok) {
        g = p.assign[(size_t)b * p.r + r];
        iou = p.iou[(size_t)b * p.r + r];
        ok = g >= 0 && (g < p.g || (p.g == 0 && g == 0));
    }
    float *rois = p.rois + o * p.roi_cols, *src = p.gt_src + o * p.gt_cols, *can = p.gt_can + o * p.gt_cols;
    if (!ok) {   // a pick outside its list: a slot of zeros
        for (int c = 0; c < p.roi_cols; ++c) rois[c] = 0.f;
        for (int c = 0; c < p.gt_cols; ++c) src[c] = can[c] = 0.f;
        p.scores[o] = 0.f;
        p.gt_iou[o] = 0.f;
        p.labels[o] = 0;
        p.reg_valid[o] = 0;
        if (p.score_type == SCORE_CLS) static_cast<int64_t *>(p.cls_labels)[o] = 0;
        else static_cast<float *>(p.cls_labels)[o] = 0.f;
        return;
    }
    const float *roi = p.rois_in + ((size_t)b * p.r + r) * p.roi_cols;
    for (int c = 0; c < p.roi_cols; ++c) rois[c] = roi[c];
    p.scores[o] = p.scores_in[(size_t)b * p.r + r];
    p.labels[o] = p.labels_in[(size_t)b * p.r + r];
    p.gt_iou[o] = iou;
    p.reg_valid[o] = iou > p.reg_fg ? 1 : 0;
    if (p.score_type == SCORE_CLS) {
        int64_t v = iou > p.cls_fg ? 1 : 0;
        if (iou > p.cls_bg && iou < p.cls_fg) v = -1;
        static_cast<int64_t *>(p.cls_labels)[o] = v;
    } else {
        const bool fg = iou > p.cls_fg, bg = iou < p.cls_bg;
        float v = fg ? 1.f : 0.f;
        if (!fg && !bg) v = (iou - p.cls_bg) / p.den;   // a NaN lands here and stays
        static_cast<float *>(p.cls_labels)[o] = v;
    }
    // the gt row, and its canonical form
    const float *gt = p.gt + (int64_t)b * p.gs0 + (int64_t)g * p.gs1;
    for (int c = 0; c < p.gt_cols; ++c) {
        const float v = p.g > 0 ? gt[(int64_t)c * p.gs2] : 0.f;
        src[c] = v;
        can[c] = v;
    }
    const float TWO_PI = 6.28318530717958647692f, PI = 3.14159265358979323846f;
    const float HALF_PI = 1.57079632679489661923f, PI_3_2 = 4.71238898038468985769f;
    const float ry = rem_f32(roi[6], TWO_PI);
    const float x = src[0] - roi[0], y = src[1] - roi[1], z = src[2] - roi[2];
    const float ang = -ry;
    const float c = modest::cos_f32(ang), s = modest::sin_f32(ang);
    // matmul of (x, y, z) with [[c, s, 0], [-s, c, 0], [0, 0, 1]]: products rounded, summed in column order
    can[0] = x * c + y * (-s) + z * 0.f;
    can[1] = x * s + y * c + z * 0.f;
    can[2] = x * 0.f + y * 0.f + z * 1.f;
    float h = rem_f32(src[6] - ry, TWO_PI);
    if (h > HALF_PI && h < PI_3_2) h = rem_f32(h + PI, TWO_PI);
    if (h > PI) h = h - TWO_PI;
    if (h < -HALF_PI) h = -HALF_PI;   // clamp: a NaN stays
    if (h > HALF_PI) h = HALF_PI;
    can[6] = h;
}

// the limits shared by both calls (MODEST_REQUIRE names the calling function)
#define RT_CHECK_SHAPES(batch_size, n_rois, n_gt, roi_cols, m)                                                                 \
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= RT_MAX_BATCH, "batch_size at most 65535 (one workgroup row per sample)");  \
    MODEST_REQUIRE(roi_cols >= 7 && roi_cols <= RT_MAX_COLS, "7 + C roi columns, 4096 at most");                               \
    MODEST_REQUIRE(n_rois >= 0 && n_gt >= 0, "negative row count");                                                            \
    MODEST_REQUIRE((int64_t)batch_size * n_rois <= 2147483647LL && (int64_t)batch_size * n_gt <= 2147483647LL,                 \
                   "at most 2^31 - 1 roi rows and gt rows in a call");                                                         \
    MODEST_REQUIRE(m >= 1, "ROI_PER_IMAGE at least 1");                                                                        \
    MODEST_REQUIRE((int64_t)batch_size * m <= 2147483647LL, "at most 2^31 - 1 output rows in a call")

}  // namespace

extern "C" int modest_roi_targets_gt_tile(void) { return RT_TILE; }

extern "C" int64_t modest_roi_targets_workspace_bytes(int batch_size, int n_rois) {
    if (batch_size < 0 || batch_size > RT_MAX_BATCH || n_rois < 0 || (int64_t)batch_size * n_rois > 2147483647LL) {
        modest_set_error("modest_roi_targets_workspace_bytes: requirement failed: 0 <= batch_size <= 65535 and at most 2^31 - 1 roi rows in a call");
        return MODEST_ERR_ARG;
    }
    return (int64_t)layout(batch_size, n_rois).total;
}

extern "C" int modest_roi_targets_workspace_offsets(int batch_size, int n_rois, int64_t *offsets_host) {
    MODEST_REQUIRE(batch_size >= 0 && batch_size <= RT_MAX_BATCH, "0 <= batch_size <= 65535");
    MODEST_REQUIRE(n_rois >= 0 && (int64_t)batch_size * n_rois <= 2147483647LL, "at most 2^31 - 1 roi rows in a call");
    MODEST_REQUIRE(offsets_host, "NULL offsets");
    const Layout L = layout(batch_size, n_rois);
    const size_t at[6] = {L.counts, L.iou, L.assign, L.list[LIST_FG], L.list[LIST_HARD], L.list[LIST_EASY]};
    for (int k = 0; k < 6; ++k) offsets_host[k] = (int64_t)at[k];
    return MODEST_OK;
}

extern "C" int modest_roi_targets_match(int batch_size, int n_rois, int n_gt, const float *rois_dev, int roi_cols,
                                        const int64_t *roi_labels_dev, const float *gt_dev, int64_t gt_stride_b,
                                        int64_t gt_stride_n, int64_t gt_stride_c, float fg_thresh, float bg_thresh_lo,
                                        float reg_fg_thresh, int by_class, void *workspace_dev, int64_t workspace_bytes,
                                        int32_t *counts_pinned_host, void *stream) {
    RT_CHECK_SHAPES(batch_size, n_rois, n_gt, roi_cols, 1);
    if (batch_size == 0) return MODEST_OK;
    MODEST_REQUIRE(counts_pinned_host, "NULL counts");
    MODEST_REQUIRE(n_rois == 0 || (rois_dev && roi_labels_dev), "NULL buffer");
    MODEST_REQUIRE(n_gt == 0 || gt_dev, "NULL gt_boxes");
    const Layout L = layout(batch_size, n_rois);
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)L.total, "workspace smaller than modest_roi_targets_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
    char *ws = static_cast<char *>(workspace_dev);
    MatchParams p;
    p.r = n_rois;
    p.g = n_gt;
    p.gt_cols = roi_cols + 1;
    p.rois = rois_dev;
    p.roi_cols = roi_cols;
    p.labels = roi_labels_dev;
    p.gt = gt_dev;
    p.gs0 = gt_stride_b;
    p.gs1 = gt_stride_n;
    p.gs2 = gt_stride_c;
    p.fg_thresh = fg_thresh;
    p.bg_lo = bg_thresh_lo;
    p.reg_fg = reg_fg_thresh;
    p.by_class = by_class;
    p.iou = reinterpret_cast<float *>(ws + L.iou);
    p.assign = reinterpret_cast<int32_t *>(ws + L.assign);
    for (int l = 0; l < 3; ++l) p.list[l] = reinterpret_cast<int32_t *>(ws + L.list[l]);
    p.counts = reinterpret_cast<int32_t *>(ws + L.counts);
    p.pinned = counts_pinned_host;
    hipStream_t st = as_stream(stream);
    rt_match<<<(unsigned)batch_size, RT_T, 0, st>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    MODEST_HIP_CHECK(hipStreamSynchronize(st));
    return MODEST_OK;
}

extern "C" int modest_roi_targets_sample(int batch_size, int n_rois, int n_gt, int roi_per_image, const int32_t *picks,
                                         const float *rois_dev, int roi_cols, const float *roi_scores_dev,
                                         const int64_t *roi_labels_dev, const float *gt_dev, int64_t gt_stride_b,
                                         int64_t gt_stride_n, int64_t gt_stride_c, float reg_fg_thresh, float cls_fg_thresh,
                                         float cls_bg_thresh, float fg_minus_bg, int score_type,
                                         const void *workspace_dev, int64_t workspace_bytes, float *out_rois_dev,
                                         float *out_gt_of_rois_dev, float *out_gt_iou_dev, float *out_roi_scores_dev,
                                         int64_t *out_roi_labels_dev, int64_t *out_reg_valid_dev, void *out_cls_labels_dev,
                                         float *out_gt_of_rois_src_dev, void *stream) {
    RT_CHECK_SHAPES(batch_size, n_rois, n_gt, roi_cols, roi_per_image);
    MODEST_REQUIRE(score_type == SCORE_CLS || score_type == SCORE_ROI_IOU, "score type: 0 cls, 1 roi_iou");
    if (batch_size == 0) return MODEST_OK;
    MODEST_REQUIRE(picks, "NULL picks");
    MODEST_REQUIRE(n_rois == 0 || (rois_dev && roi_scores_dev && roi_labels_dev), "NULL buffer");
    MODEST_REQUIRE(n_gt == 0 || gt_dev, "NULL gt_boxes");
    MODEST_REQUIRE(out_rois_dev && out_gt_of_rois_dev && out_gt_iou_dev && out_roi_scores_dev && out_roi_labels_dev &&
                       out_reg_valid_dev && out_cls_labels_dev && out_gt_of_rois_src_dev, "NULL output");
    const Layout L = layout(batch_size, n_rois);
    MODEST_REQUIRE(workspace_dev && workspace_bytes >= (int64_t)L.total, "workspace smaller than modest_roi_targets_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace not 8-byte aligned");
    const char *ws = static_cast<const char *>(workspace_dev);
    SampleParams p;
    p.r = n_rois;
    p.g = n_gt;
    p.m = roi_per_image;
    p.roi_cols = roi_cols;
    p.gt_cols = roi_cols + 1;
    p.picks = picks;
    p.iou = reinterpret_cast<const float *>(ws + L.iou);
    p.assign = reinterpret_cast<const int32_t *>(ws + L.assign);
    for (int l = 0; l < 3; ++l) p.list[l] = reinterpret_cast<const int32_t *>(ws + L.list[l]);
    p.counts = reinterpret_cast<const int32_t *>(ws + L.counts);
    p.rois_in = rois_dev;
    p.scores_in = roi_scores_dev;
    p.labels_in = roi_labels_dev;
    p.gt = gt_dev;
    p.gs0 = gt_stride_b;
    p.gs1 = gt_stride_n;
    p.gs2 = gt_stride_c;
    p.reg_fg = reg_fg_thresh;
    p.cls_fg = cls_fg_thresh;
    p.cls_bg = cls_bg_thresh;
    p.den = fg_minus_bg;
    p.score_type = score_type;
    p.rois = out_rois_dev;
    p.scores = out_roi_scores_dev;
    p.gt_iou = out_gt_iou_dev;
    p.gt_src = out_gt_of_rois_src_dev;
    p.gt_can = out_gt_of_rois_dev;
    p.labels = out_roi_labels_dev;
    p.reg_valid = out_reg_valid_dev;
    p.cls_labels = out_cls_labels_dev;
    const dim3 grid((unsigned)((roi_per_image + 255) / 256), (unsigned)batch_size);
    rt_sample<<<grid, 256, 0, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
