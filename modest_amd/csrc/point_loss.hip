// Loss of OpenPCDet's point heads with its gradients (PointHeadBox / PointIntraPartOffsetHead / PointHeadSimple .get_loss over
// get_cls_layer_loss, get_part_layer_loss and get_box_layer_loss of pcdet/models/dense_heads/point_head_template.py:131-191,
// SigmoidFocalClassificationLoss and WeightedSmoothL1Loss of pcdet/utils/loss_utils.py), hand-written for gfx950.  Two entry
// points (include/modest_hip.h, "a36"): enqueue only, no synchronise, no context, no device allocation, nothing read back.
//
// The one-hot tensor of the reference is never formed, and a point that is not positive costs the part and box terms nothing
// but its zero gradient rows: their tensors are not read there.  Kernels:
//   pl_count   positives (label > 0) of the WHOLE stacked batch: ballot + popcount per wavefront over 16 rows a lane, one INTEGER
//              atomic add per wavefront into a counter the call zeroes first (integer sums do not depend on arrival order);
//   pl_loss    one lane per point, 256 per workgroup: the C focal terms and their gradients for every lane; part and box terms
//              for positive lanes only, zero gradient rows for the others; the three sums of the workgroup into the partials
//              array;
//   pl_finish  one workgroup: the partials' sums, then the table;
//   pl_scale   (modest_point_loss_backward) the three gradient buffers times the upstream gradient read from the device.
// The arithmetic, the terms and the summation tree are those of csrc/loss_terms.h (DESIGN.md sections 7p and 7r).  Nothing is
// indexed by an input value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "loss_terms.h"

namespace {

using namespace modest::loss;

constexpr int PL_MAX_CLASS = 32, PL_MAX_CODE = 16, PL_PART = 3;
constexpr int PL_COUNT_ROWS = 16;  // rows a lane of pl_count looks at
constexpr int64_t PL_MAX_ROWS = 1 << 24;   // the count of positives stays exact as a float32

struct PointLossParams {
    int64_t n, blocks;
    int c, code, lab64, want_grad;
    const float *cls, *part, *part_t, *box, *box_t, *cw;
    const void *labels;
    SmoothL1 sl1;
    float alpha, one_m_alpha, floor100, eps12;
    float w_cls, w_part, w_box;    // the loss weights: also the gradients that reach the summed cls and box terms
    float *gcls, *gpart, *gbox, *out;
    int32_t *cnt;                  // (1) positives of the whole batch
    float *sums;                   // (3, blocks) workgroup sums
};

// 16 rows a lane, a workgroup over 4096 consecutive rows: the one atomic of a wavefront then stands for 1024 rows, and the
// single counter sees N / 1024 additions (one per 64 rows took longer than pl_loss itself at N = 65 536)
__global__ __launch_bounds__(LANES) void pl_count(PointLossParams p) {
    const int64_t base = (int64_t)blockIdx.x * (LANES * PL_COUNT_ROWS) + threadIdx.x;
    int n_pos = 0;
#pragma unroll 4
    for (int k = 0; k < PL_COUNT_ROWS; ++k) {
        const int64_t i = base + (int64_t)k * LANES;
        const bool pos = i < p.n && label_i32(p.labels, p.lab64, i) > 0;
        n_pos += __popcll(__ballot(pos));
    }
    if ((threadIdx.x & 63) == 0 && n_pos) atomicAdd(p.cnt, n_pos);
}

__global__ __launch_bounds__(LANES) void pl_loss(PointLossParams p) {
    const int64_t row = (int64_t)blockIdx.x * LANES + threadIdx.x;
    float sum_cls = 0.f, sum_part = 0.f, sum_box = 0.f;
    if (row < p.n) {
        const int label = label_i32(p.labels, p.lab64, row);
        const int n_pos = p.cnt[0] > 1 ? p.cnt[0] : 1;
        const float w = 1.0f / (float)n_pos;
        const float wc = label >= 0 ? w : 0.f, wr = label > 0 ? w : 0.f;
        // ---- classification: the focal term, the target strictly label == c + 1
        const float gw = p.w_cls * wc;
        for (int c = 0; c < p.c; ++c)
            sum_cls = sum_cls + focal_term(p.cls[row * p.c + c], label == c + 1 ? 1.f : 0.f, p.alpha, p.one_m_alpha, wc, gw,
                                           p.want_grad ? p.gcls + row * p.c + c : nullptr);
        // ---- part: binary cross entropy of the sigmoid, positive rows only
        if (p.part) {
            float *gp = p.want_grad ? p.gpart + row * PL_PART : nullptr;
            if (label > 0) {
                const float *xp = p.part + row * PL_PART, *tp = p.part_t + row * PL_PART;
                const float g0 = p.w_part / (float)(3 * n_pos);
#pragma unroll
                for (int k = 0; k < PL_PART; ++k)
                    sum_part = sum_part + bce_term(xp[k], tp[k], g0, p.floor100, p.eps12, gp ? gp + k : nullptr);
            } else if (gp) {
#pragma unroll
                for (int k = 0; k < PL_PART; ++k) gp[k] = 0.f;
            }
        }
        // ---- box: smooth L1 of the code-weighted difference, positive rows only
        if (p.box) {
            float *gb = p.want_grad ? p.gbox + row * p.code : nullptr;
            if (label > 0) {
                const float *bp = p.box + row * p.code, *tg = p.box_t + row * p.code;
                const float gl = p.w_box * wr;
                for (int k = 0; k < p.code; ++k) {
                    float g_in, g_t;
                    sum_box = sum_box + smooth_l1_term(bp[k], tg[k], p.cw[k], gl, p.sl1, g_in, g_t) * wr;
                    if (gb) gb[k] = g_in;
                }
            } else if (gb) {
                for (int k = 0; k < p.code; ++k) gb[k] = 0.f;
            }
        }
    }
    workgroup_sums(sum_cls, sum_part, sum_box, p.sums, p.blocks, blockIdx.x);
}

__global__ __launch_bounds__(LANES) void pl_finish(PointLossParams p) {
    float v[3];
    finish_sums(p.sums, p.blocks, v);
    if (threadIdx.x == 0) {
        const int n_pos = p.cnt[0];
        const float cls = v[0] * p.w_cls;
        const float part = p.part ? (v[1] / (float)(3 * (n_pos > 1 ? n_pos : 1))) * p.w_part : 0.f;
        const float box = p.box ? v[2] * p.w_box : 0.f;
        float loss = cls;                      // absent terms are skipped, not added as 0
        if (p.part) loss = loss + part;
        if (p.box) loss = loss + box;
        p.out[0] = cls;
        p.out[1] = part;
        p.out[2] = box;
        p.out[3] = loss;
        p.out[4] = (float)n_pos;
    }
}

__global__ __launch_bounds__(LANES) void pl_scale(int64_t n0, int64_t n1, int64_t n2, float *__restrict__ g0,
                                                 float *__restrict__ g1, float *__restrict__ g2,
                                                 const float *__restrict__ upstream) {
    scale_grads(n0, n1, n2, g0, g1, g2, upstream);
}

size_t ws_counter() { return arena_sz(4); }
size_t ws_total(int64_t n) { return ws_counter() + arena_sz(4 * 3 * (size_t)(blocks_of(n) > 0 ? blocks_of(n) : 1)); }

}  // namespace

extern "C" int64_t modest_point_loss_max_rows(void) { return PL_MAX_ROWS; }

extern "C" int64_t modest_point_loss_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows > PL_MAX_ROWS) {
        modest_set_error("modest_point_loss_workspace_bytes: requirement failed: 0 <= n_rows <= 2^24");
        return MODEST_ERR_ARG;
    }
    return (int64_t)ws_total(n_rows);
}

extern "C" int modest_point_loss(int64_t n_rows, int num_class, int code, const float *cls_preds_dev, const void *labels_dev,
                                 int labels_int64, const float *part_preds_dev, const float *part_labels_dev,
                                 const float *box_preds_dev, const float *box_labels_dev, const float *code_weights_dev,
                                 float beta, float cls_weight, float part_weight, float box_weight, float *grad_cls_dev,
                                 float *grad_part_dev, float *grad_box_dev, float *table_dev, void *workspace_dev,
                                 int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= PL_MAX_ROWS, "n_rows between 0 and 2^24 (the count of positives stays exact in float32)");
    MODEST_REQUIRE(num_class >= 1 && num_class <= PL_MAX_CLASS, "num_class between 1 and 32");
    const bool with_part = part_preds_dev != nullptr, with_box = box_preds_dev != nullptr;
    MODEST_REQUIRE(!with_box || (code >= 1 && code <= PL_MAX_CODE), "code size between 1 and 16");
    MODEST_REQUIRE(with_part == (part_labels_dev != nullptr), "part_preds and part_labels come together");
    MODEST_REQUIRE(with_box == (box_labels_dev != nullptr) && with_box == (code_weights_dev != nullptr),
                   "box_preds, box_labels and code_weights come together");
    MODEST_REQUIRE(table_dev && workspace_dev && ((uintptr_t)workspace_dev & 3) == 0, "NULL or unaligned buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)ws_total(n_rows), "workspace smaller than modest_point_loss_workspace_bytes");
    const bool want = grad_cls_dev != nullptr;
    MODEST_REQUIRE((grad_part_dev != nullptr) == (want && with_part) && (grad_box_dev != nullptr) == (want && with_box),
                   "the gradient buffers come together, one per term");
    MODEST_REQUIRE(n_rows == 0 || (cls_preds_dev && labels_dev), "NULL buffer");
    PointLossParams p;
    p.n = n_rows; p.blocks = blocks_of(n_rows);
    p.c = num_class; p.code = with_box ? code : 0; p.lab64 = labels_int64 ? 1 : 0;
    p.want_grad = want ? 1 : 0;
    p.cls = cls_preds_dev; p.part = part_preds_dev; p.part_t = part_labels_dev; p.box = box_preds_dev; p.box_t = box_labels_dev;
    p.cw = code_weights_dev; p.labels = labels_dev;
    p.sl1 = smooth_l1_of(beta);
    p.alpha = 0.25f; p.one_m_alpha = 0.75f; p.floor100 = -100.f; p.eps12 = (float)1e-12;
    p.w_cls = cls_weight; p.w_part = part_weight; p.w_box = box_weight;
    p.gcls = grad_cls_dev; p.gpart = grad_part_dev; p.gbox = grad_box_dev; p.out = table_dev;
    char *ws = static_cast<char *>(workspace_dev);
    p.cnt = reinterpret_cast<int32_t *>(ws);
    p.sums = reinterpret_cast<float *>(ws + ws_counter());
    hipStream_t s = as_stream(stream);
    MODEST_HIP_CHECK(hipMemsetAsync(p.cnt, 0, 4, s));
    if (p.blocks > 0) {
        pl_count<<<(unsigned)((n_rows + LANES * PL_COUNT_ROWS - 1) / (LANES * PL_COUNT_ROWS)), LANES, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
        pl_loss<<<(unsigned)p.blocks, LANES, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    pl_finish<<<1, LANES, 0, s>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_point_loss_backward(int64_t n_cls, int64_t n_part, int64_t n_box, float *grad_cls_dev, float *grad_part_dev,
                                          float *grad_box_dev, const float *upstream_dev, void *stream) {
    MODEST_REQUIRE(n_cls >= 0 && n_part >= 0 && n_box >= 0, "negative size");
    MODEST_REQUIRE(n_cls <= PL_MAX_ROWS * PL_MAX_CLASS && n_part <= PL_MAX_ROWS * PL_PART && n_box <= PL_MAX_ROWS * PL_MAX_CODE,
                   "more gradient elements than 2^24 rows of 32, 3 and 16 columns");
    MODEST_REQUIRE((n_cls == 0 || grad_cls_dev) && (n_part == 0 || grad_part_dev) && (n_box == 0 || grad_box_dev), "NULL buffer");
    const int64_t total = n_cls + n_part + n_box;
    if (total == 0) return MODEST_OK;
    MODEST_REQUIRE(upstream_dev, "NULL upstream gradient");
    pl_scale<<<(unsigned)blocks_of(total), LANES, 0, as_stream(stream)>>>(n_cls, n_part, n_box, grad_cls_dev, grad_part_dev, grad_box_dev,
                                                                        upstream_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
