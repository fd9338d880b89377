// Loss of OpenPCDet's anchor heads with its gradients (AnchorHeadTemplate.get_loss,
// pcdet/models/dense_heads/anchor_head_template.py:101-223, over SigmoidFocalClassificationLoss, WeightedSmoothL1Loss /
// WeightedL1Loss and WeightedCrossEntropyLoss of pcdet/utils/loss_utils.py), hand-written for gfx950.  Two entry points
// (include/modest_hip.h, "a34"): enqueue only, no synchronise, no context, no device allocation, nothing read back.
//
// The one-hot tensors, the repeated anchors and the concatenated box tensors of the reference are never formed, and an
// anchor that is not positive costs the box and direction terms nothing but its zero gradient rows.  Kernels:
//   al_count   positives per sample: ballot + popcount per wavefront, one INTEGER atomic add per wavefront into a counter the
//              call zeroes first (integer sums do not depend on arrival order);
//   al_loss    one lane per anchor, 256 per workgroup, a workgroup inside one sample: the C focal terms and their gradients
//              for every lane; box (column 6 as sin(p - t) in two products) and direction terms for positive lanes only, zero
//              gradient rows for the others; the three sums of the workgroup into the partials array;
//   al_finish  one workgroup: the partials' sums, then the four scalars;
//   al_scale   (modest_anchor_loss_backward) the three gradient buffers times the upstream gradient read from the device.
// The arithmetic, the terms and the summation tree are those of csrc/loss_terms.h; sin / cos are
// csrc/trig_f32.h's.  The direction cross entropy is this file's own.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "loss_terms.h"
#include "trig_f32.h"

namespace {

using namespace modest::loss;

constexpr int AL_MAX_CLASS = 32, AL_MAX_CODE = 16, AL_MAX_BINS = 8, AL_MAX_BATCH = 65535;

struct LossParams {
    int b, c, code, bins, a_cols, lab64, want_grad;
    int64_t n, blocks;             // anchors per sample, workgroups per sample
    const float *cls, *box, *dir, *tg, *anchors, *cw;
    const void *labels;
    SmoothL1 sl1;
    float dir_offset, two_pi, bin_width, alpha, one_m_alpha;
    float g_cls, g_loc, g_dir;     // fl(weight / B): the gradient that reaches the summed terms
    float w_cls, w_loc, w_dir, fb; // the loss weights and float(B)
    float *gcls, *gbox, *gdir, *out;
    int32_t *cnt;                  // (B) positives
    float *part;                   // (3, B * blocks) workgroup sums
};

__global__ __launch_bounds__(LANES) void al_count(LossParams p) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    const bool pos = i < p.n && label_i32(p.labels, p.lab64, (int64_t)b * p.n + i) > 0;
    const unsigned long long mask = __ballot(pos);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(p.cnt + b, __popcll(mask));
}

__global__ __launch_bounds__(LANES) void al_loss(LossParams p) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    float sum_cls = 0.f, sum_loc = 0.f, sum_dir = 0.f;
    if (i < p.n) {
        const int64_t row = (int64_t)b * p.n + i;
        const int label = label_i32(p.labels, p.lab64, row);
        const float w = 1.0f / fmaxf((float)p.cnt[b], 1.0f);
        const float wc = label >= 0 ? w : 0.f, wr = label > 0 ? w : 0.f;
        // ---- classification: the focal term, the target label == c + 1 or, with one class, any positive label
        const float gw = p.g_cls * wc;
        for (int c = 0; c < p.c; ++c) {
            const float t = (label == c + 1 || (p.c == 1 && label > 0)) ? 1.f : 0.f;
            sum_cls = sum_cls + focal_term(p.cls[row * p.c + c], t, p.alpha, p.one_m_alpha, wc, gw,
                                           p.want_grad ? p.gcls + row * p.c + c : nullptr);
        }
        // ---- box regression: smooth L1 (or L1) of the code-weighted difference, column 6 as sin(p - t) in two products
        const float *bp = p.box + row * p.code, *tg = p.tg + row * p.code;
        float *gb = p.want_grad ? p.gbox + row * p.code : nullptr;
        if (label > 0) {
            const float gl = p.g_loc * wr;
            for (int k = 0; k < p.code; ++k) {
                const float pk = bp[k], rk = tg[k];
                float in = pk, t = rk, sp = 0.f, cp = 0.f, sr = 0.f, cr = 0.f;
                if (k == 6) {
                    sp = modest::sin_f32(pk); cp = modest::cos_f32(pk);
                    sr = modest::sin_f32(rk); cr = modest::cos_f32(rk);
                    in = sp * cr;
                    t = cp * sr;
                }
                float g_in, g_t;
                sum_loc = sum_loc + smooth_l1_term(in, t, p.cw[k], gl, p.sl1, g_in, g_t) * wr;
                if (gb) gb[k] = k == 6 ? ((g_in * cr) * cp) + ((g_t * sr) * (-sp)) : g_in;
            }
        } else if (gb) {
            for (int k = 0; k < p.code; ++k) gb[k] = 0.f;
        }
        // ---- direction: cross entropy of the bin of the gt's heading
        if (p.dir) {
            const float *z = p.dir + row * p.bins;
            float *gd = p.want_grad ? p.gdir + row * p.bins : nullptr;
            if (label > 0) {
                const float rot = tg[6] + p.anchors[i * p.a_cols + 6];
                const float val = rot - p.dir_offset;
                const float lim = val - floorf(val / p.two_pi + 0.f) * p.two_pi;   // limit_period(val, 0, 2 pi)
                const float f = floorf(lim / p.bin_width);
                const int bin = !(f >= 0.f) ? 0 : (f >= (float)(p.bins - 1) ? p.bins - 1 : (int)f);
                float m = z[0];
                for (int j = 1; j < p.bins; ++j) m = z[j] > m ? z[j] : m;
                float se = 0.f;
                for (int j = 0; j < p.bins; ++j) se = se + exp_f32(z[j] - m);
                const float lse = log_f32(se);
                sum_dir = (-((z[bin] - m) - lse)) * wr;
                if (gd) {
                    const float g = -(p.g_dir * wr);                       // gradient of the picked log-probability
                    for (int j = 0; j < p.bins; ++j) {
                        const float prob = exp_f32((z[j] - m) - lse);
                        gd[j] = (j == bin ? g : 0.f) - prob * g;
                    }
                }
            } else if (gd) {
                for (int j = 0; j < p.bins; ++j) gd[j] = 0.f;
            }
        }
    }
    workgroup_sums(sum_cls, sum_loc, sum_dir, p.part, (int64_t)p.b * p.blocks, (int64_t)b * p.blocks + blockIdx.x);
}

__global__ __launch_bounds__(LANES) void al_finish(LossParams p) {
    float v[3];
    finish_sums(p.part, (int64_t)p.b * p.blocks, v);
    if (threadIdx.x == 0) {
        const float cls = (v[0] / p.fb) * p.w_cls, loc = (v[1] / p.fb) * p.w_loc;
        const float dir = p.dir ? (v[2] / p.fb) * p.w_dir : 0.f;
        p.out[0] = cls;
        p.out[1] = loc;
        p.out[2] = dir;
        p.out[3] = p.dir ? cls + (loc + dir) : cls + loc;
    }
}

__global__ __launch_bounds__(LANES) void al_scale(int64_t n0, int64_t n1, int64_t n2, float *__restrict__ g0,
                                                 float *__restrict__ g1, float *__restrict__ g2,
                                                 const float *__restrict__ upstream) {
    scale_grads(n0, n1, n2, g0, g1, g2, upstream);
}

size_t ws_total(int b, int64_t n) { return arena_sz(4 * (size_t)(b > 0 ? b : 1)) + arena_sz(4 * 3 * (size_t)b * (size_t)blocks_of(n)); }

}  // namespace

extern "C" int64_t modest_anchor_loss_workspace_bytes(int batch_size, int64_t n_anchors) {
    if (batch_size < 0 || batch_size > AL_MAX_BATCH || n_anchors < 0 || blocks_of(n_anchors) > 2147483647LL) {
        modest_set_error("modest_anchor_loss_workspace_bytes: requirement failed: 0 <= batch_size <= 65535 and 0 <= n_anchors < 2^39");
        return MODEST_ERR_ARG;
    }
    return (int64_t)ws_total(batch_size, n_anchors);
}

extern "C" int modest_anchor_loss(int batch_size, int64_t n_anchors, int num_class, int code, int bins, const float *cls_preds_dev,
                                  const float *box_preds_dev, const float *dir_preds_dev, const void *labels_dev,
                                  int labels_int64, const float *reg_targets_dev, const float *anchors_dev, int anchor_cols,
                                  const float *code_weights_dev, float beta, float dir_offset, float cls_weight,
                                  float loc_weight, float dir_weight, float alpha, float gamma, float *losses_dev,
                                  float *grad_cls_dev, float *grad_box_dev, float *grad_dir_dev, void *workspace_dev,
                                  int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(batch_size >= 1 && batch_size <= AL_MAX_BATCH, "batch_size between 1 and 65535 (the grid's second dimension)");
    MODEST_REQUIRE(n_anchors >= 0 && blocks_of(n_anchors) <= 2147483647LL, "n_anchors between 0 and 2^39 - 256");
    MODEST_REQUIRE(num_class >= 1 && num_class <= AL_MAX_CLASS, "num_class between 1 and 32");
    MODEST_REQUIRE(code >= 7 && code <= AL_MAX_CODE, "code size between 7 and 16");
    MODEST_REQUIRE(dir_preds_dev == nullptr || (bins >= 1 && bins <= AL_MAX_BINS), "NUM_DIR_BINS between 1 and 8");
    MODEST_REQUIRE(anchor_cols >= 7, "anchors (N, >= 7)");
    MODEST_REQUIRE(gamma == 2.0f, "gamma = 2 (the focal power is the product pt * pt)");
    MODEST_REQUIRE(losses_dev && workspace_dev && ((uintptr_t)workspace_dev & 3) == 0, "NULL or unaligned buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)ws_total(batch_size, n_anchors), "workspace smaller than modest_anchor_loss_workspace_bytes");
    const bool want = grad_cls_dev != nullptr;
    MODEST_REQUIRE(want == (grad_box_dev != nullptr) && (!dir_preds_dev || want == (grad_dir_dev != nullptr)),
                   "the gradient buffers come together");
    MODEST_REQUIRE(n_anchors == 0 || (cls_preds_dev && box_preds_dev && labels_dev && reg_targets_dev && anchors_dev && code_weights_dev),
                   "NULL buffer");
    LossParams p;
    p.b = batch_size; p.c = num_class; p.code = code; p.bins = dir_preds_dev ? bins : 0; p.a_cols = anchor_cols;
    p.lab64 = labels_int64 ? 1 : 0;
    p.want_grad = want ? 1 : 0;
    p.n = n_anchors; p.blocks = blocks_of(n_anchors);
    p.cls = cls_preds_dev; p.box = box_preds_dev; p.dir = dir_preds_dev; p.tg = reg_targets_dev; p.anchors = anchors_dev;
    p.cw = code_weights_dev; p.labels = labels_dev;
    p.sl1 = smooth_l1_of(beta);
    p.dir_offset = dir_offset;
    p.two_pi = (float)(2 * 3.14159265358979323846);
    p.bin_width = (float)(2 * 3.14159265358979323846 / (double)(bins > 0 ? bins : 1));
    p.alpha = alpha; p.one_m_alpha = (float)(1.0 - (double)alpha);
    p.fb = (float)batch_size;
    p.w_cls = cls_weight; p.w_loc = loc_weight; p.w_dir = dir_weight;
    p.g_cls = cls_weight / p.fb; p.g_loc = loc_weight / p.fb; p.g_dir = dir_weight / p.fb;
    p.gcls = grad_cls_dev; p.gbox = grad_box_dev; p.gdir = grad_dir_dev; p.out = losses_dev;
    char *ws = static_cast<char *>(workspace_dev);
    p.cnt = reinterpret_cast<int32_t *>(ws);
    p.part = reinterpret_cast<float *>(ws + arena_sz(4 * (size_t)batch_size));
    hipStream_t s = as_stream(stream);
    MODEST_HIP_CHECK(hipMemsetAsync(p.cnt, 0, 4 * (size_t)batch_size, s));
    if (p.blocks > 0) {
        const dim3 grid((unsigned)p.blocks, (unsigned)batch_size);
        al_count<<<grid, LANES, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
        al_loss<<<grid, LANES, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    al_finish<<<1, LANES, 0, s>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_anchor_loss_backward(int64_t n_cls, int64_t n_box, int64_t n_dir, float *grad_cls_dev, float *grad_box_dev,
                                           float *grad_dir_dev, const float *upstream_dev, void *stream) {
    MODEST_REQUIRE(n_cls >= 0 && n_box >= 0 && n_dir >= 0, "negative size");
    const int64_t total = n_cls + n_box + n_dir;
    MODEST_REQUIRE(blocks_of(total) <= 2147483647LL, "at most 2^39 - 256 gradient elements");
    MODEST_REQUIRE((n_cls == 0 || grad_cls_dev) && (n_box == 0 || grad_box_dev) && (n_dir == 0 || grad_dir_dev), "NULL buffer");
    if (total == 0) return MODEST_OK;
    MODEST_REQUIRE(upstream_dev, "NULL upstream gradient");
    al_scale<<<(unsigned)blocks_of(total), LANES, 0, as_stream(stream)>>>(n_cls, n_box, n_dir, grad_cls_dev, grad_box_dev, grad_dir_dev,
                                                                        upstream_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
