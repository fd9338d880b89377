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
//              for every lane; box and direction terms for positive lanes only, zero gradient rows for the others; the three
//              sums of the workgroup through a fixed tree (xor butterfly over the wavefront, (w0 + w1) + (w2 + w3) in LDS)
//              into the partials array;
//   al_finish  one workgroup: lane t adds partials t, t + 256, ... in ascending order, then the same tree, then the four
//              scalars;
//   al_scale   (modest_anchor_loss_backward) the three gradient buffers times the upstream gradient read from the device.
// No float atomics: no result depends on arrival order.  The arithmetic is the contract of DESIGN.md section 7p: float32,
// one rounding per operation in the written order (built with -ffp-contract=off), exp / log / log1p / sin / cos as the double
// function rounded once; the gradient follows autograd's own chain through the reference's expression, path by path.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "trig_f32.h"

namespace {

constexpr int AL_T = 256;          // lanes (anchors) per workgroup
constexpr int AL_WAVES = AL_T / 64;
constexpr int AL_MAX_CLASS = 32, AL_MAX_CODE = 16, AL_MAX_BINS = 8, AL_MAX_BATCH = 65535;

__device__ __forceinline__ float exp_f32(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_f32(float x) { return (float)log((double)x); }
__device__ __forceinline__ float log1p_f32(float x) { return (float)log1p((double)x); }
__device__ __forceinline__ float sigmoid_f32(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
// torch's sgn of a real: (0 < x) - (x < 0), so 0 for a NaN
__device__ __forceinline__ float sign_f32(float x) { return (float)((0.f < x) - (x < 0.f)); }

struct LossParams {
    int b, c, code, bins, a_cols, lab64, l1, want_grad;
    int64_t n, blocks;             // anchors per sample, workgroups per sample
    const float *cls, *box, *dir, *tg, *anchors, *cw;
    const void *labels;
    float beta, half_beta, dir_offset, two_pi, bin_width, alpha, one_m_alpha;
    float g_cls, g_loc, g_dir;     // fl(weight / B): the gradient that reaches the summed terms
    float w_cls, w_loc, w_dir, fb; // the loss weights and float(B)
    float *gcls, *gbox, *gdir, *out;
    int32_t *cnt;                  // (B) positives
    float *part;                   // (3, B * blocks) workgroup sums
};

__device__ __forceinline__ int label_at(const LossParams &p, int64_t row) {
    if (p.lab64) {
        const int64_t v = static_cast<const int64_t *>(p.labels)[row];
        return v > 2147483647LL ? 2147483647 : (v < 0 ? -1 : (int)v);
    }
    return static_cast<const int32_t *>(p.labels)[row];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(AL_T) void al_count(LossParams p) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * AL_T + threadIdx.x;
    const bool pos = i < p.n && label_at(p, (int64_t)b * p.n + i) > 0;
    const unsigned long long mask = __ballot(pos);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(p.cnt + b, __popcll(mask));
}

__global__ __launch_bounds__(AL_T) void al_loss(LossParams p) {
    __shared__ float s_sum[3][AL_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * AL_T + tid;
    float sum_cls = 0.f, sum_loc = 0.f, sum_dir = 0.f;
    if (i < p.n) {
        const int64_t row = (int64_t)b * p.n + i;
        const int label = label_at(p, row);
        const float w = 1.0f / fmaxf((float)p.cnt[b], 1.0f);
        const float wc = label >= 0 ? w : 0.f, wr = label > 0 ? w : 0.f;
        // ---- classification: ((aw * pt^2) * bce) * w
        const float gw = p.g_cls * wc;
        for (int c = 0; c < p.c; ++c) {
            const float x = p.cls[row * p.c + c];
            const float t = (label == c + 1 || (p.c == 1 && label > 0)) ? 1.f : 0.f;
            const float s = sigmoid_f32(x);
            const float aw = t * p.alpha + (1.f - t) * p.one_m_alpha;
            const float oms = 1.f - s;
            const float pt = t * oms + (1.f - t) * s;
            const float fw = aw * (pt * pt);
            const float e = exp_f32(-fabsf(x));
            const float bce = (fmaxf(x, 0.f) - x * t) + log1p_f32(e);
            sum_cls = sum_cls + (fw * bce) * wc;
            if (p.want_grad) {
                const float g_fw = gw * bce, g_bce = gw * fw;
                const float c1 = x >= 0.f ? g_bce : 0.f;                   // clamp(min=0): 1 at +-0
                const float c2 = -(g_bce * t);
                const float c3 = (-((g_bce / (e + 1.f)) * e)) * sign_f32(x);      // log1p, exp, neg, abs (0 at +-0)
                const float g_pt = (g_fw * aw) * (2.f * pt);               // pow(pt, 2)
                const float g_s = t != 0.f ? -g_pt : g_pt;                 // pt = t (1 - s) + (1 - t) s
                const float p1 = (g_s * oms) * s;                          // sigmoid
                p.gcls[row * p.c + c] = ((c1 + c2) + c3) + p1;
            }
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
                const bool replaced = t != t;     // a NaN target is replaced by the input
                if (replaced) t = in;
                const float d = (in - t) * p.cw[k];
                const float nrm = fabsf(d);
                const bool quad = !p.l1 && nrm < p.beta;
                const float v = p.l1 ? nrm : (quad ? ((0.5f * (nrm * nrm)) / p.beta) : (nrm - p.half_beta));
                sum_loc = sum_loc + v * wr;
                if (gb) {
                    // where() hands the branch not taken a zero and pow's backward multiplies it by 2 n: +0 for a finite n (gl + 0 is
                    // gl), a NaN for an infinite or NaN one, as autograd gives it
                    const float dead = ((0.f / p.beta) * 0.5f) * (2.f * nrm);
                    const float g_n = quad ? (((gl / p.beta) * 0.5f) * (2.f * nrm)) : (p.l1 ? gl : gl + dead);
                    const float g_d = (g_n * sign_f32(d)) * p.cw[k];
                    const float g_t = replaced ? 0.f : -g_d;               // where(isnan): no gradient to the replaced target
                    const float g_in = replaced ? g_d + (-g_d) : g_d;      // ... its share goes to the input and cancels
                    gb[k] = k == 6 ? ((g_in * cr) * cp) + ((g_t * sr) * (-sp)) : g_in;
                }
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
    const float a = wave_sum(sum_cls), l = wave_sum(sum_loc), d = wave_sum(sum_dir);
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = a;
        s_sum[1][tid >> 6] = l;
        s_sum[2][tid >> 6] = d;
    }
    __syncthreads();
    if (tid < 3) {
        const int64_t total = (int64_t)p.b * p.blocks;
        p.part[tid * total + (int64_t)b * p.blocks + blockIdx.x] = (s_sum[tid][0] + s_sum[tid][1]) + (s_sum[tid][2] + s_sum[tid][3]);
    }
}

__global__ __launch_bounds__(AL_T) void al_finish(LossParams p) {
    __shared__ float s_sum[3][AL_WAVES];
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)p.b * p.blocks;
    float acc[3] = {0.f, 0.f, 0.f};
    // partials t, t + 256, ... in ascending order; 8 rows of loads are in flight before their additions.  A row past the
    // end adds +0, which changes nothing: an accumulator that starts at +0 is never -0
    for (int64_t j0 = tid; j0 < total; j0 += 8 * AL_T) {
        float v[3][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t j = j0 + k * AL_T;
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q][k] = j < total ? p.part[q * total + j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = acc[q] + v[q][k];
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        acc[q] = wave_sum(acc[q]);
        if ((tid & 63) == 0) s_sum[q][tid >> 6] = acc[q];
    }
    __syncthreads();
    if (tid == 0) {
        float v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] = (s_sum[q][0] + s_sum[q][1]) + (s_sum[q][2] + s_sum[q][3]);
        const float cls = (v[0] / p.fb) * p.w_cls, loc = (v[1] / p.fb) * p.w_loc;
        const float dir = p.dir ? (v[2] / p.fb) * p.w_dir : 0.f;
        p.out[0] = cls;
        p.out[1] = loc;
        p.out[2] = dir;
        p.out[3] = p.dir ? cls + (loc + dir) : cls + loc;
    }
}

__global__ __launch_bounds__(AL_T) void al_scale(int64_t n0, int64_t n1, int64_t n2, float *__restrict__ g0,
                                                float *__restrict__ g1, float *__restrict__ g2,
                                                const float *__restrict__ upstream) {
    const float u = upstream[0];
    const int64_t i = (int64_t)blockIdx.x * AL_T + threadIdx.x;
    if (i < n0) g0[i] = g0[i] * u;
    else if (i < n0 + n1) g1[i - n0] = g1[i - n0] * u;
    else if (i < n0 + n1 + n2) g2[i - n0 - n1] = g2[i - n0 - n1] * u;
}

int64_t blocks_of(int64_t n) { return (n + AL_T - 1) / AL_T; }
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
    p.l1 = (double)beta < 1e-5 ? 1 : 0;
    p.want_grad = want ? 1 : 0;
    p.n = n_anchors; p.blocks = blocks_of(n_anchors);
    p.cls = cls_preds_dev; p.box = box_preds_dev; p.dir = dir_preds_dev; p.tg = reg_targets_dev; p.anchors = anchors_dev;
    p.cw = code_weights_dev; p.labels = labels_dev;
    p.beta = beta; p.half_beta = (float)(0.5 * (double)beta); p.dir_offset = dir_offset;
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
        al_count<<<grid, AL_T, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
        al_loss<<<grid, AL_T, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    al_finish<<<1, AL_T, 0, s>>>(p);
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
    al_scale<<<(unsigned)blocks_of(total), AL_T, 0, as_stream(stream)>>>(n_cls, n_box, n_dir, grad_cls_dev, grad_box_dev, grad_dir_dev,
                                                                        upstream_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
