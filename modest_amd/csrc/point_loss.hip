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
//              for positive lanes only, zero gradient rows for the others; the three sums of the workgroup through the fixed
//              tree of section 7p (xor butterfly over the wavefront, (w0 + w1) + (w2 + w3) in LDS) into the partials array;
//   pl_finish  one workgroup: lane t adds partials t, t + 256, ... in ascending order, then the same tree, then the table;
//   pl_scale   (modest_point_loss_backward) the three gradient buffers times the upstream gradient read from the device.
// No float atomics: no result depends on arrival order.  The arithmetic is the contract of DESIGN.md section 7r (7p's): float32,
// one rounding per operation in the written order (built with -ffp-contract=off), exp / log / log1p and the sigmoid as the
// double function rounded once, / correctly rounded; the gradient follows autograd's own chain through the reference's
// expression, path by path.  Nothing is indexed by an input value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"

namespace {

constexpr int PL_T = 256;          // lanes (points) per workgroup
constexpr int PL_WAVES = PL_T / 64;
constexpr int PL_MAX_CLASS = 32, PL_MAX_CODE = 16, PL_PART = 3;
constexpr int PL_COUNT_ROWS = 16;  // rows a lane of pl_count looks at
constexpr int64_t PL_MAX_ROWS = 1 << 24;   // the count of positives stays exact as a float32

__device__ __forceinline__ float exp_f32(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_f32(float x) { return (float)log((double)x); }
__device__ __forceinline__ float log1p_f32(float x) { return (float)log1p((double)x); }
__device__ __forceinline__ float sigmoid_f32(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
// torch's sgn of a real: (0 < x) - (x < 0), so 0 for a NaN
__device__ __forceinline__ float sign_f32(float x) { return (float)((0.f < x) - (x < 0.f)); }
// torch's clamp(min=lo): a NaN stays a NaN
__device__ __forceinline__ float at_least(float v, float lo) { return v < lo ? lo : v; }

struct PointLossParams {
    int64_t n, blocks;
    int c, code, lab64, l1, want_grad;
    const float *cls, *part, *part_t, *box, *box_t, *cw;
    const void *labels;
    float beta, half_beta, alpha, one_m_alpha, floor100, eps12;
    float w_cls, w_part, w_box;    // the loss weights: also the gradients that reach the summed cls and box terms
    float *gcls, *gpart, *gbox, *out;
    int32_t *cnt;                  // (1) positives of the whole batch
    float *sums;                   // (3, blocks) workgroup sums
};

__device__ __forceinline__ int label_at(const PointLossParams &p, int64_t row) {
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

// 16 rows a lane, a workgroup over 4096 consecutive rows: the one atomic of a wavefront then stands for 1024 rows, and the
// single counter sees N / 1024 additions (one per 64 rows took longer than pl_loss itself at N = 65 536)
__global__ __launch_bounds__(PL_T) void pl_count(PointLossParams p) {
    const int64_t base = (int64_t)blockIdx.x * (PL_T * PL_COUNT_ROWS) + threadIdx.x;
    int n_pos = 0;
#pragma unroll 4
    for (int k = 0; k < PL_COUNT_ROWS; ++k) {
        const int64_t i = base + (int64_t)k * PL_T;
        const bool pos = i < p.n && label_at(p, i) > 0;
        n_pos += __popcll(__ballot(pos));
    }
    if ((threadIdx.x & 63) == 0 && n_pos) atomicAdd(p.cnt, n_pos);
}

__global__ __launch_bounds__(PL_T) void pl_loss(PointLossParams p) {
    __shared__ float s_sum[3][PL_WAVES];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * PL_T + tid;
    float sum_cls = 0.f, sum_part = 0.f, sum_box = 0.f;
    if (row < p.n) {
        const int label = label_at(p, row);
        const int n_pos = p.cnt[0] > 1 ? p.cnt[0] : 1;
        const float w = 1.0f / (float)n_pos;
        const float wc = label >= 0 ? w : 0.f, wr = label > 0 ? w : 0.f;
        // ---- classification: ((aw * pt^2) * bce) * w, the target strictly label == c + 1
        const float gw = p.w_cls * wc;
        for (int c = 0; c < p.c; ++c) {
            const float x = p.cls[row * p.c + c];
            const float t = label == c + 1 ? 1.f : 0.f;
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
        // ---- part: binary cross entropy of the sigmoid, positive rows only
        if (p.part) {
            float *gp = p.want_grad ? p.gpart + row * PL_PART : nullptr;
            if (label > 0) {
                const float *xp = p.part + row * PL_PART, *tp = p.part_t + row * PL_PART;
                const float g0 = p.w_part / (float)(3 * n_pos);
#pragma unroll
                for (int k = 0; k < PL_PART; ++k) {
                    const float x = xp[k], t = tp[k];
                    const float s = sigmoid_f32(x);
                    const float la = at_least(log1p_f32(-s), p.floor100), lb = at_least(log_f32(s), p.floor100);
                    sum_part = sum_part + ((t - 1.f) * la - t * lb);
                    if (gp) {
                        const float oms = 1.f - s;
                        const float g_s = (g0 * (s - t)) / at_least(oms * s, p.eps12);
                        gp[k] = (g_s * oms) * s;
                    }
                }
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
                    const float in = bp[k];
                    float t = tg[k];
                    const bool replaced = t != t;     // a NaN target is replaced by the input
                    if (replaced) t = in;
                    const float cw = p.cw[k];
                    const float d = (in - t) * cw;
                    const float nrm = fabsf(d);
                    const bool quad = !p.l1 && nrm < p.beta;
                    const float v = p.l1 ? nrm : (quad ? ((0.5f * (nrm * nrm)) / p.beta) : (nrm - p.half_beta));
                    sum_box = sum_box + v * wr;
                    if (gb) {
                        // where() hands the branch not taken a zero and pow's backward multiplies it by 2 n: +0 for a finite n (gl + 0 is
                        // gl), a NaN for an infinite or NaN one, as autograd gives it
                        const float dead = ((0.f / p.beta) * 0.5f) * (2.f * nrm);
                        const float g_n = quad ? (((gl / p.beta) * 0.5f) * (2.f * nrm)) : (p.l1 ? gl : gl + dead);
                        const float g_d = (g_n * sign_f32(d)) * cw;
                        gb[k] = replaced ? g_d + (-g_d) : g_d;             // where(isnan): the target's share goes to the input and cancels
                    }
                }
            } else if (gb) {
                for (int k = 0; k < p.code; ++k) gb[k] = 0.f;
            }
        }
    }
    const float a = wave_sum(sum_cls), b = wave_sum(sum_part), c = wave_sum(sum_box);
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = a;
        s_sum[1][tid >> 6] = b;
        s_sum[2][tid >> 6] = c;
    }
    __syncthreads();
    if (tid < 3) p.sums[tid * p.blocks + blockIdx.x] = (s_sum[tid][0] + s_sum[tid][1]) + (s_sum[tid][2] + s_sum[tid][3]);
}

__global__ __launch_bounds__(PL_T) void pl_finish(PointLossParams p) {
    __shared__ float s_sum[3][PL_WAVES];
    const int tid = threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    // partials t, t + 256, ... in ascending order; an accumulator that starts at +0 is never -0
    for (int64_t j = tid; j < p.blocks; j += PL_T) {
        a0 = a0 + p.sums[j];
        a1 = a1 + p.sums[p.blocks + j];
        a2 = a2 + p.sums[2 * p.blocks + j];
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = a0;
        s_sum[1][tid >> 6] = a1;
        s_sum[2][tid >> 6] = a2;
    }
    __syncthreads();
    if (tid == 0) {
        const float v0 = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
        const float v1 = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
        const float v2 = (s_sum[2][0] + s_sum[2][1]) + (s_sum[2][2] + s_sum[2][3]);
        const int n_pos = p.cnt[0];
        const float cls = v0 * p.w_cls;
        const float part = p.part ? (v1 / (float)(3 * (n_pos > 1 ? n_pos : 1))) * p.w_part : 0.f;
        const float box = p.box ? v2 * p.w_box : 0.f;
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

__global__ __launch_bounds__(PL_T) void pl_scale(int64_t n0, int64_t n1, int64_t n2, float *__restrict__ g0,
                                                float *__restrict__ g1, float *__restrict__ g2,
                                                const float *__restrict__ upstream) {
    const float u = upstream[0];
    const int64_t i = (int64_t)blockIdx.x * PL_T + threadIdx.x;
    if (i < n0) g0[i] = g0[i] * u;
    else if (i < n0 + n1) g1[i - n0] = g1[i - n0] * u;
    else if (i < n0 + n1 + n2) g2[i - n0 - n1] = g2[i - n0 - n1] * u;
}

int64_t blocks_of(int64_t n) { return (n + PL_T - 1) / PL_T; }
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
    p.l1 = (double)beta < 1e-5 ? 1 : 0;
    p.want_grad = want ? 1 : 0;
    p.cls = cls_preds_dev; p.part = part_preds_dev; p.part_t = part_labels_dev; p.box = box_preds_dev; p.box_t = box_labels_dev;
    p.cw = code_weights_dev; p.labels = labels_dev;
    p.beta = beta; p.half_beta = (float)(0.5 * (double)beta);
    p.alpha = 0.25f; p.one_m_alpha = 0.75f; p.floor100 = -100.f; p.eps12 = (float)1e-12;
    p.w_cls = cls_weight; p.w_part = part_weight; p.w_box = box_weight;
    p.gcls = grad_cls_dev; p.gpart = grad_part_dev; p.gbox = grad_box_dev; p.out = table_dev;
    char *ws = static_cast<char *>(workspace_dev);
    p.cnt = reinterpret_cast<int32_t *>(ws);
    p.sums = reinterpret_cast<float *>(ws + ws_counter());
    hipStream_t s = as_stream(stream);
    MODEST_HIP_CHECK(hipMemsetAsync(p.cnt, 0, 4, s));
    if (p.blocks > 0) {
        pl_count<<<(unsigned)((n_rows + PL_T * PL_COUNT_ROWS - 1) / (PL_T * PL_COUNT_ROWS)), PL_T, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
        pl_loss<<<(unsigned)p.blocks, PL_T, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    pl_finish<<<1, PL_T, 0, s>>>(p);
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
    pl_scale<<<(unsigned)blocks_of(total), PL_T, 0, as_stream(stream)>>>(n_cls, n_part, n_box, grad_cls_dev, grad_part_dev, grad_box_dev,
                                                                        upstream_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
