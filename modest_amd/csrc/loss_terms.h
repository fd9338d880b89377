// The arithmetic contract of the head losses, stated once for csrc/anchor_loss.hip, csrc/roi_loss.hip
// and csrc/point_loss.hip: float32, one rounding per operation in the written order (built with -ffp-contract=off), exp / log /
// log1p and the sigmoid as the double function rounded once, / correctly rounded, a fixed summation tree, no float atomics.
// The gradient of a term follows autograd's own chain through the reference's expression, path by path.  The kernels keep
// their own target rules, weights and epilogues; tests/anchor_loss_seq.py restates these functions in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace modest {
namespace loss {

constexpr int LANES = 256;         // lanes (rows) per workgroup of every head-loss kernel
constexpr int WAVES = LANES / 64;

inline int64_t blocks_of(int64_t n) { return (n + LANES - 1) / LANES; }

__device__ __forceinline__ float exp_f32(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_f32(float x) { return (float)log((double)x); }
__device__ __forceinline__ float log1p_f32(float x) { return (float)log1p((double)x); }
__device__ __forceinline__ float sigmoid_f32(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
// torch's sgn of a real: (0 < x) - (x < 0), so 0 for a NaN
__device__ __forceinline__ float sign_f32(float x) { return (float)((0.f < x) - (x < 0.f)); }
// torch's clamp(min=lo): a NaN stays a NaN
__device__ __forceinline__ float at_least(float v, float lo) { return v < lo ? lo : v; }

// an int32 or int64 label as an int, saturated: only its sign and its equality with a class index matter
__device__ __forceinline__ int label_i32(const void *labels, int is_int64, int64_t row) {
    if (is_int64) {
        const int64_t v = static_cast<const int64_t *>(labels)[row];
        return v > 2147483647LL ? 2147483647 : (v < 0 ? -1 : (int)v);
    }
    return static_cast<const int32_t *>(labels)[row];
}

// ---- the summation tree: xor butterfly over the wavefront, (w0 + w1) + (w2 + w3) over the workgroup
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// the workgroup's sums of three terms -> dst[q * stride + idx]
__device__ __forceinline__ void workgroup_sums(float a, float b, float c, float *dst, int64_t stride, int64_t idx) {
    __shared__ float s_sum[3][WAVES];
    const int tid = threadIdx.x;
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = a;
        s_sum[1][tid >> 6] = b;
        s_sum[2][tid >> 6] = c;
    }
    __syncthreads();
    if (tid < 3) dst[tid * stride + idx] = (s_sum[tid][0] + s_sum[tid][1]) + (s_sum[tid][2] + s_sum[tid][3]);
}

// one workgroup over part (3, total): lane t adds partials t, t + 256, ... in ascending order, then the same tree -> v, valid
// in lane 0
__device__ __forceinline__ void finish_sums(const float *part, int64_t total, float v[3]) {
    __shared__ float s_sum[3][WAVES];
    const int tid = threadIdx.x;
    float acc[3] = {0.f, 0.f, 0.f};
    // 8 rows of loads are in flight before their additions.  A row past the end adds +0, which changes nothing: an accumulator
    // that starts at +0 is never -0
    for (int64_t j0 = tid; j0 < total; j0 += 8 * LANES) {
        float r[3][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t j = j0 + k * LANES;
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q][k] = j < total ? part[q * total + j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = acc[q] + r[q][k];
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        acc[q] = wave_sum(acc[q]);
        if ((tid & 63) == 0) s_sum[q][tid >> 6] = acc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = (s_sum[q][0] + s_sum[q][1]) + (s_sum[q][2] + s_sum[q][3]);
}

// ---- SigmoidFocalClassificationLoss with gamma = 2: ((aw * pt^2) * bce) * w of logit x against the target t (0 or 1).
// -> the weighted value; with grad, *grad = its gradient for the gradient gw that reaches the unweighted product
__device__ __forceinline__ float focal_term(float x, float t, float alpha, float one_m_alpha, float w, float gw, float *grad) {
    const float s = sigmoid_f32(x);
    const float aw = t * alpha + (1.f - t) * one_m_alpha;
    const float oms = 1.f - s;
    const float pt = t * oms + (1.f - t) * s;
    const float fw = aw * (pt * pt);
    const float e = exp_f32(-fabsf(x));
    const float bce = (fmaxf(x, 0.f) - x * t) + log1p_f32(e);
    if (grad) {
        const float g_fw = gw * bce, g_bce = gw * fw;
        const float c1 = x >= 0.f ? g_bce : 0.f;                   // clamp(min=0): 1 at +-0
        const float c2 = -(g_bce * t);
        const float c3 = (-((g_bce / (e + 1.f)) * e)) * sign_f32(x);      // log1p, exp, neg, abs (0 at +-0)
        const float g_pt = (g_fw * aw) * (2.f * pt);               // pow(pt, 2)
        const float g_s = t != 0.f ? -g_pt : g_pt;                 // pt = t (1 - s) + (1 - t) s
        const float p1 = (g_s * oms) * s;                          // sigmoid
        *grad = ((c1 + c2) + c3) + p1;
    }
    return (fw * bce) * w;
}

// ---- binary_cross_entropy of the sigmoid of logit x against the target t, its logarithms clamped at floor100 = -100.
// -> the value; with grad, *grad = its gradient for the gradient g0 that reaches the value (eps12 = 1e-12)
__device__ __forceinline__ float bce_term(float x, float t, float g0, float floor100, float eps12, float *grad) {
    const float s = sigmoid_f32(x);
    const float la = at_least(log1p_f32(-s), floor100), lb = at_least(log_f32(s), floor100);
    if (grad) {
        const float oms = 1.f - s;
        const float g_s = (g0 * (s - t)) / at_least(oms * s, eps12);
        *grad = (g_s * oms) * s;
    }
    return (t - 1.f) * la - t * lb;
}

// ---- one column of WeightedSmoothL1Loss (WeightedL1Loss with l1) of the code-weighted difference
struct SmoothL1 {
    float beta, half_beta;
    int l1;                        // beta < 1e-5: the plain L1 norm
};
inline SmoothL1 smooth_l1_of(float beta) { return {beta, (float)(0.5 * (double)beta), (double)beta < 1e-5 ? 1 : 0}; }

// -> the unweighted value; g_in and g_tg its gradients to the input and to the target for the gradient gl that reaches the value
__device__ __forceinline__ float smooth_l1_term(float in, float tg, float cw, float gl, const SmoothL1 &k, float &g_in, float &g_tg) {
    const bool replaced = tg != tg;           // a NaN target is replaced by the input
    if (replaced) tg = in;
    const float d = (in - tg) * cw;
    const float nrm = fabsf(d);
    const bool quad = !k.l1 && nrm < k.beta;
    // where() hands the branch not taken a zero and pow's backward multiplies it by 2 n: +0 for a finite n (gl + 0 is
    // gl), a NaN for an infinite or NaN one, as autograd gives it
    const float dead = ((0.f / k.beta) * 0.5f) * (2.f * nrm);
    const float g_n = quad ? (((gl / k.beta) * 0.5f) * (2.f * nrm)) : (k.l1 ? gl : gl + dead);
    const float g_d = (g_n * sign_f32(d)) * cw;
    g_tg = replaced ? 0.f : -g_d;             // where(isnan): no gradient to the replaced target
    g_in = replaced ? g_d + (-g_d) : g_d;     // ... its share goes to the input and cancels
    return k.l1 ? nrm : (quad ? ((0.5f * (nrm * nrm)) / k.beta) : (nrm - k.half_beta));
}

// ---- the *_loss_backward kernels: lane i of the grid scales element i of the three buffers laid end to end
__device__ __forceinline__ void scale_grads(int64_t n0, int64_t n1, int64_t n2, float *__restrict__ g0, float *__restrict__ g1,
                                            float *__restrict__ g2, const float *__restrict__ upstream) {
    const float u = upstream[0];
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i < n0) g0[i] = g0[i] * u;
    else if (i < n0 + n1) g1[i - n0] = g1[i - n0] * u;
    else if (i < n0 + n1 + n2) g2[i - n0 - n1] = g2[i - n0 - n1] * u;
}

}  // namespace loss
}  // namespace modest
