// Loss of OpenPCDet's RoI heads with its gradients (RoIHeadTemplate.get_loss, pcdet/models/roi_heads/roi_head_template.py:133-228,
// over ResidualCoder of pcdet/utils/box_coder_utils.py, WeightedSmoothL1Loss and get_corner_loss_lidar of
// pcdet/utils/loss_utils.py), hand-written for gfx950.  Two entry points (include/modest_hip.h, "a35"): enqueue only, no
// synchronise, no context, no device allocation, nothing read back.
//
// The encoded targets, the foreground subset, the rotation matrices and the three (fg, 8, 3) corner tensors of the reference
// are never formed; a row that is not foreground reads nothing for the box terms and costs them its zero gradient row.  Kernels:
//   rl_loss    one lane per RoI, 256 per workgroup.  Every workgroup first counts the foreground rows (reg_valid_mask > 0) and
//              the valid class rows (label >= 0) of the WHOLE arrays with ballot + popcount into LDS integers (the arrays are R
//              words and live in L2; no count kernel, no atomic), then the lane computes its row's three terms and writes its
//              gradient rows; the three sums of the workgroup into the partials array;
//   rl_finish  one workgroup: the partials' sums, then the table;
//   rl_scale   (modest_roi_loss_backward) the two gradient buffers times the upstream gradient read from the device.
// The arithmetic, the terms and the summation tree are those of csrc/loss_terms.h (DESIGN.md sections 7p and 7q); sin / cos are
// csrc/trig_f32.h's, sqrt is correctly rounded.  The float label load, the encoding and the corner term are this file's own.
// The 8 corners and code columns 0 .. 6 are unrolled: no indexed per-thread array.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "loss_terms.h"
#include "trig_f32.h"

namespace {

using namespace modest::loss;

constexpr int RL_MAX_CODE = 16;
constexpr int64_t RL_MAX_ROWS = 1 << 20;   // every workgroup counts over all rows: R^2 / 256 reads

struct RoiLossParams {
    int64_t r, blocks;
    int code, label_kind, mask64, corner, want_grad;   // label_kind 0 int32, 1 int64, 2 float32
    int64_t gt_stride, src_stride;
    const float *cls, *reg, *gt, *src, *rois, *cw;
    const void *labels, *mask;
    SmoothL1 sl1;
    float w_cls, w_reg, w_corner, tiny, pi, floor100, eps12;
    float *gcls, *greg, *out;
    float *part;                   // (3, blocks) workgroup sums
};

__device__ __forceinline__ bool fg_at(const RoiLossParams &p, int64_t row) {
    return p.mask64 ? static_cast<const int64_t *>(p.mask)[row] > 0 : static_cast<const int32_t *>(p.mask)[row] > 0;
}

// -> the label as float32 (what .float() gives); valid: label >= 0
__device__ __forceinline__ float label_at(const RoiLossParams &p, int64_t row, bool &valid) {
    if (p.label_kind == 1) {
        const int64_t v = static_cast<const int64_t *>(p.labels)[row];
        valid = v >= 0;
        return (float)v;
    }
    if (p.label_kind == 2) {
        const float v = static_cast<const float *>(p.labels)[row];
        valid = v >= 0.f;
        return v;
    }
    const int32_t v = static_cast<const int32_t *>(p.labels)[row];
    valid = v >= 0;
    return (float)v;
}

// column k of ResidualCoder.encode_torch of the canonical gt against the roi with centre and heading zeroed
__device__ __forceinline__ float encode_col(const RoiLossParams &p, int k, const float *g, const float *roi, float diag_c, float dz_c) {
    if (k < 2) return g[k] / diag_c;
    if (k == 2) return g[2] / dz_c;
    if (k < 6) return log_f32(at_least(g[k], p.tiny) / at_least(roi[k], p.tiny));
    if (k == 6) return g[6];
    return g[k] - roi[k];
}

__global__ __launch_bounds__(LANES) void rl_loss(RoiLossParams p) {
    __shared__ int s_cnt[2][WAVES];
    const int tid = threadIdx.x;
    // ---- the two counts over the whole arrays
    int n_fg = 0, n_valid = 0;
    for (int64_t j0 = 0; j0 < p.r; j0 += LANES) {
        const int64_t j = j0 + tid;
        bool valid = false, fg = false;
        if (j < p.r) {
            label_at(p, j, valid);
            fg = fg_at(p, j);
        }
        n_fg += __popcll(__ballot(fg));
        n_valid += __popcll(__ballot(valid));
    }
    if ((tid & 63) == 0) {
        s_cnt[0][tid >> 6] = n_fg;
        s_cnt[1][tid >> 6] = n_valid;
    }
    __syncthreads();
    const int fg_sum = (s_cnt[0][0] + s_cnt[0][1]) + (s_cnt[0][2] + s_cnt[0][3]);
    const int valid_sum = (s_cnt[1][0] + s_cnt[1][1]) + (s_cnt[1][2] + s_cnt[1][3]);

    const int64_t row = (int64_t)blockIdx.x * LANES + tid;
    float sum_cls = 0.f, sum_reg = 0.f, sum_corner = 0.f;
    if (row < p.r) {
        // ---- classification: binary cross entropy of the sigmoid
        bool valid;
        const float t = label_at(p, row, valid);
        if (valid) {
            const float g0 = p.w_cls / fmaxf((float)valid_sum, 1.f);
            sum_cls = bce_term(p.cls[row], t, g0, p.floor100, p.eps12, p.want_grad ? p.gcls + row : nullptr);
        } else if (p.want_grad) {
            p.gcls[row] = 0.f;
        }
        // ---- the box terms, foreground rows only
        float *gr = p.want_grad ? p.greg + row * p.code : nullptr;
        if (fg_at(p, row)) {
            const float *in = p.reg + row * p.code, *roi = p.rois + row * p.code;
            const float *g = p.gt + row * p.gt_stride;
            const float rdx = roi[3], rdy = roi[4], rdz = roi[5];
            float gc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // the corner term's share, constant indices only
            if (p.corner) {
                const float *q = p.src + row * p.src_stride;
                const float rh = roi[6];
                const float diag = sqrtf(rdx * rdx + rdy * rdy);      // the decode does not clamp the roi's sizes
                const float e3 = exp_f32(in[3]), e4 = exp_f32(in[4]), e5 = exp_f32(in[5]);
                const float x0 = in[0] * diag, y0 = in[1] * diag, z0 = in[2] * rdz;
                const float dx = e3 * rdx, dy = e4 * rdy, dz = e5 * rdz;
                const float hp = in[6] + rh;
                const float cr = modest::cos_f32(rh), sr = modest::sin_f32(rh);
                const float cx = (x0 * cr - y0 * sr) + roi[0], cy = (x0 * sr + y0 * cr) + roi[1], cz = z0 + roi[2];
                const float cp = modest::cos_f32(hp), sp = modest::sin_f32(hp);
                const float qx = q[0], qy = q[1], qz = q[2], qdx = q[3], qdy = q[4], qdz = q[5], qh = q[6];
                const float cg = modest::cos_f32(qh), sg = modest::sin_f32(qh);
                const float qf = qh + p.pi;
                const float cf = modest::cos_f32(qf), sf = modest::sin_f32(qf);
                const float g_row = p.w_corner / (float)fg_sum;
                const float g_c = g_row / 8.f;
                float csum = 0.f, gcx = 0.f, gcy = 0.f, gcz = 0.f, gdx = 0.f, gdy = 0.f, gdz = 0.f;
                float G00 = 0.f, G01 = 0.f, G10 = 0.f, G11 = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float ax = (k & 3) < 2 ? 0.5f : -0.5f;
                    const float ay = ((k & 3) == 0 || (k & 3) == 3) ? 0.5f : -0.5f;
                    const float az = k < 4 ? -0.5f : 0.5f;
                    const float lx = dx * ax, ly = dy * ay, lz = dz * az;
                    const float PX = (lx * cp - ly * sp) + cx, PY = (lx * sp + ly * cp) + cy, PZ = lz + cz;
                    const float mx = qdx * ax, my = qdy * ay, mz = qdz * az;
                    const float GX = (mx * cg - my * sg) + qx, GY = (mx * sg + my * cg) + qy, GZ = mz + qz;
                    const float FX = (mx * cf - my * sf) + qx, FY = (mx * sf + my * cf) + qy;
                    const float ax_ = PX - GX, ay_ = PY - GY, az_ = PZ - GZ;
                    const float bx_ = PX - FX, by_ = PY - FY;
                    const float na = sqrtf((ax_ * ax_ + ay_ * ay_) + az_ * az_);
                    const float nb = sqrtf((bx_ * bx_ + by_ * by_) + az_ * az_);
                    const float m = nb < na ? nb : na;
                    const bool quad = m < 1.f;
                    csum = csum + (quad ? 0.5f * (m * m) : m - 0.5f);
                    if (gr) {
                        // the same smooth L1 (beta = 1): where()'s zero for the branch not taken, times 2 m
                        const float dead = 0.f * (2.f * m);
                        const float g_m = (quad ? (g_c * 0.5f) * (2.f * m) : g_c + dead) * sign_f32(m);
                        const float g_h = na == nb ? g_m / 2.f : g_m;          // min of two equal values: half to each side
                        const float ga = na > nb ? 0.f : g_h, gb = na < nb ? 0.f : g_h;
                        // the norm of a zero vector hands on 0
                        const float uax = na == 0.f ? 0.f : ax_ / na, uay = na == 0.f ? 0.f : ay_ / na, uaz = na == 0.f ? 0.f : az_ / na;
                        const float ubx = nb == 0.f ? 0.f : bx_ / nb, uby = nb == 0.f ? 0.f : by_ / nb, ubz = nb == 0.f ? 0.f : az_ / nb;
                        const float gPX = ga * uax + gb * ubx, gPY = ga * uay + gb * uby, gPZ = ga * uaz + gb * ubz;
                        gcx = gcx + gPX; gcy = gcy + gPY; gcz = gcz + gPZ;
                        G00 = G00 + lx * gPX; G11 = G11 + ly * gPY; G01 = G01 + lx * gPY; G10 = G10 + ly * gPX;
                        const float glx = gPX * cp + gPY * sp, gly = gPY * cp - gPX * sp;
                        gdx = gdx + glx * ax; gdy = gdy + gly * ay; gdz = gdz + gPZ * az;
                    }
                }
                sum_corner = csum / 8.f;
                if (gr) {
                    const float g_cos = G00 + G11, g_sin = G01 - G10;
                    const float gx0 = gcx * cr + gcy * sr, gy0 = gcy * cr - gcx * sr;
                    gc[0] = gx0 * diag;
                    gc[1] = gy0 * diag;
                    gc[2] = gcz * rdz;
                    gc[3] = (gdx * rdx) * e3;
                    gc[4] = (gdy * rdy) * e4;
                    gc[5] = (gdz * rdz) * e5;
                    gc[6] = g_sin * cp - g_cos * sp;
                }
            }
            // ---- smooth L1 of the encoding, columns in order
            const float ca = at_least(rdx, p.tiny), cb = at_least(rdy, p.tiny), dz_c = at_least(rdz, p.tiny);
            const float diag_c = sqrtf(ca * ca + cb * cb);
            const float gl = p.w_reg / fmaxf((float)fg_sum, 1.f);
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                float gk, g_t;
                sum_reg = sum_reg + smooth_l1_term(in[k], encode_col(p, k, g, roi, diag_c, dz_c), p.cw[k], gl, p.sl1, gk, g_t);
                if (gr) gr[k] = gk + gc[k];
            }
            for (int k = 7; k < p.code; ++k) {
                float gk, g_t;
                sum_reg = sum_reg + smooth_l1_term(in[k], encode_col(p, k, g, roi, diag_c, dz_c), p.cw[k], gl, p.sl1, gk, g_t);
                if (gr) gr[k] = gk;
            }
        } else if (gr) {
            for (int k = 0; k < p.code; ++k) gr[k] = 0.f;
        }
    }
    workgroup_sums(sum_cls, sum_reg, sum_corner, p.part, p.blocks, blockIdx.x);
    if (blockIdx.x == 0 && tid == 0) {
        p.out[4] = (float)fg_sum;
        p.out[5] = (float)valid_sum;
    }
}

__global__ __launch_bounds__(LANES) void rl_finish(RoiLossParams p) {
    float v[3];
    finish_sums(p.part, p.blocks, v);
    if (threadIdx.x == 0) {
        const float fg = p.blocks > 0 ? p.out[4] : 0.f, valid = p.blocks > 0 ? p.out[5] : 0.f;   // written by rl_loss, earlier on the stream
        const float cls = (v[0] / fmaxf(valid, 1.f)) * p.w_cls;
        const float reg = (v[1] / fmaxf(fg, 1.f)) * p.w_reg;
        const bool with_corner = p.corner && fg > 0.f;
        const float corner = with_corner ? (v[2] / fg) * p.w_corner : 0.f;
        p.out[0] = cls;
        p.out[1] = reg;
        p.out[2] = corner;
        p.out[3] = with_corner ? cls + (reg + corner) : cls + reg;
        p.out[4] = fg;
        p.out[5] = valid;
    }
}

__global__ __launch_bounds__(LANES) void rl_scale(int64_t n0, int64_t n1, float *__restrict__ g0, float *__restrict__ g1,
                                                 const float *__restrict__ upstream) {
    scale_grads(n0, n1, 0, g0, g1, nullptr, upstream);
}

size_t ws_total(int64_t r) { return arena_sz(4 * 3 * (size_t)(blocks_of(r) > 0 ? blocks_of(r) : 1)); }

}  // namespace

extern "C" int64_t modest_roi_loss_max_rows(void) { return RL_MAX_ROWS; }

extern "C" int64_t modest_roi_loss_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows > RL_MAX_ROWS) {
        modest_set_error("modest_roi_loss_workspace_bytes: requirement failed: 0 <= n_rows <= 2^20");
        return MODEST_ERR_ARG;
    }
    return (int64_t)ws_total(n_rows);
}

extern "C" int modest_roi_loss(int64_t n_rows, int code, const float *rcnn_cls_dev, const float *rcnn_reg_dev,
                               const void *cls_labels_dev, int label_kind, const void *reg_valid_mask_dev, int mask_int64,
                               const float *gt_of_rois_dev, int64_t gt_row_stride, const float *gt_of_rois_src_dev,
                               int64_t src_row_stride, const float *rois_dev, const float *code_weights_dev, float beta,
                               float cls_weight, float reg_weight, float corner_weight, int corner, float *table_dev,
                               float *grad_cls_dev, float *grad_reg_dev, void *workspace_dev, int64_t workspace_bytes,
                               void *stream) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= RL_MAX_ROWS, "n_rows between 0 and 2^20 (every workgroup counts over all rows)");
    MODEST_REQUIRE(code >= 7 && code <= RL_MAX_CODE, "code size between 7 and 16");
    MODEST_REQUIRE(label_kind >= 0 && label_kind <= 2, "label_kind 0 (int32), 1 (int64) or 2 (float32)");
    MODEST_REQUIRE(gt_row_stride >= code && src_row_stride >= code, "a row stride of gt_of_rois / gt_of_rois_src below the code size");
    MODEST_REQUIRE(table_dev && workspace_dev && ((uintptr_t)workspace_dev & 3) == 0, "NULL or unaligned buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)ws_total(n_rows), "workspace smaller than modest_roi_loss_workspace_bytes");
    const bool want = grad_cls_dev != nullptr;
    MODEST_REQUIRE(want == (grad_reg_dev != nullptr), "the gradient buffers come together");
    MODEST_REQUIRE(n_rows == 0 || (rcnn_cls_dev && rcnn_reg_dev && cls_labels_dev && reg_valid_mask_dev && gt_of_rois_dev &&
                                   gt_of_rois_src_dev && rois_dev && code_weights_dev), "NULL buffer");
    RoiLossParams p;
    p.r = n_rows; p.blocks = blocks_of(n_rows);
    p.code = code; p.label_kind = label_kind; p.mask64 = mask_int64 ? 1 : 0; p.corner = corner ? 1 : 0;
    p.want_grad = want ? 1 : 0;
    p.gt_stride = gt_row_stride; p.src_stride = src_row_stride;
    p.cls = rcnn_cls_dev; p.reg = rcnn_reg_dev; p.gt = gt_of_rois_dev; p.src = gt_of_rois_src_dev; p.rois = rois_dev;
    p.cw = code_weights_dev; p.labels = cls_labels_dev; p.mask = reg_valid_mask_dev;
    p.sl1 = smooth_l1_of(beta);
    p.w_cls = cls_weight; p.w_reg = reg_weight; p.w_corner = corner_weight;
    p.tiny = (float)1e-5; p.pi = (float)3.14159265358979323846; p.floor100 = -100.f; p.eps12 = (float)1e-12;
    p.gcls = grad_cls_dev; p.greg = grad_reg_dev; p.out = table_dev;
    p.part = static_cast<float *>(workspace_dev);
    hipStream_t s = as_stream(stream);
    if (p.blocks > 0) {
        rl_loss<<<(unsigned)p.blocks, LANES, 0, s>>>(p);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    rl_finish<<<1, LANES, 0, s>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_roi_loss_backward(int64_t n_cls, int64_t n_reg, float *grad_cls_dev, float *grad_reg_dev,
                                        const float *upstream_dev, void *stream) {
    MODEST_REQUIRE(n_cls >= 0 && n_reg >= 0, "negative size");
    MODEST_REQUIRE(n_cls <= RL_MAX_ROWS && n_reg <= RL_MAX_ROWS * RL_MAX_CODE, "more gradient elements than 2^20 rows of 16 columns");
    MODEST_REQUIRE((n_cls == 0 || grad_cls_dev) && (n_reg == 0 || grad_reg_dev), "NULL buffer");
    const int64_t total = n_cls + n_reg;
    if (total == 0) return MODEST_OK;
    MODEST_REQUIRE(upstream_dev, "NULL upstream gradient");
    rl_scale<<<(unsigned)blocks_of(total), LANES, 0, as_stream(stream)>>>(n_cls, n_reg, grad_cls_dev, grad_reg_dev, upstream_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
