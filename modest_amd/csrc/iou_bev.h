// The rotated-rectangle clipping and the two IoU device functions of the BEV IoU / NMS kernels, shared by iou3d.hip
// (pair kernels, nms_tiles) and proposals.hip (the capped walk): one text, so both make the same decisions.  The
// arithmetic contract is stated at the top of iou3d.hip; include from a translation unit built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "trig_f32.h"

namespace {

constexpr float IOU_EPS = 1e-8f;
constexpr int NMS_TPB = 64;  // one wavefront per block, 64-bit suppression words

struct Pt {
    float x, y;
};

__host__ __device__ __forceinline__ float cross2(const Pt &a, const Pt &b) { return a.x * b.y - a.y * b.x; }

__host__ __device__ __forceinline__ float cross3(const Pt &p1, const Pt &p2, const Pt &p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__host__ __device__ __forceinline__ bool rect_cross(const Pt &p1, const Pt &p2, const Pt &q1, const Pt &q2) {
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// Point-in-rotated-box with the reference's 1e-2 margin; (c,s) = cos/sin(-heading).
__host__ __device__ __forceinline__ bool in_box2d(const float *box, float c, float s, const Pt &p) {
    const float MARGIN = 1e-2f;
    const float cx = box[0], cy = box[1];
    const float rx = (p.x - cx) * c + (p.y - cy) * (-s);
    const float ry = (p.x - cx) * s + (p.y - cy) * c;
    return fabsf(rx) < box[3] / 2 + MARGIN && fabsf(ry) < box[4] / 2 + MARGIN;
}

__host__ __device__ __forceinline__ bool seg_intersection(const Pt &p1, const Pt &p0, const Pt &q1,
                                                 const Pt &q0, Pt &ans) {
    if (!rect_cross(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > IOU_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__host__ __device__ __forceinline__ void rot_center(const Pt &ctr, float c, float s, Pt &p) {
    const float nx = (p.x - ctr.x) * c + (p.y - ctr.y) * (-s) + ctr.x;
    const float ny = (p.x - ctr.x) * s + (p.y - ctr.y) * c + ctr.y;
    p.x = nx;
    p.y = ny;
}

// The clipped polygon (at most 24 vertices) and its polar angles live in LDS, one column per lane
// ([vertex][lane], conflict-free): as indexed per-thread arrays they went to scratch memory, which a
// kernel pays for at dispatch even before the first access.
constexpr int POLY_MAX = 24;
struct PolyLds {
    float x[POLY_MAX][NMS_TPB], y[POLY_MAX][NMS_TPB], ang[POLY_MAX][NMS_TPB];
};

// TIES: the kernels that are handed the host's cosf / sinf must equal the reference's CPU path bit for bit (objs_nms),
// and that path sorts the vertices by glibc's atan2f, which is not correctly rounded and cannot be evaluated here.  Both
// atan2f and atan2_f32 are within 1 ulp of the angle, so they order two vertices alike unless the sorted angles lie
// closer than TIE_REL (8 ulp) of each other: such a pair is reported (unless the two vertices are the same point,
// which any order serves) and its value recomputed on the host (host_iou_bev).  Measured on constructed degenerate
// pairs (the same rectangle in another parametrisation, boxes turned by 1e-7, shared edges): 1 pair in 2 500; none among
// random boxes or identical ones.
constexpr float TIE_REL = 1e-6f;

// ta / tb = (cos h, sin h, cos(-h), sin(-h)) of the two headings
template <bool TIES = false>
__device__ float box_overlap(const float *a, const float *b, const float4 ta, const float4 tb, PolyLds &L, bool *tie = nullptr) {
    const int ln = threadIdx.x & (NMS_TPB - 1);
    const float a_dxh = a[3] / 2, b_dxh = b[3] / 2, a_dyh = a[4] / 2, b_dyh = b[4] / 2;
    const float ax1 = a[0] - a_dxh, ay1 = a[1] - a_dyh, ax2 = a[0] + a_dxh, ay2 = a[1] + a_dyh;
    const float bx1 = b[0] - b_dxh, by1 = b[1] - b_dyh, bx2 = b[0] + b_dxh, by2 = b[1] + b_dyh;
    const Pt ca{a[0], a[1]}, cb{b[0], b[1]};
    Pt A[5] = {{ax1, ay1}, {ax2, ay1}, {ax2, ay2}, {ax1, ay2}, {0, 0}};
    Pt B[5] = {{bx1, by1}, {bx2, by1}, {bx2, by2}, {bx1, by2}, {0, 0}};
    const float a_cos = ta.x, a_sin = ta.y, b_cos = tb.x, b_sin = tb.y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rot_center(ca, a_cos, a_sin, A[k]);
        rot_center(cb, b_cos, b_sin, B[k]);
    }
    A[4] = A[0];
    B[4] = B[0];

    Pt center{0.f, 0.f};
    int cnt = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            Pt x;
            if (seg_intersection(A[i + 1], A[i], B[j + 1], B[j], x)) {
                center.x = center.x + x.x;
                center.y = center.y + x.y;
                L.x[cnt][ln] = x.x;
                L.y[cnt][ln] = x.y;
                ++cnt;
            }
        }
    // the containment tests rotate by the opposite angle: cos(-h), sin(-h)
    const float a_ncos = ta.z, a_nsin = ta.w, b_ncos = tb.z, b_nsin = tb.w;
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(a, a_ncos, a_nsin, B[k])) {
            center.x = center.x + B[k].x;
            center.y = center.y + B[k].y;
            L.x[cnt][ln] = B[k].x;
            L.y[cnt][ln] = B[k].y;
            ++cnt;
        }
        if (in_box2d(b, b_ncos, b_nsin, A[k])) {
            center.x = center.x + A[k].x;
            center.y = center.y + A[k].y;
            L.x[cnt][ln] = A[k].x;
            L.y[cnt][ln] = A[k].y;
            ++cnt;
        }
    }
    center.x /= cnt;
    center.y /= cnt;

    // bubble sort by polar angle around the centroid, descending swaps as in the reference
    for (int i = 0; i < cnt; ++i) L.ang[i][ln] = modest::atan2_f32(L.y[i][ln] - center.y, L.x[i][ln] - center.x);
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i) {
            const float a0 = L.ang[i][ln], a1 = L.ang[i + 1][ln];
            if (a0 > a1) {
                const float tx = L.x[i][ln], ty = L.y[i][ln];
                L.x[i][ln] = L.x[i + 1][ln];
                L.y[i][ln] = L.y[i + 1][ln];
                L.x[i + 1][ln] = tx;
                L.y[i + 1][ln] = ty;
                L.ang[i][ln] = a1;
                L.ang[i + 1][ln] = a0;
            }
        }
    if (TIES) {
        bool t = false;
        for (int k = 0; k + 1 < cnt; ++k) {
            const float a0 = L.ang[k][ln], a1 = L.ang[k + 1][ln];
            if (a1 - a0 <= fmaxf(fabsf(a0), fabsf(a1)) * TIE_REL &&
                (L.x[k][ln] != L.x[k + 1][ln] || L.y[k][ln] != L.y[k + 1][ln]))
                t = true;
        }
        *tie = t;
    }
    float area = 0.f;
    const float x0 = cnt > 0 ? L.x[0][ln] : 0.f, y0 = cnt > 0 ? L.y[0][ln] : 0.f;
    for (int k = 0; k < cnt - 1; ++k) {
        const Pt u{L.x[k][ln] - x0, L.y[k][ln] - y0};
        const Pt v{L.x[k + 1][ln] - x0, L.y[k + 1][ln] - y0};
        area += cross2(u, v);
    }
    return fabsf(area) / 2.0f;
}

// trig of a heading evaluated on the device: float64 evaluation rounded once (trig_f32.h)
__device__ __forceinline__ float4 device_trig(float h) {
    return make_float4(modest::cos_f32(h), modest::sin_f32(h), modest::cos_f32(-h), modest::sin_f32(-h));
}

template <bool TIES = false>
__device__ __forceinline__ float iou_bev(const float *a, const float *b, const float4 ta, const float4 tb, PolyLds &L,
                                         bool *tie = nullptr) {
    const float sa = a[3] * a[4];
    const float sb = b[3] * b[4];
    const float so = box_overlap<TIES>(a, b, ta, tb, L, tie);
    return so / fmaxf(sa + sb - so, IOU_EPS);
}

__device__ __forceinline__ float iou_normal(const float *a, const float *b) {
    // src/iou3d_nms_kernel.cu:314-325 (axis-aligned)
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
    const float inter = w * h;
    const float sa = a[3] * a[4], sb = b[3] * b[4];
    return inter / fmaxf(sa + sb - inter, IOU_EPS);
}

}  // namespace
