// The float32 steps boxes_iou3d_gpu (pcdet/ops/iou3d_nms/iou3d_nms_utils.py:57-81) takes on top of the BEV overlap, in the
// reference's operations and order: shared by rt_match (csrc/roi_targets.hip) and post_recall (csrc/post_process.hip), so both
// make the decision on the same bits.  a is the box of boxes_a, bb the box of boxes_b, bev = box_overlap(a, bb, ...) of
// csrc/iou_bev.h.
#pragma once
#include <hip/hip_runtime.h>

// torch.max / torch.min / torch.clamp(min=) of two numbers: a NaN propagates
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }

// what of box a does not change from pair to pair
struct Iou3dSide {
    float top, bot, vol;
};

__device__ __forceinline__ Iou3dSide iou3d_side(const float *a) {
    Iou3dSide s;
    s.top = a[2] + a[5] / 2;
    s.bot = a[2] - a[5] / 2;
    s.vol = a[3] * a[4] * a[5];
    return s;
}

__device__ __forceinline__ float iou3d_from_bev(const Iou3dSide &sa, const float *bb, float bev) {
    const float b_top = bb[2] + bb[5] / 2, b_bot = bb[2] - bb[5] / 2;
    const float d = min_nan(sa.top, b_top) - max_nan(sa.bot, b_bot);
    const float h = d < 0.f ? 0.f : d;           // clamp(min=0): a NaN stays
    const float o3 = bev * h;
    const float vb = bb[3] * bb[4] * bb[5];
    const float u = sa.vol + vb - o3;
    return o3 / (u < 1e-6f ? 1e-6f : u);         // clamp(min=1e-6): a NaN stays
}
