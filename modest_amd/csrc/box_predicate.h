// The box-membership predicate of the RoI ops (check_pt_in_box3d of roipoint_pool3d_kernel.cu:22-35 and
// roiaware_pool3d_kernel.cu:23-36), shared by roipool.hip and roiaware_pool.hip.  The contract is DESIGN.md section 7e
// and the header of roipool.hip: float32 differences, products and sums without contraction, cos / sin of -rz as the
// rounded double functions, the three comparisons between a float32 value a and a double bound D decided in float32
// against a per-box threshold, exactly:
//     a > D  <=>  a > down(D),   down(D) = the largest float32 <= D
//     a < D  <=>  a < up(D),     up(D)   = the smallest float32 >= D
#pragma once
#include <hip/hip_runtime.h>

#include "trig_f32.h"

namespace {

// the float32 neighbours of f (finite or infinite, not NaN) towards -inf / +inf
__device__ __forceinline__ float f32_below(float f) {
    const unsigned u = __float_as_uint(f);
    if (f > 0.f) return __uint_as_float(u - 1u);
    if (f == 0.f) return __uint_as_float(0x80000001u);
    return __uint_as_float(u + 1u);
}
__device__ __forceinline__ float f32_above(float f) {
    const unsigned u = __float_as_uint(f);
    if (f > 0.f) return __uint_as_float(u + 1u);
    if (f == 0.f) return __uint_as_float(0x00000001u);
    return __uint_as_float(u - 1u);
}
// down(D) / up(D): round to nearest, then step back if that went past D.  NaN stays NaN (both comparisons are false);
// an infinite D is its own float32; a finite D beyond FLT_MAX rounds to an infinity that compares past D and steps back.
__device__ __forceinline__ float f32_down(double d) {
    const float f = (float)d;
    return (double)f > d ? f32_below(f) : f;
}
__device__ __forceinline__ float f32_up(double d) {
    const float f = (float)d;
    return (double)f < d ? f32_above(f) : f;
}

// what a box contributes to the predicate: nine float32 values
struct BoxTerms {
    float cx, cy, cz, cosa, sina, nsina, tz, tx, ty;
};
__device__ __forceinline__ BoxTerms box_terms(const float *__restrict__ bx) {
    BoxTerms t;
    t.cx = bx[0]; t.cy = bx[1]; t.cz = bx[2];
    const float dx = bx[3], dy = bx[4], dz = bx[5], rz = bx[6];
    t.cosa = modest::cos_f32(-rz);
    t.sina = modest::sin_f32(-rz);
    t.nsina = -t.sina;
    const double margin = (double)1e-5f;
    t.tz = f32_down((double)dz / 2.0);
    t.tx = f32_up((double)dx / 2.0 + margin);
    t.ty = f32_up((double)dy / 2.0 + margin);
    return t;
}
__device__ __forceinline__ bool pt_in_box(float x, float y, float z, float cx, float cy, float cz, float cosa, float sina,
                                          float nsina, float tz, float tx, float ty) {
    const bool zout = fabsf(z - cz) > tz;
    const float sx = x - cx, sy = y - cy;
    const float lx = sx * cosa + sy * nsina;
    const float ly = sx * sina + sy * cosa;
    return !zout && (fabsf(lx) < tx) && (fabsf(ly) < ty);
}

// the same predicate, handing back the local coordinates as well (they are computed whatever the answer)
__device__ __forceinline__ bool pt_in_box_local(float x, float y, float z, float cx, float cy, float cz, float cosa,
                                                float sina, float nsina, float tz, float tx, float ty, float &lx,
                                                float &ly) {
    const bool zout = fabsf(z - cz) > tz;
    const float sx = x - cx, sy = y - cy;
    lx = sx * cosa + sy * nsina;
    ly = sx * sina + sy * cosa;
    return !zout && (fabsf(lx) < tx) && (fabsf(ly) < ty);
}

}  // namespace
