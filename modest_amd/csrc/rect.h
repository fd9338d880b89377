// project_velo_to_rect (utils/kitti_util.py:327-329) for one point, shared by transform.hip and ground_planes.hip:
// rect = (R0 @ ([p,1] @ V2C^T)^T)^T in float64.  numpy hands both products to dgemm, whose k loop is one fused
// multiply-add chain per output element (first product rounded, then fma per further term; the appended 1 makes the
// last term of the first product an exact addend).  The rounding of this chain is the bit-exact contract of
// modest_project_velo_to_rect; every caller goes through this function.
#pragma once
#include <hip/hip_runtime.h>

namespace modest {

struct RectMats {
    double v[12];   // V2C, row major 3x4
    double r[9];    // R0, row major 3x3
};

__device__ __forceinline__ void velo_to_rect(double x, double y, double z, const RectMats &M, double *out) {
    double ref[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double acc = __dmul_rn(x, M.v[4 * j]);
        acc = fma(y, M.v[4 * j + 1], acc);
        acc = fma(z, M.v[4 * j + 2], acc);
        ref[j] = fma(1.0, M.v[4 * j + 3], acc);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double acc = __dmul_rn(M.r[3 * j], ref[0]);
        acc = fma(M.r[3 * j + 1], ref[1], acc);
        out[j] = fma(M.r[3 * j + 2], ref[2], acc);
    }
}

}  // namespace modest
