// Box decoding of OpenPCDet's three kinds of head (generate_predicted_boxes of pcdet/models/dense_heads/anchor_head_template.py,
// point_head_template.py and pcdet/models/roi_heads/roi_head_template.py over ResidualCoder / PointResidualCoder .decode_torch of
// pcdet/utils/box_coder_utils.py, limit_period and rotate_points_along_z of pcdet/utils/common_utils.py), hand-written for
// gfx950.  Three entry points (include/modest_hip.h, "a37"): enqueue only, no synchronise, no context, no device allocation,
// nothing read back, every output element written.
//
// The kernels are streams: each input is read once and the output written once.  A workgroup of 256 lanes owns a tile of 256
// consecutive rows, moves it in and out as consecutive dwords per lane (csrc/box_tile.h) and computes a row per lane out of LDS:
//   bd_anchor  the anchors' tile is loaded ONCE and what a row needs of it is kept in registers while the workgroup walks the
//              samples of the batch (blockIdx.y, += gridDim.y): no (B, N, 7) repeat of the anchors, and no second read of them
//              from another XCD's L2;
//   bd_point   the class logits' tile shares its LDS with the output tile (the argmax is taken before the boxes are written);
//   bd_roi     the residual decode against the centred roi, the rotation about z with its zero terms and the shift, in one.
// The arithmetic (the contract of csrc/loss_terms.h): float32, one rounding per operation in the written
// order (-ffp-contract=off), sqrt and / correctly rounded, exp / sin / cos / atan2 the double function rounded once, x ** 2 as
// x * x.  ARGMAX (both uses): torch's max(dim=-1) on the CPU -- the first index of the maximum, a NaN counts as the maximum and
// the first NaN wins.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "loss_terms.h"
#include "trig_f32.h"
#include "box_tile.h"

namespace {

using modest::loss::exp_f32;
using modest::sin_f32;
using modest::cos_f32;
using modest::atan2_f32;
namespace tile = modest::tile;
using tile::LANES;

constexpr int BD_MAX_CODE = 16, BD_MAX_BINS = 8, BD_MAX_CLASS = 32;
constexpr int64_t BD_MAX_ROWS = 2147483647LL;      // rows are counted in an int; element offsets are int64
constexpr int BD_TARGET_BLOCKS = 1024;             // the batch is split over blockIdx.y until the grid has about this many

// the ARGMAX rule over columns [0, n) of row `row` of a tile of width n
__device__ __forceinline__ int argmax_of(const float *s, int row, int n) {
    int best = 0;
    float bv = s[tile::at(row * n)];
    for (int k = 1; k < n; ++k) {
        const float v = s[tile::at(row * n + k)];
        if (bv == bv && (v > bv || v != v)) { bv = v; best = k; }
    }
    return best;
}

struct AnchorDecodeParams {
    int64_t n;                     // anchors
    int batch, code_in, cols, bins, sincos;      // cols = columns of an anchor = of an output row
    const float *box, *anchors, *dir;
    float dir_offset, dir_limit_offset, period;
    float *out;
};

// four wavefronts a SIMD: the three double exp of a row would otherwise take 133 registers and leave three
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(4))) void bd_anchor(AnchorDecodeParams p) {
    extern __shared__ float lds[];
    float *s_anchor = lds, *s_in = s_anchor + tile::floats_of(p.cols), *s_out = s_in + tile::floats_of(p.code_in),
          *s_dir = s_out + tile::floats_of(p.cols);
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * LANES;
    const int rows = (int)(p.n - row0 < LANES ? p.n - row0 : LANES);
    tile::load(p.anchors + row0 * p.cols, s_anchor, rows * p.cols);
    __syncthreads();
    // what the row needs of its anchor, for every sample
    float xa = 0.f, ya = 0.f, za = 0.f, dxa = 0.f, dya = 0.f, dza = 0.f, ra = 0.f, diag = 0.f, cos_ra = 0.f, sin_ra = 0.f;
    if (t < rows) {
        const float *a = s_anchor;
        const int o = t * p.cols;
        xa = a[tile::at(o)]; ya = a[tile::at(o + 1)]; za = a[tile::at(o + 2)];
        dxa = a[tile::at(o + 3)]; dya = a[tile::at(o + 4)]; dza = a[tile::at(o + 5)]; ra = a[tile::at(o + 6)];
        diag = sqrtf(dxa * dxa + dya * dya);
        if (p.sincos) { cos_ra = cos_f32(ra); sin_ra = sin_f32(ra); }
    }
    const int extra0 = p.sincos ? 8 : 7;         // the first extra column of an encoding
    for (int b = blockIdx.y; b < p.batch; b += gridDim.y) {
        const int64_t first = (int64_t)b * p.n + row0;
        tile::load(p.box + first * p.code_in, s_in, rows * p.code_in);
        if (p.dir) tile::load(p.dir + first * p.bins, s_dir, rows * p.bins);
        __syncthreads();
        if (t < rows) {
            const int i = t * p.code_in, o = t * p.cols;
            const float xt = s_in[tile::at(i)], yt = s_in[tile::at(i + 1)], zt = s_in[tile::at(i + 2)];
            const float dxt = s_in[tile::at(i + 3)], dyt = s_in[tile::at(i + 4)], dzt = s_in[tile::at(i + 5)];
            s_out[tile::at(o)] = xt * diag + xa;
            s_out[tile::at(o + 1)] = yt * diag + ya;
            s_out[tile::at(o + 2)] = zt * dza + za;
            s_out[tile::at(o + 3)] = exp_f32(dxt) * dxa;
            s_out[tile::at(o + 4)] = exp_f32(dyt) * dya;
            s_out[tile::at(o + 5)] = exp_f32(dzt) * dza;
            float rg;
            if (p.sincos) {
                const float rg_cos = s_in[tile::at(i + 6)] + cos_ra, rg_sin = s_in[tile::at(i + 7)] + sin_ra;
                rg = atan2_f32(rg_sin, rg_cos);
            } else {
                rg = s_in[tile::at(i + 6)] + ra;
            }
            if (p.dir) {
                const int label = argmax_of(s_dir, t, p.bins);
                const float v = rg - p.dir_offset;
                const float rot = v - floorf(v / p.period + p.dir_limit_offset) * p.period;
                rg = (rot + p.dir_offset) + p.period * (float)label;
            }
            s_out[tile::at(o + 6)] = rg;
            for (int k = 7; k < p.cols; ++k) s_out[tile::at(o + k)] = s_in[tile::at(i + extra0 + (k - 7))] + s_anchor[tile::at(o + k)];
        }
        __syncthreads();
        tile::store(p.out + first * p.cols, s_out, rows * p.cols);
        // the next sample's loads write s_in and s_dir, which every lane has read before the barrier above; its rows are
        // written to s_out after the next barrier, which this store precedes
    }
}

struct PointDecodeParams {
    int64_t n, point_stride;
    int code_in, cols, classes;
    const float *box, *points, *cls, *mean_size;
    float *out;
};

__global__ __launch_bounds__(LANES) void bd_point(PointDecodeParams p) {
    extern __shared__ float lds[];
    float *s_in = lds, *s_out = s_in + tile::floats_of(p.code_in);      // s_out also holds the class logits first
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * LANES;
    const int rows = (int)(p.n - row0 < LANES ? p.n - row0 : LANES);
    tile::load(p.box + row0 * p.code_in, s_in, rows * p.code_in);
    tile::load(p.cls + row0 * p.classes, s_out, rows * p.classes);
    __syncthreads();
    const int c = t < rows ? argmax_of(s_out, t, p.classes) : 0;
    __syncthreads();                                                    // every argmax is taken: the logits may go
    if (t < rows) {
        const float *pt = p.points + (row0 + t) * p.point_stride;
        const float xa = pt[0], ya = pt[1], za = pt[2];
        const int i = t * p.code_in, o = t * p.cols;
        const float xt = s_in[tile::at(i)], yt = s_in[tile::at(i + 1)], zt = s_in[tile::at(i + 2)];
        const float dxt = s_in[tile::at(i + 3)], dyt = s_in[tile::at(i + 4)], dzt = s_in[tile::at(i + 5)];
        if (p.mean_size) {
            const float dxa = p.mean_size[c * 3], dya = p.mean_size[c * 3 + 1], dza = p.mean_size[c * 3 + 2];
            const float diag = sqrtf(dxa * dxa + dya * dya);
            s_out[tile::at(o)] = xt * diag + xa;
            s_out[tile::at(o + 1)] = yt * diag + ya;
            s_out[tile::at(o + 2)] = zt * dza + za;
            s_out[tile::at(o + 3)] = exp_f32(dxt) * dxa;
            s_out[tile::at(o + 4)] = exp_f32(dyt) * dya;
            s_out[tile::at(o + 5)] = exp_f32(dzt) * dza;
        } else {
            s_out[tile::at(o)] = xt + xa;
            s_out[tile::at(o + 1)] = yt + ya;
            s_out[tile::at(o + 2)] = zt + za;
            s_out[tile::at(o + 3)] = exp_f32(dxt);
            s_out[tile::at(o + 4)] = exp_f32(dyt);
            s_out[tile::at(o + 5)] = exp_f32(dzt);
        }
        s_out[tile::at(o + 6)] = atan2_f32(s_in[tile::at(i + 7)], s_in[tile::at(i + 6)]);      // atan2(sint, cost)
        for (int k = 7; k < p.cols; ++k) s_out[tile::at(o + k)] = s_in[tile::at(i + k + 1)];
    }
    __syncthreads();
    tile::store(p.out + row0 * p.cols, s_out, rows * p.cols);
}

struct RoiDecodeParams {
    int64_t n;
    int code;
    const float *rois, *box;
    float *out;
};

__global__ __launch_bounds__(LANES) void bd_roi(RoiDecodeParams p) {
    extern __shared__ float lds[];
    float *s_roi = lds, *s_in = s_roi + tile::floats_of(p.code), *s_out = s_in + tile::floats_of(p.code);
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * LANES;
    const int rows = (int)(p.n - row0 < LANES ? p.n - row0 : LANES);
    tile::load(p.rois + row0 * p.code, s_roi, rows * p.code);
    tile::load(p.box + row0 * p.code, s_in, rows * p.code);
    __syncthreads();
    if (t < rows) {
        const int o = t * p.code;
        const float rx = s_roi[tile::at(o)], ry = s_roi[tile::at(o + 1)], rz = s_roi[tile::at(o + 2)];
        const float dxa = s_roi[tile::at(o + 3)], dya = s_roi[tile::at(o + 4)], dza = s_roi[tile::at(o + 5)], ra = s_roi[tile::at(o + 6)];
        const float xt = s_in[tile::at(o)], yt = s_in[tile::at(o + 1)], zt = s_in[tile::at(o + 2)];
        const float diag = sqrtf(dxa * dxa + dya * dya);
        // the decode against the roi with its centre at zero
        const float xg = xt * diag + 0.f, yg = yt * diag + 0.f, zg = zt * dza + 0.f;
        // the row vector times [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]], its zero terms kept: an infinite coordinate turns
        // the others into NaN as the reference's matmul does
        const float c = cos_f32(ra), s = sin_f32(ra);
        const float xr = (xg * c + yg * (-s)) + zg * 0.f;
        const float yr = (xg * s + yg * c) + zg * 0.f;
        const float zr = ((xg * 0.f) + (yg * 0.f)) + zg * 1.f;
        s_out[tile::at(o)] = xr + rx;
        s_out[tile::at(o + 1)] = yr + ry;
        s_out[tile::at(o + 2)] = zr + rz;
        s_out[tile::at(o + 3)] = exp_f32(s_in[tile::at(o + 3)]) * dxa;
        s_out[tile::at(o + 4)] = exp_f32(s_in[tile::at(o + 4)]) * dya;
        s_out[tile::at(o + 5)] = exp_f32(s_in[tile::at(o + 5)]) * dza;
        s_out[tile::at(o + 6)] = s_in[tile::at(o + 6)] + ra;
        for (int k = 7; k < p.code; ++k) s_out[tile::at(o + k)] = s_in[tile::at(o + k)] + s_roi[tile::at(o + k)];
    }
    __syncthreads();
    tile::store(p.out + row0 * p.code, s_out, rows * p.code);
}

inline bool aligned4(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }

}  // namespace

extern "C" int64_t modest_box_decode_max_rows(void) { return BD_MAX_ROWS; }

extern "C" int modest_anchor_decode(int batch, int64_t n_anchors, int code_in, int sincos, const float *box_preds_dev,
                                    const float *anchors_dev, const float *dir_cls_preds_dev, int bins, float dir_offset,
                                    float dir_limit_offset, float *boxes_dev, void *stream) {
    MODEST_REQUIRE(batch >= 0 && n_anchors >= 0 && n_anchors <= BD_MAX_ROWS, "batch >= 0 and 0 <= n_anchors <= 2^31 - 1");
    MODEST_REQUIRE(batch == 0 || n_anchors <= BD_MAX_ROWS / batch, "batch * n_anchors at most 2^31 - 1 rows");
    const int lo = sincos ? 8 : 7;
    MODEST_REQUIRE(code_in >= lo && code_in <= BD_MAX_CODE, "code size between 7 (8 with sincos) and 16");
    const bool with_dir = dir_cls_preds_dev != nullptr;
    MODEST_REQUIRE(!with_dir || (bins >= 1 && bins <= BD_MAX_BINS), "bins between 1 and 8");
    if (batch == 0 || n_anchors == 0) return MODEST_OK;
    MODEST_REQUIRE(box_preds_dev && anchors_dev && boxes_dev, "NULL buffer");
    MODEST_REQUIRE(aligned4(box_preds_dev) && aligned4(anchors_dev) && aligned4(dir_cls_preds_dev) && aligned4(boxes_dev),
                   "unaligned buffer");
    AnchorDecodeParams p;
    p.n = n_anchors; p.batch = batch; p.code_in = code_in; p.cols = sincos ? code_in - 1 : code_in;
    p.bins = with_dir ? bins : 0; p.sincos = sincos ? 1 : 0;
    p.box = box_preds_dev; p.anchors = anchors_dev; p.dir = dir_cls_preds_dev;
    p.dir_offset = dir_offset; p.dir_limit_offset = dir_limit_offset;
    p.period = with_dir ? (float)(2.0 * 3.141592653589793 / (double)bins) : 0.f;     // Python's 2 * np.pi / bins, then float32
    p.out = boxes_dev;
    const int64_t tiles = (n_anchors + LANES - 1) / LANES;
    int64_t split = (BD_TARGET_BLOCKS + tiles - 1) / tiles;
    if (split > batch) split = batch;
    if (split > 65535) split = 65535;
    const size_t lds = sizeof(float) * (size_t)(2 * tile::floats_of(p.cols) + tile::floats_of(p.code_in) + tile::floats_of(p.bins));
    bd_anchor<<<dim3((unsigned)tiles, (unsigned)split), LANES, lds, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_point_decode(int64_t n_rows, int code_in, int num_class, const float *box_preds_dev, const float *points_dev,
                                   int64_t point_stride, const float *cls_preds_dev, const float *mean_size_dev, float *boxes_dev,
                                   void *stream) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= BD_MAX_ROWS, "n_rows between 0 and 2^31 - 1");
    MODEST_REQUIRE(code_in >= 8 && code_in <= BD_MAX_CODE, "code size between 8 and 16");
    MODEST_REQUIRE(num_class >= 1 && num_class <= BD_MAX_CLASS, "num_class between 1 and 32");
    MODEST_REQUIRE(point_stride >= 3, "a row stride of the points of at least 3");
    if (n_rows == 0) return MODEST_OK;
    MODEST_REQUIRE(box_preds_dev && points_dev && cls_preds_dev && boxes_dev, "NULL buffer");
    MODEST_REQUIRE(aligned4(box_preds_dev) && aligned4(points_dev) && aligned4(cls_preds_dev) && aligned4(mean_size_dev) &&
                   aligned4(boxes_dev), "unaligned buffer");
    PointDecodeParams p;
    p.n = n_rows; p.point_stride = point_stride; p.code_in = code_in; p.cols = code_in - 1; p.classes = num_class;
    p.box = box_preds_dev; p.points = points_dev; p.cls = cls_preds_dev; p.mean_size = mean_size_dev; p.out = boxes_dev;
    const int shared = num_class > p.cols ? num_class : p.cols;
    const size_t lds = sizeof(float) * (size_t)(tile::floats_of(code_in) + tile::floats_of(shared));
    bd_point<<<(unsigned)((n_rows + LANES - 1) / LANES), LANES, lds, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_roi_decode(int64_t n_rows, int code, const float *rois_dev, const float *box_preds_dev, float *boxes_dev,
                                 void *stream) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= BD_MAX_ROWS, "n_rows between 0 and 2^31 - 1");
    MODEST_REQUIRE(code >= 7 && code <= BD_MAX_CODE, "code size between 7 and 16");
    if (n_rows == 0) return MODEST_OK;
    MODEST_REQUIRE(rois_dev && box_preds_dev && boxes_dev, "NULL buffer");
    MODEST_REQUIRE(aligned4(rois_dev) && aligned4(box_preds_dev) && aligned4(boxes_dev), "unaligned buffer");
    RoiDecodeParams p;
    p.n = n_rows; p.code = code; p.rois = rois_dev; p.box = box_preds_dev; p.out = boxes_dev;
    const size_t lds = sizeof(float) * (size_t)(3 * tile::floats_of(code));
    bd_roi<<<(unsigned)((n_rows + LANES - 1) / LANES), LANES, lds, as_stream(stream)>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
