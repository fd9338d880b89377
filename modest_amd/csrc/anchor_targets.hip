// Anchor target assignment of OpenPCDet's anchor heads (AxisAlignedTargetAssigner.assign_targets,
// pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py, with POS_FRACTION < 0, MATCH_HEIGHT and
// NORM_BY_NUM_EXAMPLES off), hand-written for gfx950.  One entry point (include/modest_hip.h, "a27") assigns a whole
// batch, all anchor classes: enqueue only, no synchronise, no context, no device allocation, nothing read back.
//
// The (anchors, gts) IoU matrix is never stored.  Three kernels:
//   select  one wavefront per (sample, anchor class): the sample's kept gt rows (0 .. the last row whose box values do
//           not sum to 0), those of this class compacted in index order into the workspace as nearest-BEV rectangles,
//           their column maxima zeroed;
//   colmax  one lane per anchor: the IoU with every selected gt (rectangles staged in LDS), the column maximum merged
//           with an integer atomicMax on the float's bits, first in LDS, then one global atomic per gt and workgroup.
//           IoUs are >= +0, so the integer order is the float order and the result does not depend on arrival order;
//   assign  one lane per anchor: the same IoUs from the same code, row maximum with the lowest index, "forced" where an
//           IoU equals its gt's non-zero column maximum bit for bit, the label rule, the residual encoding, and every
//           element of the three outputs written at its place in the head's layout.
// The arithmetic is the contract of DESIGN.md section 7i: float32, one rounding per operation in the written order
// (built with -ffp-contract=off), log / cos / sin as the double function rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "trig_f32.h"

namespace {

constexpr int AT_T = 256;      // lanes (anchors) per workgroup
constexpr int AT_TILE = 256;   // gt rectangles staged in LDS at a time
constexpr int AT_HEAD = 8;     // words ahead of the per-(sample, class) arrays; word 0 = number of selected gts
constexpr int AT_ARRAYS = 7;   // row index, class id, x1, y1, x2, y2, column maximum (float bits)

struct Rect {
    float x1, y1, x2, y2;
};

// boxes3d_lidar_to_aligned_bev_boxes: rot = |r - floor(r / pi + 0.5) * pi| with pi as float32, (dx, dy) kept if
// rot < float32(pi / 4), swapped otherwise; corners x -+ d / 2
__device__ __forceinline__ Rect nearest_bev(float x, float y, float dx, float dy, float r) {
    const float pi = (float)3.14159265358979323846, quarter = (float)(3.14159265358979323846 / 4);
    const float turns = floorf(r / pi + 0.5f);
    const float rot = fabsf(r - turns * pi);
    const bool keep = rot < quarter;
    const float hx = (keep ? dx : dy) / 2.f, hy = (keep ? dy : dx) / 2.f;
    return Rect{x - hx, y - hy, x + hx, y + hy};
}
__device__ __forceinline__ float rect_area(const Rect &a) { return (a.x2 - a.x1) * (a.y2 - a.y1); }
// boxes_iou_normal
__device__ __forceinline__ float rect_iou(const Rect &a, float area_a, float bx1, float by1, float bx2, float by2) {
    const float xmin = fmaxf(a.x1, bx1), xmax = fminf(a.x2, bx2);
    const float ymin = fmaxf(a.y1, by1), ymax = fminf(a.y2, by2);
    const float xl = fmaxf(xmax - xmin, 0.f), yl = fmaxf(ymax - ymin, 0.f);
    const float area_b = (bx2 - bx1) * (by2 - by1);
    const float inter = xl * yl;
    return inter / fmaxf((area_a + area_b) - inter, 1e-6f);
}

struct Params {
    int b, m, gt_cols;             // gt (b, m, gt_cols), the class id in the last column
    int64_t gs_b, gs_m, gs_c;      // its strides in elements
    int a_cols, n_cls, n_names;
    int sincos, extra, code;       // code = 7 + sincos + extra columns, extra = min(a_cols - 7, gt_cols - 8)
    int64_t n_out;                 // anchors per sample, all classes
    const float *gt, *anchors;
    const int64_t *cls;            // (n_cls, 5) first row, rows, k, stride, offset: row i goes to (i / k) * stride + offset + i % k
    const float *thr;              // (n_cls, 2) matched, unmatched
    const uint8_t *match;          // (n_cls, n_names)
    uint32_t *ws;
};

__device__ __forceinline__ uint32_t *ws_of(const Params &p, int b, int c) {
    return p.ws + ((int64_t)b * p.n_cls + c) * (AT_HEAD + (int64_t)AT_ARRAYS * p.m);
}

__global__ __launch_bounds__(64) void at_select(Params p) {
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float *gt = p.gt + b * p.gs_b;
    uint32_t *w = ws_of(p, b, c);
    const int box_cols = p.gt_cols - 1;
    int last = 0;   // row 0 is always kept
    for (int j0 = 0; j0 < p.m; j0 += 64) {
        const int j = j0 + lane;
        bool live = false;
        if (j < p.m) {
            float s = 0.f;
            for (int k = 0; k < box_cols; ++k) s += gt[j * p.gs_m + k * p.gs_c];
            live = !(s == 0.f);
        }
        const unsigned long long mask = __ballot(live);
        if (mask) last = j0 + 63 - __clzll((long long)mask);
    }
    const int kept = p.m > 0 ? last + 1 : 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n_sel = 0;
    for (int j0 = 0; j0 < kept; j0 += 64) {
        const int j = j0 + lane;
        bool mine = false;
        int cid = 0;
        if (j < kept) {
            cid = (int)gt[j * p.gs_m + (int64_t)box_cols * p.gs_c];
            int name = cid - 1;
            if (name < 0) name += p.n_names;   // Python's wrap: id 0 names the last class
            mine = name >= 0 && name < p.n_names && p.match[c * p.n_names + name] != 0;
        }
        const unsigned long long mask = __ballot(mine);
        if (mine) {
            const int at = n_sel + __popcll(mask & below);
            const float *g = gt + j * p.gs_m;
            const Rect r = nearest_bev(g[0], g[p.gs_c], g[3 * p.gs_c], g[4 * p.gs_c], g[6 * p.gs_c]);
            uint32_t *a = w + AT_HEAD + at;
            a[0] = (uint32_t)j;
            a[1 * (int64_t)p.m] = (uint32_t)cid;
            a[2 * (int64_t)p.m] = __float_as_uint(r.x1);
            a[3 * (int64_t)p.m] = __float_as_uint(r.y1);
            a[4 * (int64_t)p.m] = __float_as_uint(r.x2);
            a[5 * (int64_t)p.m] = __float_as_uint(r.y2);
            a[6 * (int64_t)p.m] = 0u;
        }
        n_sel += __popcll(mask);
    }
    if (lane == 0) w[0] = (uint32_t)n_sel;
}

// the lane's anchor: row `row` of the class's block, or none
struct Lane {
    bool ok;
    int64_t row;      // in the anchors buffer
    int64_t out;      // row of the outputs within the sample
};
__device__ __forceinline__ Lane lane_of(const Params &p, int c) {
    const int64_t *t = p.cls + c * 5;
    const int64_t i = (int64_t)blockIdx.x * AT_T + threadIdx.x;
    Lane l;
    l.ok = i < t[1];
    l.row = t[0] + (l.ok ? i : 0);
    l.out = (i / t[2]) * t[3] + t[4] + i % t[2];
    return l;
}

__global__ __launch_bounds__(AT_T) void at_colmax(Params p) {
    __shared__ float s_rect[4][AT_TILE];
    __shared__ uint32_t s_col[AT_TILE];
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if ((int64_t)blockIdx.x * AT_T >= p.cls[c * 5 + 1]) return;
    uint32_t *w = ws_of(p, b, c);
    const int n_sel = (int)w[0];
    if (n_sel == 0) return;
    const Lane l = lane_of(p, c);
    const float *a = p.anchors + l.row * p.a_cols;
    const Rect ra = nearest_bev(a[0], a[1], a[3], a[4], a[6]);
    const float area_a = rect_area(ra);
    for (int j0 = 0; j0 < n_sel; j0 += AT_TILE) {
        const int cnt = min(AT_TILE, n_sel - j0);
        if (tid < cnt) {
            const uint32_t *g = w + AT_HEAD + j0 + tid;
#pragma unroll
            for (int k = 0; k < 4; ++k) s_rect[k][tid] = __uint_as_float(g[(2 + k) * (int64_t)p.m]);
            s_col[tid] = 0u;
        }
        __syncthreads();
        if (l.ok) {
            for (int j = 0; j < cnt; ++j) {
                const float iou = rect_iou(ra, area_a, s_rect[0][j], s_rect[1][j], s_rect[2][j], s_rect[3][j]);
                const uint32_t bits = __float_as_uint(iou);
                if (iou > 0.f && bits > s_col[j]) atomicMax(&s_col[j], bits);
            }
        }
        __syncthreads();
        if (tid < cnt && s_col[tid] != 0u) atomicMax(w + AT_HEAD + 6 * (int64_t)p.m + j0 + tid, s_col[tid]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(AT_T) void at_assign(Params p, int32_t *__restrict__ labels, float *__restrict__ targets,
                                                 float *__restrict__ weights) {
    __shared__ float s_rect[4][AT_TILE];
    __shared__ uint32_t s_col[AT_TILE];
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if ((int64_t)blockIdx.x * AT_T >= p.cls[c * 5 + 1]) return;
    const uint32_t *w = ws_of(p, b, c);
    const int n_sel = (int)w[0];
    const Lane l = lane_of(p, c);
    const float *a = p.anchors + l.row * p.a_cols;
    const Rect ra = nearest_bev(a[0], a[1], a[3], a[4], a[6]);
    const float area_a = rect_area(ra);
    float best = -1.f;
    int arg = 0;
    bool forced = false;
    for (int j0 = 0; j0 < n_sel; j0 += AT_TILE) {
        const int cnt = min(AT_TILE, n_sel - j0);
        __syncthreads();   // the previous tile has been read
        if (tid < cnt) {
            const uint32_t *g = w + AT_HEAD + j0 + tid;
#pragma unroll
            for (int k = 0; k < 4; ++k) s_rect[k][tid] = __uint_as_float(g[(2 + k) * (int64_t)p.m]);
            s_col[tid] = g[6 * (int64_t)p.m];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float iou = rect_iou(ra, area_a, s_rect[0][j], s_rect[1][j], s_rect[2][j], s_rect[3][j]);
            if (iou > best) { best = iou; arg = j0 + j; }                       // strict: the lowest index keeps a tie
            forced |= s_col[j] != 0u && __float_as_uint(iou) == s_col[j];       // a column maximum of 0 forces nothing
        }
    }
    if (!l.ok) return;
    int label = 0;
    if (n_sel > 0) {
        const int cid = (int)w[AT_HEAD + 1 * (int64_t)p.m + arg];
        label = -1;
        if (best >= p.thr[c * 2 + 0]) label = cid;
        if (best < p.thr[c * 2 + 1]) label = 0;
        if (forced) label = cid;
    }
    const int64_t o = (int64_t)b * p.n_out + l.out;
    labels[o] = label;
    weights[o] = label > 0 ? 1.f : 0.f;
    float *t = targets + o * p.code;
    if (label <= 0) {
        for (int k = 0; k < p.code; ++k) t[k] = 0.f;
        return;
    }
    // ResidualCoder.encode_torch of gt row `arg` against the anchor
    const int64_t sc = p.gs_c;
    const float *g = p.gt + b * p.gs_b + (int64_t)w[AT_HEAD + arg] * p.gs_m;
    const float tiny = 1e-5f;
    const float dxa = fmaxf(a[3], tiny), dya = fmaxf(a[4], tiny), dza = fmaxf(a[5], tiny);
    const float dxg = fmaxf(g[3 * sc], tiny), dyg = fmaxf(g[4 * sc], tiny), dzg = fmaxf(g[5 * sc], tiny);
    const float diag = sqrtf(dxa * dxa + dya * dya);
    t[0] = (g[0] - a[0]) / diag;
    t[1] = (g[sc] - a[1]) / diag;
    t[2] = (g[2 * sc] - a[2]) / dza;
    t[3] = (float)log((double)(dxg / dxa));
    t[4] = (float)log((double)(dyg / dya));
    t[5] = (float)log((double)(dzg / dza));
    const float rg = g[6 * sc], rb = a[6];
    int k = 6;
    if (p.sincos) {
        t[k++] = modest::cos_f32(rg) - modest::cos_f32(rb);
        t[k++] = modest::sin_f32(rg) - modest::sin_f32(rb);
    } else {
        t[k++] = rg - rb;
    }
    for (int e = 7; e < 7 + p.extra; ++e) t[k++] = g[e * sc] - a[e];
}

}  // namespace

extern "C" int64_t modest_anchor_targets_workspace_bytes(int b, int n_cls, int m) {
    if (b < 0 || n_cls < 0 || m < 0) {
        modest_set_error("modest_anchor_targets_workspace_bytes: negative size");
        return MODEST_ERR_ARG;
    }
    return (int64_t)b * n_cls * (AT_HEAD + (int64_t)AT_ARRAYS * m) * 4;
}

extern "C" int modest_anchor_targets(int b, int m, int gt_cols, const float *gt_dev, int64_t gt_stride_b,
                                     int64_t gt_stride_m, int64_t gt_stride_c, const float *anchors_dev, int a_cols,
                                     int n_cls, const int64_t *cls_dev, const float *thr_dev, const uint8_t *match_dev,
                                     int n_names, int64_t max_cls_rows, int sincos, int64_t n_out, int32_t *labels_dev,
                                     float *targets_dev, float *weights_dev, void *workspace_dev, int64_t workspace_bytes,
                                     void *stream) {
    MODEST_REQUIRE(b >= 0 && m >= 0 && n_cls >= 0 && n_names >= 0 && max_cls_rows >= 0 && n_out >= 0, "negative size");
    MODEST_REQUIRE(a_cols >= 7 && gt_cols >= 8, "anchors (N, 7 + Ca) and gt (B, M, 7 + Cg + 1)");
    MODEST_REQUIRE(b <= 65535 && n_cls <= 65535, "grid too large");
    if (b == 0 || n_cls == 0 || max_cls_rows == 0) return MODEST_OK;
    const int64_t blocks = (max_cls_rows + AT_T - 1) / AT_T;
    MODEST_REQUIRE(blocks <= 2147483647, "grid too large");
    MODEST_REQUIRE(anchors_dev && cls_dev && thr_dev && labels_dev && targets_dev && weights_dev, "NULL buffer");
    MODEST_REQUIRE((m == 0 || gt_dev) && (n_names == 0 || match_dev), "NULL buffer");
    MODEST_REQUIRE(workspace_dev && (reinterpret_cast<uintptr_t>(workspace_dev) & 3) == 0, "workspace NULL or unaligned");
    MODEST_REQUIRE(workspace_bytes >= modest_anchor_targets_workspace_bytes(b, n_cls, m), "workspace too small");
    Params p;
    p.b = b; p.m = m; p.gt_cols = gt_cols;
    p.gs_b = gt_stride_b; p.gs_m = gt_stride_m; p.gs_c = gt_stride_c;
    p.a_cols = a_cols; p.n_cls = n_cls; p.n_names = n_names;
    p.sincos = sincos ? 1 : 0;
    p.extra = (a_cols - 7 < gt_cols - 8) ? a_cols - 7 : gt_cols - 8;
    p.code = 7 + p.sincos + p.extra;
    p.n_out = n_out;
    p.gt = gt_dev; p.anchors = anchors_dev; p.cls = cls_dev; p.thr = thr_dev; p.match = match_dev;
    p.ws = static_cast<uint32_t *>(workspace_dev);
    hipStream_t s = as_stream(stream);
    at_select<<<dim3((unsigned)n_cls, (unsigned)b), 64, 0, s>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    const dim3 grid((unsigned)blocks, (unsigned)n_cls, (unsigned)b);
    at_colmax<<<grid, AT_T, 0, s>>>(p);
    MODEST_HIP_CHECK(hipGetLastError());
    at_assign<<<grid, AT_T, 0, s>>>(p, labels_dev, targets_dev, weights_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
