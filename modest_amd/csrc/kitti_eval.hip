// KITTI-style AP evaluation (OpenPCDet's kitti_object_eval_python/eval.py) for gfx950.
//
// Every frame holds a dt x gt block of overlaps, laid out dt-major (overlaps[j, i] of eval.py) at the frame's pair
// offset.  One evaluation of one metric runs, for every configuration (class, difficulty or range bucket, min overlap):
//   ke_overlaps    one lane per (dt, gt) pair: the float32 rotated-rectangle intersection of rotate_iou.py mirrored
//                  operation by operation (numba's float64 promotions included), giving the BEV value (criterion
//                  crit_bev) and the camera-height 3-D value of d3_box_overlap_kernel (float64, rounded to float32 as
//                  eval.py stores it); optionally the float64 image-box overlap (image_box_overlap).  The polygon and
//                  its sort keys sit in LDS: 24 vertices per lane (4 + 4 corners, 16 edge crossings), so coincident and
//                  nested boxes cannot overflow the buffer (the reference's 8-vertex buffer does).
//   ke_match<A>    compute_statistics_jit, sequential per lane exactly as eval.py:160-278.  Pass A (compute_fp=False):
//                  one wavefront per frame, one lane per configuration, TP scores out.  Pass B (compute_fp=True): one
//                  wavefront per (frame, configuration), one lane per score threshold; tp/fp/fn and the aos similarity
//                  per (configuration, threshold, frame) as partials (no float atomics).  assigned_detection is a per-lane
//                  bitmap in LDS.
//   ke_thresholds  get_thresholds (eval.py:10-28) on the descending TP scores: the selected ranks depend only on the TP
//                  count and the valid-gt count, so each is found by bisection over the monotone skip test.
//   ke_reduce      integer sums over frames, the similarity summed in frame order (fused_compute_statistics' order).
#include "common.h"
#include <cmath>

namespace {

constexpr int KE_OV_THREADS = 64;
constexpr int KE_POLY = 24;          // vertices per lane
constexpr int KE_TMAX = 64;          // thresholds per configuration (eval.py keeps at most 41)
constexpr int KE_MAX_WORDS = 256;    // assigned_detection bitmap words per lane: 8192 detections per frame
constexpr double KE_NO_DETECTION = -10000000.0;

// ---------------------------------------------------------------- rotate_iou.py, float32 with numba's promotions
__device__ __forceinline__ void rbbox_to_corners(float cx, float cy, float xd, float yd, float ang, float c[8]) {
    const float ac = cosf(ang), as = sinf(ang);
    // -x_d / 2 is a float64 division in numba; halving is exact, so the float32 store equals the float32 halving
    const float hx = (float)((double)xd / 2.0), hy = (float)((double)yd / 2.0);
    const float px[4] = {-hx, -hx, hx, hx};
    const float py[4] = {-hy, hy, hy, -hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = ac * px[i] + as * py[i] + cx;
        c[2 * i + 1] = -as * px[i] + ac * py[i] + cy;
    }
}

__device__ __forceinline__ bool point_in_quadrilateral(float x, float y, const float c[8]) {
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1];
    const float ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = x - c[0], ap1 = y - c[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

// line_segment_intersection (not _v1); i, j are compile-time after unrolling
__device__ __forceinline__ bool line_segment_intersection(const float p1[8], const float p2[8], int i, int j,
                                                          float &ox, float &oy) {
    const float A0 = p1[2 * i], A1 = p1[2 * i + 1];
    const float B0 = p1[2 * ((i + 1) % 4)], B1 = p1[2 * ((i + 1) % 4) + 1];
    const float C0 = p2[2 * j], C1 = p2[2 * j + 1];
    const float D0 = p2[2 * ((j + 1) % 4)], D1 = p2[2 * ((j + 1) % 4) + 1];
    const float BA0 = B0 - A0, BA1 = B1 - A1;
    const float DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd != bcd) {
        const bool abc = CA1 * BA0 > BA1 * CA0;
        const bool abd = DA1 * BA0 > BA1 * DA0;
        if (abc != abd) {
            const float DC0 = D0 - C0, DC1 = D1 - C1;
            const float ABBA = A0 * B1 - B0 * A1;
            const float CDDC = C0 * D1 - D0 * C1;
            const float DH = BA1 * DC0 - BA0 * DC1;
            const float Dx = ABBA * DC0 - BA0 * CDDC;
            const float Dy = ABBA * DC1 - BA1 * CDDC;
            ox = Dx / DH;
            oy = Dy / DH;
            return true;
        }
    }
    return false;
}

// float64 intersection area of rbox1 (the query box) and rbox2; pts/vs: this lane's LDS columns (stride 64)
__device__ double rotated_inter(const float r1[5], const float r2[5], float *pts, float *vs) {
    float c1[8], c2[8];
    rbbox_to_corners(r1[0], r1[1], r1[2], r1[3], r1[4], c1);
    rbbox_to_corners(r2[0], r2[1], r2[2], r2[3], r2[4], c2);
    int n = 0;
#define KE_PUT(X, Y) do { pts[(2 * n) * KE_OV_THREADS] = (X); pts[(2 * n + 1) * KE_OV_THREADS] = (Y); ++n; } while (0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (point_in_quadrilateral(c1[2 * i], c1[2 * i + 1], c2)) KE_PUT(c1[2 * i], c1[2 * i + 1]);
        if (point_in_quadrilateral(c2[2 * i], c2[2 * i + 1], c1)) KE_PUT(c2[2 * i], c2[2 * i + 1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x, y;
            if (line_segment_intersection(c1, c2, i, j, x, y)) KE_PUT(x, y);
        }
    }
#undef KE_PUT
#define P(k) pts[(k) * KE_OV_THREADS]
#define V(k) vs[(k) * KE_OV_THREADS]
    // sort_vertex_in_convex_polygon
    if (n > 0) {
        float cx = 0.f, cy = 0.f;
        for (int i = 0; i < n; ++i) {
            cx += P(2 * i);
            cy += P(2 * i + 1);
        }
        cx = (float)((double)cx / (double)n);   // center[0] /= num_of_inter: float32 / int32 is float64 in numba
        cy = (float)((double)cy / (double)n);
        for (int i = 0; i < n; ++i) {
            float v0 = P(2 * i) - cx, v1 = P(2 * i + 1) - cy;
            const float d = sqrtf(v0 * v0 + v1 * v1);
            v0 = v0 / d;
            v1 = v1 / d;
            if (v1 < 0) v0 = (float)(-2.0 - (double)v0);
            V(i) = v0;
        }
        for (int i = 1; i < n; ++i) {
            if (V(i - 1) > V(i)) {
                const float temp = V(i), tx = P(2 * i), ty = P(2 * i + 1);
                int j = i;
                while (j > 0 && V(j - 1) > temp) {
                    V(j) = V(j - 1);
                    P(j * 2) = P(j * 2 - 2);
                    P(j * 2 + 1) = P(j * 2 - 1);
                    --j;
                }
                V(j) = temp;
                P(j * 2) = tx;
                P(j * 2 + 1) = ty;
            }
        }
    }
    // area: the triangle fan, each triangle's float32 cross product halved in float64
    double area = 0.0;
    const float a0 = P(0), a1 = P(1);
    for (int i = 0; i < n - 2; ++i) {
        const float b0 = P(2 * i + 2), b1 = P(2 * i + 3), q0 = P(2 * i + 4), q1 = P(2 * i + 5);
        const float cr = (a0 - q0) * (b1 - q1) - (a1 - q1) * (b0 - q0);
        area += fabs((double)cr / 2.0);
    }
#undef P
#undef V
    return area;
}

__global__ void __launch_bounds__(KE_OV_THREADS)
ke_overlaps(const modest_eval_frame *__restrict__ fr, int n_frames, long long pair_base, long long n_pairs,
            const double *__restrict__ dtb, const double *__restrict__ gtb, const double *__restrict__ dtbb,
            const double *__restrict__ gtbb, int crit_bev, int crit_3d, int crit_img, float *__restrict__ bev,
            float *__restrict__ d3, double *__restrict__ img) {
    __shared__ float s_pts[2 * KE_POLY * KE_OV_THREADS];
    __shared__ float s_vs[KE_POLY * KE_OV_THREADS];
    const long long p = (long long)blockIdx.x * KE_OV_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    const long long gp = p + pair_base;
    int lo = 0, hi = n_frames - 1;   // last frame whose pair_off <= gp (empty frames share offsets: take the last)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (fr[mid].pair_off <= gp) lo = mid; else hi = mid - 1;
    }
    const modest_eval_frame F = fr[lo];
    const long long q = gp - F.pair_off;
    const long long j = F.dt_off + q / F.ng, i = F.gt_off + q % F.ng;   // overlaps[j, i]: dt row j, gt column i
    const double *bd = dtb + 7 * j, *bg = gtb + 7 * i;                  // x y z l h w ry (camera)
    if (bev || d3) {
        // rotate_iou_kernel_eval: devRotateIoUEval(qbox = gt, box = dt), boxes cast to float32 first
        const float r1[5] = {(float)bg[0], (float)bg[2], (float)bg[3], (float)bg[5], (float)bg[6]};
        const float r2[5] = {(float)bd[0], (float)bd[2], (float)bd[3], (float)bd[5], (float)bd[6]};
        // Coincident boxes are degenerate for the polygon walk (which corners count as inside each other is decided by
        // float32 rounding, so the reference returns anything from 0 to 1 there): their intersection is the box.
        const bool same = r1[0] == r2[0] && r1[1] == r2[1] && r1[2] == r2[2] && r1[3] == r2[3] && r1[4] == r2[4];
        const double inter = same ? (double)(r1[2] * r1[3]) : rotated_inter(r1, r2, s_pts + threadIdx.x, s_vs + threadIdx.x);
        if (bev) {
            const float area1 = r1[2] * r1[3], area2 = r2[2] * r2[3];
            double v;
            if (crit_bev == -1) v = inter / ((double)(area1 + area2) - inter);
            else if (crit_bev == 0) v = inter / (double)area1;
            else if (crit_bev == 1) v = inter / (double)area2;
            else v = inter;
            bev[p] = (float)v;
        }
        if (d3) {
            // d3_box_overlap_kernel: boxes = dt, qboxes = gt, rinc = the float32 intersection area
            const float rinc = (float)inter;
            float out = rinc;
            if (rinc > 0) {
                const double iw = fmin(bd[1], bg[1]) - fmax(bd[1] - bd[4], bg[1] - bg[4]);
                if (iw > 0) {
                    const double area1 = bd[3] * bd[4] * bd[5], area2 = bg[3] * bg[4] * bg[5];
                    const double inc = iw * (double)rinc;
                    double ua;
                    if (crit_3d == -1) ua = area1 + area2 - inc;
                    else if (crit_3d == 0) ua = area1;
                    else if (crit_3d == 1) ua = area2;
                    else ua = inc;
                    out = (float)(inc / ua);
                } else {
                    out = 0.f;
                }
            }
            d3[p] = out;
        }
    }
    if (img) {
        // image_box_overlap(boxes = dt, query_boxes = gt), float64
        const double *b = dtbb + 4 * j, *k = gtbb + 4 * i;
        const double qa = (k[2] - k[0]) * (k[3] - k[1]);
        double v = 0.0;
        const double iw = fmin(b[2], k[2]) - fmax(b[0], k[0]);
        if (iw > 0) {
            const double ih = fmin(b[3], k[3]) - fmax(b[1], k[1]);
            if (ih > 0) {
                double ua;
                if (crit_img == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qa - iw * ih;
                else if (crit_img == 0) ua = (b[2] - b[0]) * (b[3] - b[1]);
                else if (crit_img == 1) ua = qa;
                else ua = 1.0;
                v = iw * ih / ua;
            }
        }
        img[p] = v;
    }
}

// ---------------------------------------------------------------- compute_statistics_jit
template <typename OV>
__device__ void match_frame(const modest_eval_stats_args &a, const OV *__restrict__ ov, long long pair_base,
                            const modest_eval_frame &F, int f, int c, int t, bool compute_fp, unsigned *bits) {
    const modest_eval_config cf = a.cfg[c];
    const int nd = F.nd, ng = F.ng;
    const int8_t *ig = a.gt_ign + (long long)cf.flagset * a.n_gt + F.gt_off;
    const int8_t *id = a.dt_ign + (long long)cf.flagset * a.n_dt + F.dt_off;
    const double *sc = a.dt_score + F.dt_off;
    const OV *o = ov + (F.pair_off - pair_base);
    const double mo = cf.min_overlap;
    const double thresh = compute_fp ? a.thresholds[c * KE_TMAX + t] : 0.0;
    const int words = (nd + 31) >> 5;
    for (int w = 0; w < words; ++w) bits[w * 64] = 0u;
#define ASSIGNED(jj) ((bits[((jj) >> 5) * 64] >> ((jj) & 31)) & 1u)
#define ASSIGN(jj) (bits[((jj) >> 5) * 64] |= 1u << ((jj) & 31))
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    const bool aos = compute_fp && a.pair_sim != nullptr;
    const double *ps = aos ? a.pair_sim + (F.pair_off - pair_base) : nullptr;
    for (int i = 0; i < ng; ++i) {
        const int gi = ig[i];
        if (gi == -1) continue;
        int det_idx = -1;
        double valid = KE_NO_DETECTION, max_overlap = 0.0;
        bool assigned_ignored_det = false;
        for (int j = 0; j < nd; ++j) {
            const int dj = id[j];
            if (dj == -1 || ASSIGNED(j)) continue;
            const double s = sc[j];
            if (compute_fp && s < thresh) continue;
            const double v = (double)o[(long long)j * ng + i];
            if (!compute_fp && v > mo && s > valid) {
                det_idx = j;
                valid = s;
            } else if (compute_fp && v > mo && (v > max_overlap || assigned_ignored_det) && dj == 0) {
                max_overlap = v;
                det_idx = j;
                valid = 1.0;
                assigned_ignored_det = false;
            } else if (compute_fp && v > mo && valid == KE_NO_DETECTION && dj == 1) {
                det_idx = j;
                valid = 1.0;
                assigned_ignored_det = true;
            }
        }
        if (valid == KE_NO_DETECTION && gi == 0) {
            ++fn;
        } else if (valid != KE_NO_DETECTION && (gi == 1 || id[det_idx] == 1)) {
            ASSIGN(det_idx);
        } else if (valid != KE_NO_DETECTION) {
            ++tp;
            if (!compute_fp) {
                a.tp_scores[(long long)c * a.n_gt + F.gt_off + i] = sc[det_idx];
                atomicAdd(a.tp_count + c, 1);
            } else if (aos) {
                sim += ps[(long long)det_idx * ng + i];   // np.sum(tmp): fp zeros, then the deltas in gt order
            }
            ASSIGN(det_idx);
        }
    }
    if (!compute_fp) return;
    for (int j = 0; j < nd; ++j) {
        const int dj = id[j];
        if (!(ASSIGNED(j) || dj == -1 || dj == 1 || sc[j] < thresh)) ++fp;
    }
    if (a.metric == 0 && a.gt_dc) {
        // DontCare boxes (gt order) against unassigned detections, image_box_overlap criterion 0
        const uint8_t *dc = a.gt_dc + (long long)cf.flagset * a.n_gt + F.gt_off;
        int nstuff = 0;
        for (int i = 0; i < ng; ++i) {
            if (!dc[i]) continue;
            const double *k = a.gt_bbox + 4 * (F.gt_off + i);
            for (int j = 0; j < nd; ++j) {
                const int dj = id[j];
                if (ASSIGNED(j) || dj == -1 || dj == 1 || sc[j] < thresh) continue;
                const double *b = a.dt_bbox + 4 * (F.dt_off + j);
                double v = 0.0;
                const double iw = fmin(b[2], k[2]) - fmax(b[0], k[0]);
                if (iw > 0) {
                    const double ih = fmin(b[3], k[3]) - fmax(b[1], k[1]);
                    if (ih > 0) v = iw * ih / ((b[2] - b[0]) * (b[3] - b[1]));
                }
                if (v > mo) {
                    ASSIGN(j);
                    ++nstuff;
                }
            }
        }
        fp -= nstuff;
    }
#undef ASSIGNED
#undef ASSIGN
    const long long slot = ((long long)c * KE_TMAX + t) * a.n_frames + f;
    reinterpret_cast<int4 *>(a.partial)[slot] = make_int4(tp, fp, fn, 0);
    if (a.sim_partial) a.sim_partial[slot] = aos && (tp > 0 || fp > 0) ? sim : NAN;   // NaN: similarity == -1
}

template <typename OV, bool PASS_B>
__global__ void __launch_bounds__(64) ke_match(modest_eval_stats_args a, const OV *__restrict__ ov, long long pair_base,
                                               int frame_begin) {
    extern __shared__ unsigned s_bits[];
    const int f = frame_begin + blockIdx.x;
    const int lane = threadIdx.x;
    int c, t;
    if (PASS_B) {
        c = blockIdx.y;
        t = lane;
        if (t >= a.n_thresh[c]) return;
    } else {
        c = blockIdx.y * 64 + lane;
        t = 0;
        if (c >= a.n_cfg) return;
    }
    const modest_eval_frame F = a.frames[f];
    match_frame<OV>(a, ov, pair_base, F, f, c, t, PASS_B, s_bits + lane);
}

// ---------------------------------------------------------------- get_thresholds
__device__ __forceinline__ bool thr_skip(long long i, long long n, double g, double cur) {
    const double l = (double)(i + 1) / g;
    const double r = i < n - 1 ? (double)(i + 2) / g : l;
    return (r - cur) < (cur - l) && i < n - 1;
}

__global__ void ke_thresholds(modest_eval_stats_args a, const double *__restrict__ sorted) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cfg) return;
    const long long n = a.tp_count[c];
    const double g = (double)a.cfg[c].num_valid_gt;
    const double *s = sorted + (long long)c * a.n_gt;
    double cur = 0.0;
    long long start = 0;
    int k = 0;
    while (start < n) {
        // skip(i) is monotone in i (l, r grow with i; the last index is never skipped): the first kept index
        long long lo = start, hi = n - 1;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (thr_skip(mid, n, g, cur)) lo = mid + 1; else hi = mid;
        }
        if (k < KE_TMAX) a.thresholds[c * KE_TMAX + k] = s[lo];
        ++k;
        cur += 1.0 / (41 - 1.0);
        start = lo + 1;
    }
    a.n_thresh[c] = k > KE_TMAX ? -k : k;
}

// ---------------------------------------------------------------- sums over frames
__global__ void __launch_bounds__(256) ke_reduce(modest_eval_stats_args a, double *__restrict__ pr) {
    const int c = blockIdx.y, t = blockIdx.x;
    const int nt = a.n_thresh[c];
    if (t >= nt) return;
    const long long base = ((long long)c * KE_TMAX + t) * a.n_frames;
    const int4 *p = reinterpret_cast<const int4 *>(a.partial) + base;
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int f = threadIdx.x; f < a.n_frames; f += 256) {
        const int4 v = p[f];
        s0 += v.x;
        s1 += v.y;
        s2 += v.z;
    }
    __shared__ long long red[3][256];
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sim = 0.0;
        if (a.sim_partial) {
            const double *q = a.sim_partial + base;
            for (int f = 0; f < a.n_frames; ++f) {
                const double v = q[f];
                if (v == v) sim += v;
            }
        }
        double *o = pr + ((long long)c * KE_TMAX + t) * 4;
        o[0] = (double)red[0][0];
        o[1] = (double)red[1][0];
        o[2] = (double)red[2][0];
        o[3] = sim;
    }
}

}  // namespace

extern "C" int modest_eval_limits(int32_t *max_thresholds, int32_t *max_dt_per_frame) {
    MODEST_REQUIRE(max_thresholds && max_dt_per_frame, "NULL argument");
    *max_thresholds = KE_TMAX;
    *max_dt_per_frame = KE_MAX_WORDS * 32;
    return MODEST_OK;
}

extern "C" int modest_eval_overlaps(const modest_eval_frame *frames_dev, int n_frames, int64_t pair_base, int64_t n_pairs,
                                    const double *dt_boxes, const double *gt_boxes, const double *dt_bbox,
                                    const double *gt_bbox, int crit_bev, int crit_3d, int crit_img, float *bev_out,
                                    float *d3_out, double *img_out, void *stream_) {
    MODEST_REQUIRE(n_frames >= 0 && n_pairs >= 0 && pair_base >= 0, "bad sizes");
    if (n_pairs == 0) return MODEST_OK;
    MODEST_REQUIRE(frames_dev && n_frames > 0, "NULL frames");
    MODEST_REQUIRE(bev_out || d3_out || img_out, "no output requested");
    MODEST_REQUIRE(!(bev_out || d3_out) || (dt_boxes && gt_boxes), "NULL boxes");
    MODEST_REQUIRE(!img_out || (dt_bbox && gt_bbox), "NULL image boxes");
    const long long blocks = (n_pairs + KE_OV_THREADS - 1) / KE_OV_THREADS;
    MODEST_REQUIRE(blocks <= 0x7fffffffLL, "too many pairs for one launch");
    hipStream_t stream = as_stream(stream_);
    ke_overlaps<<<(unsigned)blocks, KE_OV_THREADS, 0, stream>>>(frames_dev, n_frames, pair_base, n_pairs, dt_boxes, gt_boxes,
                                                                dt_bbox, gt_bbox, crit_bev, crit_3d, crit_img, bev_out,
                                                                d3_out, img_out);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_eval_statistics(int stage, const modest_eval_stats_args *args, int frame_begin, int frame_end,
                                      const void *overlaps, int overlaps_f64, int64_t pair_base, const double *sorted,
                                      double *pr_out, void *stream_) {
    MODEST_REQUIRE(args != nullptr, "NULL args");
    const modest_eval_stats_args a = *args;
    MODEST_REQUIRE(a.n_cfg > 0 && a.n_cfg <= 65535 && a.n_frames >= 0 && a.frames && a.cfg, "bad configuration table");
    MODEST_REQUIRE(a.max_nd >= 0 && a.max_nd <= KE_MAX_WORDS * 32, "a frame holds more detections than the bitmap");
    hipStream_t stream = as_stream(stream_);
    const size_t lds = (size_t)64 * std::max(1, (a.max_nd + 31) / 32) * sizeof(unsigned);
    if (stage == 0 || stage == 2) {
        MODEST_REQUIRE(0 <= frame_begin && frame_begin <= frame_end && frame_end <= a.n_frames, "bad frame range");
        MODEST_REQUIRE(a.gt_ign && a.dt_ign && a.dt_score, "NULL flags");
        if (frame_end == frame_begin) return MODEST_OK;
        MODEST_REQUIRE(overlaps != nullptr, "NULL overlaps");
        const unsigned nf = (unsigned)(frame_end - frame_begin);
        if (stage == 0) {
            MODEST_REQUIRE(a.tp_scores && a.tp_count, "NULL pass A outputs");
            dim3 grid(nf, (a.n_cfg + 63) / 64);
            if (overlaps_f64)
                ke_match<double, false><<<grid, 64, lds, stream>>>(a, (const double *)overlaps, pair_base, frame_begin);
            else
                ke_match<float, false><<<grid, 64, lds, stream>>>(a, (const float *)overlaps, pair_base, frame_begin);
        } else {
            MODEST_REQUIRE(a.thresholds && a.n_thresh && a.partial, "NULL pass B buffers");
            MODEST_REQUIRE(a.metric != 0 || a.dt_bbox, "metric 0 needs the image boxes");
            MODEST_REQUIRE(!a.gt_dc || a.gt_bbox, "DontCare flags need the gt image boxes");
            dim3 grid(nf, a.n_cfg);
            if (overlaps_f64)
                ke_match<double, true><<<grid, 64, lds, stream>>>(a, (const double *)overlaps, pair_base, frame_begin);
            else
                ke_match<float, true><<<grid, 64, lds, stream>>>(a, (const float *)overlaps, pair_base, frame_begin);
        }
    } else if (stage == 1) {
        MODEST_REQUIRE(sorted && a.tp_count && a.thresholds && a.n_thresh, "NULL threshold buffers");
        ke_thresholds<<<(a.n_cfg + 63) / 64, 64, 0, stream>>>(a, sorted);
    } else if (stage == 3) {
        MODEST_REQUIRE(pr_out && a.partial && a.n_thresh, "NULL reduction buffers");
        if (a.n_frames == 0) return MODEST_OK;
        ke_reduce<<<dim3(KE_TMAX, a.n_cfg), 256, 0, stream>>>(a, pr_out);
    } else {
        MODEST_REQUIRE(false, "stage must be 0 (pass A), 1 (thresholds), 2 (pass B) or 3 (sums)");
    }
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
