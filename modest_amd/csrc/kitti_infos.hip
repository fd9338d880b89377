// Dataset infos + ground-truth database of OpenPCDet's create_kitti_infos, batched over frames (gfx950).
//
// Reference (downstream/OpenPCDet/pcdet/):
//   datasets/kitti/kitti_dataset.py:158-173 get_fov_flag, utils/calibration_kitti.py:64-84 lidar_to_rect / rect_to_img
//   datasets/kitti/kitti_dataset.py:239-251  num_points_in_gt = in_hull(points of the field of view, corners of the box)
//   datasets/kitti/kitti_dataset.py:261-314  create_groundtruth_database: points[mask > 0], [:, :3] -= centre
//   ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168  check_pt_in_box3d_cpu, the membership predicate of the database
//
// Two kernels walk the same work decomposition: grid.y = frame, every wavefront owns IK_WAVE_PTS consecutive rows
// of its frame (a "chunk"), a workgroup of four wavefronts shares the frame's boxes in LDS (at most `pass` <= 256 per
// pass; a frame with more boxes takes further passes over the same rows).
//   infos_count   per (chunk, box) the number of database members  -> wcount[chunk][box]
//                 per box the FOV points the float64 box test decides inside (integer atomic add: the sum does not
//                 depend on the order), and the row numbers of the FOV points it cannot decide (|margin| < tau)
//   infos_scan    per (frame, box) the exclusive prefix over the frame's chunks, in place, and db_count
//   infos_gather  the member rows, centre subtracted, at box_base[box] + prefix[chunk][box] + rank in the wavefront
// The output position of a row is a pure function of the counts (ballot prefix inside a wavefront, counted bases
// across wavefronts), never of an atomic's return value: the rows of a box come out in file order on every run.
//
// Arithmetic.  Compiled with -ffp-contract=off; every fused multiply-add below is written out.
//   FOV flag: float32.  rect = [x y z 1] @ (V2C.T @ R0.T) and hom = [rect 1] @ P2.T go through numpy's sgemm, whose k
//   loop for these shapes is the chain acc = x*m0; fmaf(y, m1, acc); fmaf(z, m2, acc); acc + m3 (the chain
//   transform.hip pins in float64) -- that chain reproduces the flags recorded in tests/golden/kitti_infos.npz.
//   u = hom0 / rect_z, v = hom1 / rect_z (IEEE float32 division; a zero rect_z gives inf / nan as numpy does and
//   every comparison with nan is false), depth = hom2 - P2.T[3][2]; 0 <= u < W, 0 <= v < H, depth >= 0.
//   Database predicate: float32 differences and products, un-fused; cosf / sinf(-rz) are the HOST libm's (called through ctypes), passed with the
//   box table (no device libm reproduces them); the three comparisons in double, MARGIN = (float)1e-2.
//   Hull predicate: float64 margin of the point against the ideal box, m = min(dx/2-|lx|, dy/2-|ly|, dz/2-|lz|);
//   m >= tau inside, m <= -tau outside, else undecided and left to the host's Delaunay (modest_amd/kitti_infos.py).
//   A NaN coordinate makes m a NaN: neither inside nor undecided.  The extents come without their sign (_box_table).
//
// A cheap float32 test discards a (row, box) pair before either predicate: max(|x-cx|, |y-cy|) > reject, where the
// host sets reject above the half diagonal of the box footprint plus both margins plus the rounding of the float32
// differences, so no discarded pair can be a member or undecided.  A whole wavefront skips a box none of its rows is
// near.
#include "common.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int IK_THREADS = 256;
constexpr int IK_WAVES = IK_THREADS / 64;
constexpr int IK_ITERS = 8;                       // rows per lane and chunk
constexpr int IK_WAVE_PTS = 64 * IK_ITERS;        // rows per chunk (wavefront)
constexpr int IK_WG_PTS = IK_WAVE_PTS * IK_WAVES;
constexpr int IK_MAX_PASS = MODEST_INFOS_MAX_PASS;

static_assert(sizeof(modest_infos_frame) == 144, "modest_infos_frame layout");
static_assert(sizeof(modest_infos_box) == 128, "modest_infos_box layout");

struct InfosBufs {
    const float4 *rows;
    const modest_infos_frame *frames;
    const modest_infos_box *boxes;
    int32_t *wcount;       // per frame at cnt_offset: [chunks][box_count]
    int32_t *hull_count;   // per box
    int32_t *und_n;        // per box: undecided FOV points seen (may exceed und_cap: overflow)
    int32_t *und_idx;      // per box und_cap row numbers (frame-local)
    int32_t *db_count;     // per box
    uint8_t *fov;          // optional, per row
    int32_t *dense;        // optional, (n_boxes, dense_stride): the database predicate of every pair
    long long dense_stride;
    int und_cap;
    int pass;
};

__device__ __forceinline__ bool fov_flag(const float4 p, const modest_infos_frame &F) {
    float r[3], h[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float acc = __fmul_rn(p.x, F.m1[j]);
        acc = fmaf(p.y, F.m1[3 + j], acc);
        acc = fmaf(p.z, F.m1[6 + j], acc);
        r[j] = __fadd_rn(acc, F.m1[9 + j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float acc = __fmul_rn(r[0], F.p2t[j]);
        acc = fmaf(r[1], F.p2t[3 + j], acc);
        acc = fmaf(r[2], F.p2t[6 + j], acc);
        h[j] = __fadd_rn(acc, F.p2t[9 + j]);
    }
    const float u = __fdiv_rn(h[0], r[2]), v = __fdiv_rn(h[1], r[2]);
    const float depth = __fsub_rn(h[2], F.p2t[11]);
    return u >= 0.f && (double)u < (double)F.width && v >= 0.f && (double)v < (double)F.height && depth >= 0.f;
}

// roiaware_pool3d.cpp:128-143 for a pair that passed the reject test
__device__ __forceinline__ bool db_member(const float4 p, const modest_infos_box &B, float sx, float sy) {
    const float sz = __fsub_rn(p.z, B.bf[2]);
    if (fabs((double)sz) > (double)B.bf[5] / 2.0) return false;
    const float lx = __fadd_rn(__fmul_rn(sx, B.cosa), __fmul_rn(sy, -B.sina));
    const float ly = __fadd_rn(__fmul_rn(sx, B.sina), __fmul_rn(sy, B.cosa));
    const double margin = (double)1e-2f;
    return (fabs((double)lx) < (double)B.bf[3] / 2.0 + margin) && (fabs((double)ly) < (double)B.bf[4] / 2.0 + margin);
}

// margin of the point against the ideal float64 box (positive inside)
__device__ __forceinline__ double hull_margin(const float4 p, const modest_infos_box &B) {
    const double sx = (double)p.x - B.b[0], sy = (double)p.y - B.b[1], sz = (double)p.z - B.b[2];
    const double lx = fma(sy, B.cs[1], sx * B.cs[0]);
    const double ly = fma(sy, B.cs[0], -(sx * B.cs[1]));
    const double mx = B.b[3] * 0.5 - fabs(lx), my = B.b[4] * 0.5 - fabs(ly), mz = B.b[5] * 0.5 - fabs(sz);
    // a row with a NaN coordinate is neither inside nor undecided (Delaunay.find_simplex answers -1 for it): its margin
    // is a NaN, which fails both comparisons.  fmin alone hands back the operand that is not a NaN, the margin of the
    // other axes (and the reject test's fmaxf lets such a row through, which keeps that test conservative).
    if (mx != mx || my != my || mz != mz) return mx + my + mz;
    return fmin(mx, fmin(my, mz));
}

__device__ __forceinline__ void load_boxes(modest_infos_box *s_box, const modest_infos_box *src, int nb) {
    const uint4 *g = reinterpret_cast<const uint4 *>(src);
    uint4 *s = reinterpret_cast<uint4 *>(s_box);
    for (int i = threadIdx.x; i < nb * (int)(sizeof(modest_infos_box) / 16); i += IK_THREADS) s[i] = g[i];
}

__global__ __launch_bounds__(IK_THREADS) void infos_count(InfosBufs A) {
    __shared__ modest_infos_box s_box[IK_MAX_PASS];
    __shared__ int s_db[IK_WAVES][IK_MAX_PASS];
    __shared__ int s_hull[IK_WAVES][IK_MAX_PASS];
    __shared__ modest_infos_frame s_fr;
    const int f = blockIdx.y;
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(A.frames + f);
        if (threadIdx.x < sizeof(modest_infos_frame) / 16) reinterpret_cast<uint4 *>(&s_fr)[threadIdx.x] = g[threadIdx.x];
    }
    __syncthreads();
    const int n = s_fr.n, nbox = s_fr.box_count;
    if ((long long)blockIdx.x * IK_WG_PTS >= n) return;               // (whole workgroup)
    if (nbox == 0 && A.fov == nullptr) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int chunk = blockIdx.x * IK_WAVES + w;
    const int first = chunk * IK_WAVE_PTS;
    const float4 *rows = A.rows + s_fr.row_offset;
    float4 p[IK_ITERS];
    unsigned fovbits = 0;
#pragma unroll
    for (int it = 0; it < IK_ITERS; ++it) {
        const int i = first + it * 64 + lane;
        p[it] = i < n ? rows[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const bool fv = i < n && fov_flag(p[it], s_fr);
        if (A.fov && i < n) A.fov[s_fr.row_offset + i] = fv ? 1 : 0;
        const bool counted = i < n && (fv || !s_fr.fov_only);
        fovbits |= (counted ? 1u : 0u) << it;
    }
    const int nchunks = (n + IK_WAVE_PTS - 1) / IK_WAVE_PTS;
    for (int base = 0; base < nbox; base += A.pass) {
        const int nb = min(A.pass, nbox - base);
        __syncthreads();
        load_boxes(s_box, A.boxes + s_fr.box_begin + base, nb);
        for (int b = lane; b < nb; b += 64) s_db[w][b] = 0, s_hull[w][b] = 0;
        __syncthreads();
        if (first < n) {
#pragma unroll 1
            for (int b = 0; b < nb; ++b) {
                const modest_infos_box &B = s_box[b];
                const int gb = s_fr.box_begin + base + b;
                int ndb = 0, nh = 0;
#pragma unroll
                for (int it = 0; it < IK_ITERS; ++it) {
                    const int i = first + it * 64 + lane;
                    const float sx = __fsub_rn(p[it].x, B.bf[0]), sy = __fsub_rn(p[it].y, B.bf[1]);
                    const bool near = i < n && fmaxf(fabsf(sx), fabsf(sy)) <= B.reject;
                    if (__ballot(near) == 0ULL) continue;
                    const bool mem = near && db_member(p[it], B, sx, sy);
                    ndb += __popcll(__ballot(mem));
                    if (A.dense && mem) A.dense[(long long)gb * A.dense_stride + i] = 1;
                    bool inside = false;
                    if (near && ((fovbits >> it) & 1u)) {
                        const double m = hull_margin(p[it], B);
                        inside = m >= B.tau;
                        if (!inside && m > -B.tau) {
                            const int pos = atomicAdd(A.und_n + gb, 1);
                            if (pos < A.und_cap) A.und_idx[(long long)gb * A.und_cap + pos] = i;
                        }
                    }
                    nh += __popcll(__ballot(inside));
                }
                if (lane == 0) s_db[w][b] = ndb, s_hull[w][b] = nh;
            }
        }
        __syncthreads();
        if (chunk < nchunks) {
            int32_t *wc = A.wcount + s_fr.cnt_offset + (long long)chunk * nbox + base;
            for (int b = lane; b < nb; b += 64) {
                wc[b] = s_db[w][b];
                if (s_hull[w][b]) atomicAdd(A.hull_count + s_fr.box_begin + base + b, s_hull[w][b]);
            }
        }
    }
}

// one thread per (frame, box): exclusive prefix over the frame's chunks, in place
__global__ __launch_bounds__(IK_THREADS) void infos_scan(InfosBufs A) {
    const modest_infos_frame &F = A.frames[blockIdx.y];
    const int b = blockIdx.x * IK_THREADS + threadIdx.x;
    if (b >= F.box_count) return;
    const int nchunks = (F.n + IK_WAVE_PTS - 1) / IK_WAVE_PTS;
    int32_t *wc = A.wcount + F.cnt_offset + b;
    int run = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int v = wc[(long long)c * F.box_count];
        wc[(long long)c * F.box_count] = run;
        run += v;
    }
    A.db_count[F.box_begin + b] = run;
}

__global__ __launch_bounds__(IK_THREADS) void infos_gather(InfosBufs A, const long long *box_base, float4 *out) {
    __shared__ modest_infos_box s_box[IK_MAX_PASS];
    __shared__ int s_run[IK_WAVES][IK_MAX_PASS];
    __shared__ modest_infos_frame s_fr;
    const int f = blockIdx.y;
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(A.frames + f);
        if (threadIdx.x < sizeof(modest_infos_frame) / 16) reinterpret_cast<uint4 *>(&s_fr)[threadIdx.x] = g[threadIdx.x];
    }
    __syncthreads();
    const int n = s_fr.n, nbox = s_fr.box_count;
    if ((long long)blockIdx.x * IK_WG_PTS >= n || nbox == 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int chunk = blockIdx.x * IK_WAVES + w;
    const int first = chunk * IK_WAVE_PTS;
    const float4 *rows = A.rows + s_fr.row_offset;
    float4 p[IK_ITERS];
#pragma unroll
    for (int it = 0; it < IK_ITERS; ++it) {
        const int i = first + it * 64 + lane;
        p[it] = i < n ? rows[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const unsigned long long below = (1ULL << lane) - 1ULL;
    for (int base = 0; base < nbox; base += A.pass) {
        const int nb = min(A.pass, nbox - base);
        __syncthreads();
        load_boxes(s_box, A.boxes + s_fr.box_begin + base, nb);
        if (first < n) {
            const int32_t *wc = A.wcount + s_fr.cnt_offset + (long long)chunk * nbox + base;
            for (int b = lane; b < nb; b += 64) s_run[w][b] = wc[b];
        }
        __syncthreads();
        if (first >= n) continue;
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            const modest_infos_box &B = s_box[b];
            const int gb = s_fr.box_begin + base + b;
            int run = s_run[w][b];   // (written before the barrier, read-only from here on)
            float4 *dst = out + box_base[gb];
#pragma unroll
            for (int it = 0; it < IK_ITERS; ++it) {
                const int i = first + it * 64 + lane;
                const float sx = __fsub_rn(p[it].x, B.bf[0]), sy = __fsub_rn(p[it].y, B.bf[1]);
                const bool near = i < n && fmaxf(fabsf(sx), fabsf(sy)) <= B.reject;
                if (__ballot(near) == 0ULL) continue;
                const bool mem = near && db_member(p[it], B, sx, sy);
                const unsigned long long bal = __ballot(mem);
                if (mem) {
                    // numpy's in-place float32 -= float64: the difference in float64, rounded once
                    float4 q;
                    q.x = (float)((double)p[it].x - B.b[0]);
                    q.y = (float)((double)p[it].y - B.b[1]);
                    q.z = (float)((double)p[it].z - B.b[2]);
                    q.w = p[it].w;
                    dst[run + __popcll(bal & below)] = q;
                }
                run += __popcll(bal);
            }
        }
    }
}

int check_tables(const modest_infos_frame *fr, int n_frames, bool have_boxes, int n_boxes, long long n_rows,
                 long long wcount_words, int pass, int *max_n, int *max_boxes) {
    MODEST_REQUIRE(n_frames >= 1 && n_frames <= 65535, "1..65535 frames per call");
    MODEST_REQUIRE(n_boxes >= 0 && (n_boxes == 0 || have_boxes), "bad boxes");
    MODEST_REQUIRE(pass >= 1 && pass <= IK_MAX_PASS, "pass_boxes must lie in 1..MODEST_INFOS_MAX_PASS");
    long long next_box = 0, next_cnt = 0;
    *max_n = 0, *max_boxes = 0;
    for (int f = 0; f < n_frames; ++f) {
        const modest_infos_frame &F = fr[f];
        MODEST_REQUIRE(F.n >= 0 && F.row_offset >= 0 && F.row_offset + F.n <= n_rows, "frame rows outside rows_dev");
        MODEST_REQUIRE(F.box_begin == next_box && F.box_count >= 0 && next_box + F.box_count <= n_boxes,
                       "boxes must be listed frame after frame");
        MODEST_REQUIRE(F.cnt_offset == next_cnt, "cnt_offset must be the running sum of chunks * box_count");
        next_box += F.box_count;
        next_cnt += (long long)((F.n + IK_WAVE_PTS - 1) / IK_WAVE_PTS) * F.box_count;
        *max_n = std::max(*max_n, F.n);
        *max_boxes = std::max(*max_boxes, F.box_count);
    }
    MODEST_REQUIRE(next_box == n_boxes, "frames do not cover the box table");
    MODEST_REQUIRE(next_cnt <= wcount_words, "wcount_dev too small: sum over frames of ceil(n / modest_infos_chunk_rows()) * box_count words");
    return MODEST_OK;
}

size_t table_bytes(int n_frames, int n_boxes) {
    return arena_sz(sizeof(modest_infos_frame) * (size_t)n_frames) + arena_sz(sizeof(modest_infos_box) * (size_t)std::max(n_boxes, 1));
}

}  // namespace

extern "C" int modest_infos_chunk_rows(void) { return IK_WAVE_PTS; }

extern "C" int modest_infos_count(const float *rows_dev, int64_t n_rows, const modest_infos_frame *frames_host, int n_frames,
                                  const modest_infos_box *boxes_host, int n_boxes, int pass_boxes, int und_cap,
                                  void *tables_dev, int64_t tables_bytes, int32_t *wcount_dev, int64_t wcount_words,
                                  int32_t *hull_count_dev, int32_t *und_n_dev, int32_t *und_idx_dev, int32_t *db_count_dev,
                                  uint8_t *fov_dev, int32_t *dense_dev, int64_t dense_stride, void *stream_) {
    MODEST_REQUIRE(frames_host && tables_dev && hull_count_dev && und_n_dev && db_count_dev, "NULL argument");
    MODEST_REQUIRE(und_cap >= 0 && (und_cap == 0 || und_idx_dev), "bad undecided capacity");
    MODEST_REQUIRE(n_rows >= 0 && (n_rows == 0 || rows_dev), "NULL rows");
    MODEST_REQUIRE((reinterpret_cast<uintptr_t>(rows_dev) & 15u) == 0 && (reinterpret_cast<uintptr_t>(tables_dev) & 255u) == 0,
                   "rows must be 16-byte and tables 256-byte aligned");
    int max_n = 0, max_boxes = 0;
    int rc = check_tables(frames_host, n_frames, boxes_host != nullptr, n_boxes, n_rows, wcount_words, pass_boxes, &max_n, &max_boxes);
    if (rc) return rc;
    MODEST_REQUIRE(wcount_dev || wcount_words == 0 || n_boxes == 0, "NULL wcount");
    MODEST_REQUIRE((size_t)tables_bytes >= table_bytes(n_frames, n_boxes), "tables_dev too small (modest_infos_table_bytes)");
    if (dense_dev) {
        for (int f = 0; f < n_frames; ++f) MODEST_REQUIRE(frames_host[f].n <= dense_stride, "dense_stride below a frame's rows");
    }
    hipStream_t stream = as_stream(stream_);
    Arena T(static_cast<char *>(tables_dev));
    modest_infos_frame *d_fr = T.take<modest_infos_frame>(n_frames);
    modest_infos_box *d_box = T.take<modest_infos_box>(std::max(n_boxes, 1));
    MODEST_HIP_CHECK(hipMemcpyAsync(d_fr, frames_host, sizeof(modest_infos_frame) * n_frames, hipMemcpyHostToDevice, stream));
    if (n_boxes) {
        MODEST_HIP_CHECK(hipMemcpyAsync(d_box, boxes_host, sizeof(modest_infos_box) * n_boxes, hipMemcpyHostToDevice, stream));
        MODEST_HIP_CHECK(hipMemsetAsync(hull_count_dev, 0, sizeof(int32_t) * n_boxes, stream));
        MODEST_HIP_CHECK(hipMemsetAsync(und_n_dev, 0, sizeof(int32_t) * n_boxes, stream));
        MODEST_HIP_CHECK(hipMemsetAsync(db_count_dev, 0, sizeof(int32_t) * n_boxes, stream));
    }
    if (max_n == 0) return MODEST_OK;
    InfosBufs A;
    A.rows = reinterpret_cast<const float4 *>(rows_dev);
    A.frames = d_fr, A.boxes = d_box, A.wcount = wcount_dev, A.hull_count = hull_count_dev, A.und_n = und_n_dev;
    A.und_idx = und_idx_dev, A.db_count = db_count_dev, A.fov = fov_dev, A.dense = dense_dev, A.dense_stride = dense_stride;
    A.und_cap = und_cap, A.pass = pass_boxes;
    if (n_boxes == 0 && !fov_dev) return MODEST_OK;
    const dim3 grid((max_n + IK_WG_PTS - 1) / IK_WG_PTS, n_frames);
    infos_count<<<grid, IK_THREADS, 0, stream>>>(A);
    MODEST_HIP_CHECK(hipGetLastError());
    if (max_boxes) {
        infos_scan<<<dim3((max_boxes + IK_THREADS - 1) / IK_THREADS, n_frames), IK_THREADS, 0, stream>>>(A);
        MODEST_HIP_CHECK(hipGetLastError());
    }
    return MODEST_OK;
}

extern "C" int modest_infos_gather(const float *rows_dev, int64_t n_rows, const modest_infos_frame *frames_host, int n_frames,
                                   int n_boxes, int pass_boxes, const void *tables_dev, const int32_t *wcount_dev,
                                   int64_t wcount_words, const int64_t *box_base_dev, const int32_t *db_count_host,
                                   const int64_t *box_base_host, float *out_rows_dev, int64_t out_rows, void *stream_) {
    MODEST_REQUIRE(frames_host && tables_dev && box_base_dev && db_count_host && box_base_host, "NULL argument");
    MODEST_REQUIRE((reinterpret_cast<uintptr_t>(rows_dev) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out_rows_dev) & 15u) == 0,
                   "rows must be 16-byte aligned");
    int max_n = 0, max_boxes = 0;
    int rc = check_tables(frames_host, n_frames, true, n_boxes, n_rows,
                          wcount_words, pass_boxes, &max_n, &max_boxes);
    if (rc) return rc;
    long long run = 0;
    for (int b = 0; b < n_boxes; ++b) {   // every box's slice lies inside out_rows_dev, slices do not overlap
        MODEST_REQUIRE(db_count_host[b] >= 0 && box_base_host[b] == run, "box_base must be the exclusive sum of db_count");
        run += db_count_host[b];
    }
    MODEST_REQUIRE(run <= out_rows && (run == 0 || out_rows_dev), "out_rows_dev too small");
    if (run == 0 || max_n == 0 || max_boxes == 0) return MODEST_OK;
    hipStream_t stream = as_stream(stream_);
    Arena T(static_cast<char *>(const_cast<void *>(tables_dev)));
    InfosBufs A;
    memset(&A, 0, sizeof(A));
    A.rows = reinterpret_cast<const float4 *>(rows_dev);
    A.frames = T.take<modest_infos_frame>(n_frames);
    A.boxes = T.take<modest_infos_box>(std::max(n_boxes, 1));
    A.wcount = const_cast<int32_t *>(wcount_dev);
    A.pass = pass_boxes;
    const dim3 grid((max_n + IK_WG_PTS - 1) / IK_WG_PTS, n_frames);
    infos_gather<<<grid, IK_THREADS, 0, stream>>>(A, reinterpret_cast<const long long *>(box_base_dev),
                                                  reinterpret_cast<float4 *>(out_rows_dev));
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int64_t modest_infos_table_bytes(int n_frames, int n_boxes) {
    return (int64_t)table_bytes(std::max(n_frames, 0), std::max(n_boxes, 0));
}
