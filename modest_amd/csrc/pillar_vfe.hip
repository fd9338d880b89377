// PointPillars' front end (OpenPCDet's PillarVFE.forward of pcdet/models/backbones_3d/vfe/pillar_vfe.py with ONE PFN layer --
// feature build, Linear without bias, BatchNorm1d, ReLU, max over a pillar's slots -- and PointPillarScatter.forward of
// pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py) with their backward passes, hand-written for gfx950.  Entry points
// (include/modest_hip.h, "a38"): enqueue only, no synchronise, no context, no device allocation, nothing read back, every output
// element written.
//
// A WAVEFRONT owns a run of PV_RUN consecutive pillars, lane = output channel.  Per pillar the wavefront stages the S x Cp voxel
// floats in LDS, three lanes sum the mean, the lanes compute the S x K features once (four slots at a time, 16 features wide) and
// then every lane reads a slot's features as broadcasts and runs its own channel's K products out of registers.  The (P, S, C)
// rows of the reference's linear / norm / relu never exist in memory:
//   pv_stats      pass 1 of a training forward: per channel sum x, sum x x, sum x f_k and once sum f_k, in float64, one partial
//                 per wavefront;  pv_reduce adds PV_GROUP partials each;  pv_finalize adds the groups, makes mean / invstd and
//                 updates the running buffers in place;
//   pv_apply      normalise, relu, max over ALL S slots -> out (P, C) and the winning slot (P, C) uint8 (eval: the only pass);
//   pv_backward   one pass over the WINNERS only: sum dy, sum dy xhat, sum dy f_k in float64 over the same tree;
//   pv_finalize_backward   dW, dgamma, dbeta out of those and the forward's saved sums.
// THE TREE of every float64 sum depends on P and S only: a wavefront adds its run in pillar order then slot order, a group its
// PV_GROUP wavefronts in ascending order, the finalise kernel the groups in ascending order, each from +0.0.  No float atomics;
// the same bits at every run and on every device.  Arithmetic: float32, one rounding per operation in
// the written order (-ffp-contract=off), / and sqrt correctly rounded; a float64 fma below always has an EXACT product (two
// float32 factors), so it is the product added with one rounding.
//   ps_scatter / ps_gather   the BEV canvas: 64 pillars a workgroup, their (64, C) tile through LDS so that the feature side is
//                 read or written as consecutive dwords and the canvas side with lane = pillar (neighbouring pillars are
//                 neighbouring cells).  A row whose b, z, y or x is out of range is skipped (forward) / given zeros (backward).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"

namespace {

constexpr int PV_RUN = 32;        // pillars a wavefront sums: the first seam of the tree
constexpr int PV_GROUP = 64;      // wavefront partials a group sums: the second seam at PV_RUN * PV_GROUP pillars
constexpr int PV_MAX_C = 64, PV_MAX_K = 16, PV_MAX_S = 255, PV_MAX_BATCH = 65535;
constexpr int PV_FROW = 16;       // floats of a slot's feature row in LDS
constexpr int64_t PV_MAX_ROWS = 2147483647LL;
constexpr int PV_ABS = 1, PV_CLUSTER = 2, PV_CENTER = 4, PV_DIST = 8;      // the parts of a feature row
constexpr int PV_APPLY_RUN = 8;   // pillars a wavefront of pv_apply walks: no sum crosses pillars there, so more wavefronts
constexpr int PS_TILE = 64;       // pillars a scatter workgroup moves

enum { KIND_NONE = 0, KIND_RAW = 1, KIND_CLUSTER = 2, KIND_CENTER = 3, KIND_DIST = 4 };

struct PillarParams {
    int64_t P;
    int S, Cp, C, K, parts, num_code, coord_code;      // codes: 0 float32, 1 int32, 2 int64
    const float *voxels;
    const void *num, *coords;
    float vx, vy, vz, xoff, yoff, zoff;
    const float *W;                 // (C, K)
};

__device__ __forceinline__ float value_f32(const void *base, int code, int64_t i) {
    if (code == 0) return static_cast<const float *>(base)[i];
    if (code == 1) return (float)static_cast<const int32_t *>(base)[i];
    return (float)static_cast<const int64_t *>(base)[i];
}

__device__ __forceinline__ int value_int(const void *base, int code, int64_t i) {      // torch's .int()
    if (code == 0) return (int)static_cast<const float *>(base)[i];
    if (code == 1) return static_cast<const int32_t *>(base)[i];
    return (int)static_cast<const int64_t *>(base)[i];
}

// what feature k is: its kind and the voxel column it reads
__device__ __forceinline__ void feature_of(const PillarParams &q, int k, int &kind, int &j) {
    kind = KIND_NONE; j = 0;
    const int raw = (q.parts & PV_ABS) ? q.Cp : q.Cp - 3;
    if (k < raw) { kind = KIND_RAW; j = (q.parts & PV_ABS) ? k : k + 3; return; }
    k -= raw;
    if (q.parts & PV_CLUSTER) { if (k < 3) { kind = KIND_CLUSTER; j = k; return; } k -= 3; }
    if (q.parts & PV_CENTER) { if (k < 3) { kind = KIND_CENTER; j = k; return; } k -= 3; }
    if ((q.parts & PV_DIST) && k == 0) kind = KIND_DIST;
}

// What a wavefront loads of a pillar one pillar ahead, so that no memory latency stands between two pillars: the first
// 64 * PV_AHEAD voxel floats (a lane's share), the count and the lane's centre coordinate.
constexpr int PV_AHEAD = 4;
struct Ahead {
    float v[PV_AHEAD], numf, coord;
    int numi;
};

__device__ __forceinline__ void fetch_pillar(const PillarParams &q, int64_t p, int kind, int j, Ahead &a) {
    const int lane = threadIdx.x;
    const int n = q.S * q.Cp;
    const float *v = q.voxels + p * (int64_t)n;
#pragma unroll
    for (int t = 0; t < PV_AHEAD; ++t) a.v[t] = lane + 64 * t < n ? v[lane + 64 * t] : 0.f;
    a.numf = value_f32(q.num, q.num_code, p);
    a.numi = value_int(q.num, q.num_code, p);
    a.coord = kind == KIND_CENTER ? value_f32(q.coords, q.coord_code, p * 4 + (3 - j)) : 0.f;
}

// The S x K masked features of pillar p into sf (rows of PV_FROW floats), by the whole wavefront.  sv: S * Cp floats, sm: 3.
// `a` holds what fetch_pillar loaded of p; it is refilled with pillar `next` (next < 0: none) as soon as it is spent.
__device__ __forceinline__ void stage_pillar(const PillarParams &q, int64_t p, int64_t next, int kind, int j, Ahead &a, float *sf,
                                             float *sv, float *sm) {
    const int lane = threadIdx.x;
    const int n = q.S * q.Cp;
    const float *v = q.voxels + p * (int64_t)n;
    __syncthreads();                                   // the pillar before is read to its end
#pragma unroll
    for (int t = 0; t < PV_AHEAD; ++t)
        if (lane + 64 * t < n) sv[lane + 64 * t] = a.v[t];
    for (int i = lane + 64 * PV_AHEAD; i < n; i += 64) sv[i] = v[i];
    const float numf = a.numf, coord = a.coord;
    const int numi = a.numi;
    if (next >= 0) fetch_pillar(q, next, kind, j, a);
    __syncthreads();
    if (lane < 3) {
        float sum = sv[lane];
#pragma unroll 8
        for (int s = 1; s < q.S; ++s) sum = sum + sv[s * q.Cp + lane];
        sm[lane] = sum / numf;
    }
    __syncthreads();
    float sub = 0.f;
    if (kind == KIND_CLUSTER) sub = sm[j];
    if (kind == KIND_CENTER) sub = coord * (j == 0 ? q.vx : j == 1 ? q.vy : q.vz) + (j == 0 ? q.xoff : j == 1 ? q.yoff : q.zoff);
    const int k = lane & 15;
    if (kind != KIND_NONE) {
        for (int s = lane >> 4; s < q.S; s += 4) {
            const float *r = sv + s * q.Cp;
            float f = r[j];
            if (q.parts & PV_DIST) {                   // the same for every lane: no square root where no lane wants one
                if (kind == KIND_DIST) f = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
            }
            if (kind == KIND_CLUSTER || kind == KIND_CENTER) f = f - sub;
            sf[s * PV_FROW + k] = f * (numi > s ? 1.f : 0.f);
        }
    }
    __syncthreads();
}

// a slot's features, as four broadcast reads of 16 bytes (only the groups below K are read)
template <int K>
__device__ __forceinline__ void read_row(const float *row, float (&f)[PV_MAX_K]) {
    const float4 *r = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * g < K) t = r[g];
        f[4 * g] = t.x; f[4 * g + 1] = t.y; f[4 * g + 2] = t.z; f[4 * g + 3] = t.w;
    }
}

// x = f_0 w_0, then + f_k w_k for k = 1 .. K - 1, each product and each sum rounded
template <int K>
__device__ __forceinline__ float linear_of(const float (&f)[PV_MAX_K], const float (&w)[PV_MAX_K]) {
    float x = f[0] * w[0];
#pragma unroll
    for (int k = 1; k < PV_MAX_K; ++k)
        if (k < K) x = x + f[k] * w[k];
    return x;
}

__device__ __forceinline__ void load_weights(const PillarParams &q, int c, float (&w)[PV_MAX_K]) {
#pragma unroll
    for (int k = 0; k < PV_MAX_K; ++k) w[k] = (c < q.C && k < q.K) ? q.W[c * q.K + k] : 0.f;
}

// Layout of the forward sums (Q = 2 C + K C + K doubles): sum x [C], sum x x [C], sum x f_k [K][C], sum f_k [K]
template <int K>
__global__ __launch_bounds__(64) void pv_stats(PillarParams q, double *partials) {
    extern __shared__ float lds[];
    float *sf = lds, *sv = sf + q.S * PV_FROW, *sm = sv + q.S * q.Cp;
    const int c = threadIdx.x;
    float w[PV_MAX_K], f[PV_MAX_K];
    load_weights(q, c, w);
    int kind, j;
    feature_of(q, c & 15, kind, j);
    double sx = 0.0, sxx = 0.0, sfk = 0.0, sxf[PV_MAX_K];
#pragma unroll
    for (int k = 0; k < PV_MAX_K; ++k) sxf[k] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.x * PV_RUN;
    const int64_t p1 = p0 + PV_RUN < q.P ? p0 + PV_RUN : q.P;
    Ahead ahead;
    if (p0 < p1) fetch_pillar(q, p0, kind, j, ahead);
    for (int64_t p = p0; p < p1; ++p) {
        stage_pillar(q, p, p + 1 < p1 ? p + 1 : -1, kind, j, ahead, sf, sv, sm);
#pragma unroll 2
        for (int s = 0; s < q.S; ++s) {                 // two slots in flight: their reads and products are independent
            read_row<K>(sf + s * PV_FROW, f);
            const double xd = (double)linear_of<K>(f, w);
            sx = sx + xd;
            sxx = fma(xd, xd, sxx);
#pragma unroll
            for (int k = 0; k < PV_MAX_K; ++k)
                if (k < K) sxf[k] = fma(xd, (double)f[k], sxf[k]);
            if (c < q.K) sfk = sfk + (double)sf[s * PV_FROW + c];
        }
    }
    const int Q = 2 * q.C + q.K * q.C + q.K;
    double *out = partials + (int64_t)blockIdx.x * Q;
    if (c < q.C) {
        out[c] = sx;
        out[q.C + c] = sxx;
#pragma unroll
        for (int k = 0; k < PV_MAX_K; ++k)
            if (k < K) out[2 * q.C + k * q.C + c] = sxf[k];
    }
    if (c < q.K) out[2 * q.C + q.K * q.C + c] = sfk;
}

// out[g][q] = in[g PV_GROUP][q] + .. in ascending order from +0.0
__global__ __launch_bounds__(256) void pv_reduce(const double *__restrict__ in, int64_t n_in, int Q, double *__restrict__ out) {
    const int64_t g = blockIdx.x;
    const int64_t first = g * PV_GROUP;
    const int count = (int)(n_in - first < PV_GROUP ? n_in - first : PV_GROUP);
    for (int i = threadIdx.x; i < Q; i += 256) {
        double acc = 0.0;
#pragma unroll 8
        for (int r = 0; r < count; ++r) acc = acc + in[(first + r) * Q + i];      // the loads of eight rows in flight
        out[g * Q + i] = acc;
    }
}

__device__ __forceinline__ double keep_positive(double t) { return (t > 0.0 || t != t) ? t : 0.0; }      // max(t, 0), a NaN kept

struct FinalizeParams {
    const double *groups;
    int64_t n_groups;
    int C, K;
    double n_rows, eps, momentum;          // momentum < 0: the cumulative average 1 / num_batches_tracked
    double *sums;                          // Q
    float *stat;                           // mean32 [C], invstd32 [C]
    float *running_mean, *running_var;     // may be NULL
    int64_t *tracked;                      // may be NULL
};

// a workgroup per 256 sums; the first holds sum x and sum x x of every channel (2 C <= 128) and makes the statistics of them
__global__ __launch_bounds__(256) void pv_finalize(FinalizeParams q) {
    __shared__ double total[256];          // a barrier does not wait for global stores: the totals are handed on in LDS
    const int Q = 2 * q.C + q.K * q.C + q.K;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Q) {
        double acc = 0.0;
#pragma unroll 8
        for (int64_t g = 0; g < q.n_groups; ++g) acc = acc + q.groups[g * Q + i];
        q.sums[i] = total[threadIdx.x] = acc;
    }
    if (blockIdx.x != 0) return;
    __syncthreads();
    const int c = threadIdx.x;
    if (c < q.C) {
        const double sx = total[c], sxx = total[q.C + c];
        const double mean = sx / q.n_rows;
        const double var = keep_positive(sxx / q.n_rows - mean * mean);
        const double invstd = 1.0 / sqrt(var + q.eps);
        q.stat[c] = (float)mean;
        q.stat[q.C + c] = (float)invstd;
        if (q.running_mean) {
            double m = q.momentum;
            if (m < 0.0) m = 1.0 / (double)(q.tracked ? *q.tracked + 1 : 1);
            const double unbiased = var * q.n_rows / (q.n_rows - 1.0);
            q.running_mean[c] = (float)((1.0 - m) * (double)q.running_mean[c] + m * mean);
            q.running_var[c] = (float)((1.0 - m) * (double)q.running_var[c] + m * unbiased);
        }
    }
    __syncthreads();                       // every lane has read the count before it moves
    if (threadIdx.x == 0 && q.tracked) *q.tracked = *q.tracked + 1;
}

struct ApplyParams {
    const float *gamma, *beta;
    const float *stat;                     // training: mean32 [C], invstd32 [C]
    const float *running_mean, *running_var;      // eval (stat NULL)
    double eps;
    float *out;
    uint8_t *winner;                       // may be NULL
};

__device__ __forceinline__ void norm_of(const ApplyParams &a, int c, int C, float &mean, float &invstd) {
    mean = 0.f; invstd = 0.f;
    if (c >= C) return;
    if (a.stat) { mean = a.stat[c]; invstd = a.stat[C + c]; }
    else { mean = a.running_mean[c]; invstd = (float)(1.0 / sqrt((double)a.running_var[c] + a.eps)); }
}

template <int K>
__global__ __launch_bounds__(64) void pv_apply(PillarParams q, ApplyParams a) {
    extern __shared__ float lds[];
    float *sf = lds, *sv = sf + q.S * PV_FROW, *sm = sv + q.S * q.Cp;
    const int c = threadIdx.x;
    float w[PV_MAX_K], f[PV_MAX_K];
    load_weights(q, c, w);
    int kind, j;
    feature_of(q, c & 15, kind, j);
    float mean, invstd;
    norm_of(a, c, q.C, mean, invstd);
    const float gamma = c < q.C ? a.gamma[c] : 0.f, beta = c < q.C ? a.beta[c] : 0.f;
    const int64_t p0 = (int64_t)blockIdx.x * PV_APPLY_RUN;
    const int64_t p1 = p0 + PV_APPLY_RUN < q.P ? p0 + PV_APPLY_RUN : q.P;
    Ahead ahead;
    if (p0 < p1) fetch_pillar(q, p0, kind, j, ahead);
    for (int64_t p = p0; p < p1; ++p) {
        stage_pillar(q, p, p + 1 < p1 ? p + 1 : -1, kind, j, ahead, sf, sv, sm);
        float best = 0.f;
        int win = 0;
#pragma unroll 4
        for (int s = 0; s < q.S; ++s) {
            read_row<K>(sf + s * PV_FROW, f);
            const float xhat = (linear_of<K>(f, w) - mean) * invstd;
            const float t = xhat * gamma + beta;
            const float y = (t > 0.f || t != t) ? t : 0.f;                    // relu, a NaN kept
            // the first slot of the maximum wins; the first NaN wins and stays
            if (s == 0 || (best == best && (y > best || y != y))) { best = y; win = s; }
        }
        if (c < q.C) {
            a.out[p * q.C + c] = best;
            if (a.winner) a.winner[p * q.C + c] = (uint8_t)win;
        }
    }
}

struct BackwardParams {
    const float *stat, *out, *grad;
    const uint8_t *winner;
};

// Layout of the backward sums (QB = 2 C + K C doubles): sum dy [C], sum dy xhat [C], sum dy f_k [K][C]
template <int K>
__global__ __launch_bounds__(64) void pv_backward(PillarParams q, BackwardParams b, double *partials) {
    extern __shared__ float lds[];
    float *sf = lds, *sv = sf + q.S * PV_FROW, *sm = sv + q.S * q.Cp;
    const int c = threadIdx.x;
    float w[PV_MAX_K], f[PV_MAX_K];
    load_weights(q, c, w);
    int kind, j;
    feature_of(q, c & 15, kind, j);
    const float mean = c < q.C ? b.stat[c] : 0.f, invstd = c < q.C ? b.stat[q.C + c] : 0.f;
    double sdy = 0.0, sdx = 0.0, sdf[PV_MAX_K];
#pragma unroll
    for (int k = 0; k < PV_MAX_K; ++k) sdf[k] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.x * PV_RUN;
    const int64_t p1 = p0 + PV_RUN < q.P ? p0 + PV_RUN : q.P;
    Ahead ahead;
    if (p0 < p1) fetch_pillar(q, p0, kind, j, ahead);
    for (int64_t p = p0; p < p1; ++p) {
        stage_pillar(q, p, p + 1 < p1 ? p + 1 : -1, kind, j, ahead, sf, sv, sm);
        if (c < q.C) {
            int s = b.winner[p * q.C + c];
            if (s >= q.S) s = q.S - 1;                                       // a winner the forward never wrote stays inside LDS
            read_row<K>(sf + s * PV_FROW, f);
            const float xhat = (linear_of<K>(f, w) - mean) * invstd;
            const float dy = b.out[p * q.C + c] > 0.f ? b.grad[p * q.C + c] : 0.f;
            const double dyd = (double)dy;
            sdy = sdy + dyd;
            sdx = fma(dyd, (double)xhat, sdx);
#pragma unroll
            for (int k = 0; k < PV_MAX_K; ++k)
                if (k < K) sdf[k] = fma(dyd, (double)f[k], sdf[k]);
        }
    }
    const int QB = 2 * q.C + q.K * q.C;
    double *out = partials + (int64_t)blockIdx.x * QB;
    if (c < q.C) {
        out[c] = sdy;
        out[q.C + c] = sdx;
#pragma unroll
        for (int k = 0; k < PV_MAX_K; ++k)
            if (k < K) out[2 * q.C + k * q.C + c] = sdf[k];
    }
}

struct FinalizeBackwardParams {
    const double *groups;
    int64_t n_groups;
    int C, K;
    double n_rows;
    const double *sums;                    // the forward's
    const float *stat, *gamma;
    float *dW, *dgamma, *dbeta;
};

// a lane per element of dW: it adds its own three sums over the groups (sum dy and sum dy xhat of a channel are added by each
// of the channel's K lanes, in the same order, to the same bits)
__global__ __launch_bounds__(256) void pv_finalize_backward(FinalizeBackwardParams q) {
    const int QB = 2 * q.C + q.K * q.C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.C * q.K) return;
    const int c = i / q.K, k = i % q.K;
    double db = 0.0, dg = 0.0, a = 0.0;
#pragma unroll 4
    for (int64_t g = 0; g < q.n_groups; ++g) {
        const double *row = q.groups + g * QB;
        db = db + row[c];
        dg = dg + row[q.C + c];
        a = a + row[2 * q.C + k * q.C + c];
    }
    const double *sxf = q.sums + 2 * q.C, *sf = q.sums + 2 * q.C + q.K * q.C;
    const double g = (double)q.gamma[c], mean = (double)q.stat[c], invstd = (double)q.stat[q.C + c];
    const double t1 = g * a;
    const double t2 = ((g * db) / q.n_rows) * sf[k];
    const double t3 = (((g * dg) / q.n_rows) * invstd) * (sxf[k * q.C + c] - mean * sf[k]);
    q.dW[i] = (float)(invstd * ((t1 - t2) - t3));
    if (k == 0) {
        q.dbeta[c] = (float)db;
        q.dgamma[c] = (float)dg;
    }
}

struct ScatterParams {
    int64_t P, plane;                      // plane = ny nx
    int C, B, ny, nx, coord_code;
    const void *coords;
};

// the cell of pillar p as an element offset of channel 0 in a (B, C, ny, nx) canvas, or -1 for a row out of range
__device__ __forceinline__ int64_t cell_of(const ScatterParams &q, int64_t p) {
    int64_t v[4];
    const int hi[4] = {q.B, 1, q.ny, q.nx};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (q.coord_code == 0) {
            const float t = static_cast<const float *>(q.coords)[p * 4 + i];
            ok = ok && t >= 0.f && t < (float)hi[i];
            v[i] = ok ? (int64_t)t : 0;
        } else {
            v[i] = q.coord_code == 1 ? (int64_t)static_cast<const int32_t *>(q.coords)[p * 4 + i]
                                     : static_cast<const int64_t *>(q.coords)[p * 4 + i];
            ok = ok && v[i] >= 0 && v[i] < hi[i];
        }
    }
    if (!ok) return -1;
    return v[0] * q.C * q.plane + (v[1] + v[2] * q.nx + v[3]);
}

template <bool GATHER>
__global__ __launch_bounds__(256) void ps_move(ScatterParams q, const float *src, float *dst) {
    __shared__ float tile[PS_TILE * (PV_MAX_C + 1)];
    __shared__ int64_t cell[PS_TILE];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PS_TILE;
    const int rows = (int)(q.P - p0 < PS_TILE ? q.P - p0 : PS_TILE);
    if (t < rows) cell[t] = cell_of(q, p0 + t);
    if (!GATHER)
        for (int i = t; i < rows * q.C; i += 256) tile[(i / q.C) * (PV_MAX_C + 1) + i % q.C] = src[p0 * q.C + i];
    __syncthreads();
    const int lane = t & 63;
    if (lane < rows) {
        const int64_t at = cell[lane];
        for (int c = t >> 6; c < q.C; c += 4) {
            if (GATHER) tile[lane * (PV_MAX_C + 1) + c] = at >= 0 ? src[at + c * q.plane] : 0.f;
            else if (at >= 0) dst[at + c * q.plane] = tile[lane * (PV_MAX_C + 1) + c];
        }
    }
    if (GATHER) {
        __syncthreads();
        for (int i = t; i < rows * q.C; i += 256) dst[p0 * q.C + i] = tile[(i / q.C) * (PV_MAX_C + 1) + i % q.C];
    }
}

// the kernels are compiled for every K = 1 .. 16: the K products of a row stay in registers, with no test and no padding
#define PV_FOR_K(K, CALL)                                                                                       \
    switch (K) {                                                                                               \
        case 1: { constexpr int KK = 1; CALL; } break;   case 2: { constexpr int KK = 2; CALL; } break;      \
        case 3: { constexpr int KK = 3; CALL; } break;   case 4: { constexpr int KK = 4; CALL; } break;      \
        case 5: { constexpr int KK = 5; CALL; } break;   case 6: { constexpr int KK = 6; CALL; } break;      \
        case 7: { constexpr int KK = 7; CALL; } break;   case 8: { constexpr int KK = 8; CALL; } break;      \
        case 9: { constexpr int KK = 9; CALL; } break;   case 10: { constexpr int KK = 10; CALL; } break;    \
        case 11: { constexpr int KK = 11; CALL; } break; case 12: { constexpr int KK = 12; CALL; } break;    \
        case 13: { constexpr int KK = 13; CALL; } break; case 14: { constexpr int KK = 14; CALL; } break;    \
        case 15: { constexpr int KK = 15; CALL; } break; default: { constexpr int KK = 16; CALL; } break;    \
    }

inline bool aligned(const void *q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

inline int features_of(int Cp, int parts) {
    return ((parts & PV_ABS) ? Cp : Cp - 3) + ((parts & PV_CLUSTER) ? 3 : 0) + ((parts & PV_CENTER) ? 3 : 0) + ((parts & PV_DIST) ? 1 : 0);
}

inline int64_t runs_of(int64_t P) { return (P + PV_RUN - 1) / PV_RUN; }
inline int64_t groups_of(int64_t P) { return (runs_of(P) + PV_GROUP - 1) / PV_GROUP; }
inline size_t lds_of(int S, int Cp) { return sizeof(float) * (size_t)(S * PV_FROW + S * Cp + 4); }

}  // namespace

extern "C" int modest_pillar_vfe_run(void) { return PV_RUN; }
extern "C" int modest_pillar_vfe_group(void) { return PV_GROUP; }

// the checks the three VFE entry points share -> the number of features, or a refusal
static int pillar_shape(int64_t P, int S, int Cp, int C, int parts, int num_code, int coord_code, int *K_out) {
    MODEST_REQUIRE(P >= 0, "n_pillars >= 0");
    MODEST_REQUIRE(S >= 1 && S <= PV_MAX_S, "slots of a pillar between 1 and 255");
    MODEST_REQUIRE(C >= 1 && C <= PV_MAX_C, "output channels between 1 and 64");
    MODEST_REQUIRE(parts >= 0 && parts < 16, "parts is a mask of 1 (xyz) 2 (cluster) 4 (centre) 8 (distance)");
    MODEST_REQUIRE(Cp >= 3 && Cp <= PV_MAX_K + 3, "point features between 3 and 19");
    const int K = features_of(Cp, parts);
    MODEST_REQUIRE(K >= 1 && K <= PV_MAX_K, "features of a point between 1 and 16");
    MODEST_REQUIRE(P <= PV_MAX_ROWS / S, "n_pillars * slots at most 2^31 - 1 rows");
    MODEST_REQUIRE(num_code >= 0 && num_code <= 2 && coord_code >= 0 && coord_code <= 2, "dtype code 0 (float32) 1 (int32) 2 (int64)");
    *K_out = K;
    return MODEST_OK;
}

extern "C" int64_t modest_pillar_vfe_workspace_bytes(int64_t n_pillars, int out_channels, int features) {
    MODEST_REQUIRE(n_pillars >= 0 && n_pillars <= PV_MAX_ROWS, "n_pillars between 0 and 2^31 - 1");
    MODEST_REQUIRE(out_channels >= 1 && out_channels <= PV_MAX_C, "output channels between 1 and 64");
    MODEST_REQUIRE(features >= 1 && features <= PV_MAX_K, "features of a point between 1 and 16");
    const int64_t Q = 2 * out_channels + features * out_channels + features;
    return (int64_t)sizeof(double) * Q * (runs_of(n_pillars) + groups_of(n_pillars));
}

static PillarParams pillar_params(int64_t P, int S, int Cp, int C, int K, int parts, const float *voxels, const void *num, int num_code,
                                  const void *coords, int coord_code, const float *geometry, const float *W) {
    PillarParams q;
    q.P = P; q.S = S; q.Cp = Cp; q.C = C; q.K = K; q.parts = parts; q.num_code = num_code; q.coord_code = coord_code;
    q.voxels = voxels; q.num = num; q.coords = coords;
    q.vx = geometry[0]; q.vy = geometry[1]; q.vz = geometry[2]; q.xoff = geometry[3]; q.yoff = geometry[4]; q.zoff = geometry[5];
    q.W = W;
    return q;
}

extern "C" int modest_pillar_vfe(int64_t n_pillars, int slots, int point_features, int out_channels, int parts,
                                 const float *voxels_dev, const void *num_points_dev, int num_code, const void *coords_dev,
                                 int coord_code, const float *geometry_host, const float *weight_dev, const float *gamma_dev,
                                 const float *beta_dev, float *running_mean_dev, float *running_var_dev,
                                 int64_t *num_batches_tracked_dev, double eps, double momentum, int training, float *out_dev,
                                 uint8_t *winner_dev, double *sums_dev, float *stat_dev, void *workspace_dev,
                                 int64_t workspace_bytes, void *stream) {
    int K = 0;
    if (int rc = pillar_shape(n_pillars, slots, point_features, out_channels, parts, num_code, coord_code, &K)) return rc;
    MODEST_REQUIRE(geometry_host, "NULL geometry");
    MODEST_REQUIRE(eps == eps && eps >= 0.0, "eps >= 0");
    const int64_t rows = n_pillars * slots;
    MODEST_REQUIRE(!training || rows >= 2, "more than one row (n_pillars * slots) in training mode");
    MODEST_REQUIRE(training || (running_mean_dev && running_var_dev), "running_mean and running_var in eval mode");
    MODEST_REQUIRE((running_mean_dev == nullptr) == (running_var_dev == nullptr), "running_mean and running_var come together");
    if (n_pillars == 0) return MODEST_OK;
    MODEST_REQUIRE(voxels_dev && num_points_dev && coords_dev && weight_dev && gamma_dev && beta_dev && out_dev, "NULL buffer");
    MODEST_REQUIRE(aligned(voxels_dev, 4) && aligned(weight_dev, 4) && aligned(gamma_dev, 4) && aligned(beta_dev, 4) &&
                   aligned(out_dev, 4) && aligned(running_mean_dev, 4) && aligned(running_var_dev, 4) && aligned(stat_dev, 4) &&
                   aligned(num_points_dev, num_code == 2 ? 8 : 4) && aligned(coords_dev, coord_code == 2 ? 8 : 4) &&
                   aligned(num_batches_tracked_dev, 8) && aligned(sums_dev, 8) && aligned(workspace_dev, 8), "unaligned buffer");
    PillarParams q = pillar_params(n_pillars, slots, point_features, out_channels, K, parts, voxels_dev, num_points_dev, num_code,
                                   coords_dev, coord_code, geometry_host, weight_dev);
    const int64_t runs = runs_of(n_pillars), groups = groups_of(n_pillars);
    const size_t lds = lds_of(slots, point_features);
    hipStream_t st = as_stream(stream);
    ApplyParams a;
    a.gamma = gamma_dev; a.beta = beta_dev; a.eps = eps; a.out = out_dev; a.winner = winner_dev;
    a.stat = nullptr; a.running_mean = running_mean_dev; a.running_var = running_var_dev;
    if (training) {
        MODEST_REQUIRE(winner_dev && sums_dev && stat_dev && workspace_dev, "NULL buffer (winner, sums, stat, workspace) in training mode");
        const int64_t need = modest_pillar_vfe_workspace_bytes(n_pillars, out_channels, K);
        MODEST_REQUIRE(workspace_bytes >= need, "workspace of modest_pillar_vfe_workspace_bytes()");
        const int Q = 2 * out_channels + K * out_channels + K;
        double *partials = static_cast<double *>(workspace_dev), *grouped = partials + runs * Q;
        PV_FOR_K(K, (pv_stats<KK><<<(unsigned)runs, 64, lds, st>>>(q, partials)));
        MODEST_HIP_CHECK(hipGetLastError());
        pv_reduce<<<(unsigned)groups, 256, 0, st>>>(partials, runs, Q, grouped);
        MODEST_HIP_CHECK(hipGetLastError());
        FinalizeParams f;
        f.groups = grouped; f.n_groups = groups; f.C = out_channels; f.K = K; f.n_rows = (double)rows; f.eps = eps;
        f.momentum = momentum; f.sums = sums_dev; f.stat = stat_dev; f.running_mean = running_mean_dev;
        f.running_var = running_var_dev; f.tracked = num_batches_tracked_dev;
        pv_finalize<<<(unsigned)((Q + 255) / 256), 256, 0, st>>>(f);
        MODEST_HIP_CHECK(hipGetLastError());
        a.stat = stat_dev; a.running_mean = nullptr; a.running_var = nullptr;
    }
    PV_FOR_K(K, (pv_apply<KK><<<(unsigned)((n_pillars + PV_APPLY_RUN - 1) / PV_APPLY_RUN), 64, lds, st>>>(q, a)));
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pillar_vfe_backward(int64_t n_pillars, int slots, int point_features, int out_channels, int parts,
                                          const float *voxels_dev, const void *num_points_dev, int num_code,
                                          const void *coords_dev, int coord_code, const float *geometry_host,
                                          const float *weight_dev, const float *gamma_dev, const float *out_dev,
                                          const uint8_t *winner_dev, const float *grad_out_dev, const double *sums_dev,
                                          const float *stat_dev, float *grad_weight_dev, float *grad_gamma_dev,
                                          float *grad_beta_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    int K = 0;
    if (int rc = pillar_shape(n_pillars, slots, point_features, out_channels, parts, num_code, coord_code, &K)) return rc;
    MODEST_REQUIRE(geometry_host, "NULL geometry");
    MODEST_REQUIRE(n_pillars * slots >= 2, "more than one row (n_pillars * slots): the forward of training mode");
    MODEST_REQUIRE(voxels_dev && num_points_dev && coords_dev && weight_dev && gamma_dev && out_dev && winner_dev && grad_out_dev &&
                   sums_dev && stat_dev && grad_weight_dev && grad_gamma_dev && grad_beta_dev && workspace_dev, "NULL buffer");
    MODEST_REQUIRE(aligned(voxels_dev, 4) && aligned(weight_dev, 4) && aligned(gamma_dev, 4) && aligned(out_dev, 4) &&
                   aligned(grad_out_dev, 4) && aligned(stat_dev, 4) && aligned(grad_weight_dev, 4) && aligned(grad_gamma_dev, 4) &&
                   aligned(grad_beta_dev, 4) && aligned(num_points_dev, num_code == 2 ? 8 : 4) &&
                   aligned(coords_dev, coord_code == 2 ? 8 : 4) && aligned(sums_dev, 8) && aligned(workspace_dev, 8), "unaligned buffer");
    const int64_t need = modest_pillar_vfe_workspace_bytes(n_pillars, out_channels, K);
    MODEST_REQUIRE(workspace_bytes >= need, "workspace of modest_pillar_vfe_workspace_bytes()");
    PillarParams q = pillar_params(n_pillars, slots, point_features, out_channels, K, parts, voxels_dev, num_points_dev, num_code,
                                   coords_dev, coord_code, geometry_host, weight_dev);
    const int64_t runs = runs_of(n_pillars), groups = groups_of(n_pillars);
    const int QB = 2 * out_channels + K * out_channels;
    double *partials = static_cast<double *>(workspace_dev), *grouped = partials + runs * QB;
    hipStream_t st = as_stream(stream);
    BackwardParams b;
    b.stat = stat_dev; b.out = out_dev; b.grad = grad_out_dev; b.winner = winner_dev;
    PV_FOR_K(K, (pv_backward<KK><<<(unsigned)runs, 64, lds_of(slots, point_features), st>>>(q, b, partials)));
    MODEST_HIP_CHECK(hipGetLastError());
    pv_reduce<<<(unsigned)groups, 256, 0, st>>>(partials, runs, QB, grouped);
    MODEST_HIP_CHECK(hipGetLastError());
    FinalizeBackwardParams f;
    f.groups = grouped; f.n_groups = groups; f.C = out_channels; f.K = K; f.n_rows = (double)(n_pillars * slots);
    f.sums = sums_dev; f.stat = stat_dev; f.gamma = gamma_dev;
    f.dW = grad_weight_dev; f.dgamma = grad_gamma_dev; f.dbeta = grad_beta_dev;
    pv_finalize_backward<<<(unsigned)((out_channels * K + 255) / 256), 256, 0, st>>>(f);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

// `rows`: the (P, C) side, `canvas`: the (B, C, ny, nx) side
static int scatter_shape(int64_t P, int C, int B, int ny, int nx, int coord_code, const void *rows, const void *coords, const void *canvas) {
    MODEST_REQUIRE(P >= 0 && P <= PV_MAX_ROWS, "n_pillars between 0 and 2^31 - 1");
    MODEST_REQUIRE(C >= 1 && C <= PV_MAX_C, "channels between 1 and 64");
    MODEST_REQUIRE(B >= 0 && B <= PV_MAX_BATCH, "batch between 0 and 65535");
    MODEST_REQUIRE(ny >= 1 && nx >= 1 && (int64_t)ny * nx <= PV_MAX_ROWS, "a grid of ny, nx >= 1 and at most 2^31 - 1 cells");
    MODEST_REQUIRE(coord_code >= 0 && coord_code <= 2, "dtype code 0 (float32) 1 (int32) 2 (int64)");
    MODEST_REQUIRE(P == 0 || (rows && coords), "NULL buffer");
    MODEST_REQUIRE(B == 0 || canvas, "NULL buffer");
    MODEST_REQUIRE(aligned(rows, 4) && aligned(canvas, 4) && aligned(coords, coord_code == 2 ? 8 : 4), "unaligned buffer");
    return MODEST_OK;
}

static ScatterParams scatter_params(int64_t P, int C, int B, int ny, int nx, const void *coords, int coord_code) {
    ScatterParams q;
    q.P = P; q.plane = (int64_t)ny * nx; q.C = C; q.B = B; q.ny = ny; q.nx = nx; q.coord_code = coord_code; q.coords = coords;
    return q;
}

extern "C" int modest_pillar_scatter(int64_t n_pillars, int channels, int batch, int ny, int nx, const float *features_dev,
                                     const void *coords_dev, int coord_code, float *canvas_dev, void *stream) {
    if (int rc = scatter_shape(n_pillars, channels, batch, ny, nx, coord_code, features_dev, coords_dev, canvas_dev)) return rc;
    if (batch == 0) return MODEST_OK;
    hipStream_t st = as_stream(stream);
    MODEST_HIP_CHECK(hipMemsetAsync(canvas_dev, 0, sizeof(float) * (size_t)batch * channels * ny * nx, st));
    if (n_pillars == 0) return MODEST_OK;
    ps_move<false><<<(unsigned)((n_pillars + PS_TILE - 1) / PS_TILE), 256, 0, st>>>(
        scatter_params(n_pillars, channels, batch, ny, nx, coords_dev, coord_code), features_dev, canvas_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_pillar_scatter_backward(int64_t n_pillars, int channels, int batch, int ny, int nx,
                                              const float *grad_canvas_dev, const void *coords_dev, int coord_code,
                                              float *grad_features_dev, void *stream) {
    if (int rc = scatter_shape(n_pillars, channels, batch, ny, nx, coord_code, grad_features_dev, coords_dev, grad_canvas_dev)) return rc;
    if (n_pillars == 0) return MODEST_OK;
    ps_move<true><<<(unsigned)((n_pillars + PS_TILE - 1) / PS_TILE), 256, 0, as_stream(stream)>>>(
        scatter_params(n_pillars, channels, batch, ny, nx, coords_dev, coord_code), grad_canvas_dev, grad_features_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
