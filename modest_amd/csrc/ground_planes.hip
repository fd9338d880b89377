// Ground planes for detector training (data_preprocessing/RANSAC.py:9-68) for gfx950, float64 throughout.
//
// A batch of frames takes two launches and one synchronise:
//   gp_select  one workgroup per frame: the raw (n,4) float32 rows (16-byte loads), project_velo_to_rect (rect.h, the
//              bit-exact fma chain), the strict window of RANSAC.py:32-38, a stable compaction in row order (wave ballot,
//              per-chunk wave counts, ordered write) into float64 SoA candidates x, z, y; then median(y) and
//              median(|y - median|) with numpy's semantics by a 64-bit radix select over the candidates in global memory.
//   gp_trials  one workgroup per frame (or ONE workgroup walking the frames in order when the frames share a generator,
//              --global_seed): numpy's MT19937 in LDS drawn as sklearn's tracking selection consumes it, the exact float64
//              plane through each triplet, all candidates scored per trial (|y - pred| <= thr, count + sums for the R^2
//              tie-break), sklearn's sequential accept rule and _dynamic_max_trials, the refit of the consensus set
//              (centred normal equations) and the normalised plane.
// No tickets and no cross-workgroup hand-offs: every frame's work stays inside its workgroup.
#include "common.h"
#include "ransac_host.h"
#include "rect.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_WAVES = GP_THREADS / 64;
static_assert(GP_THREADS == 256, "one histogram bin per thread");
constexpr int GP_SMALL = 300;   // sklearn's sample_without_replacement permutes for 3/n > 0.01: the host mirror fits those

__device__ __forceinline__ unsigned long long d2key(double d) {   // order-preserving 64-bit key
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key2d(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

struct SelShared {
    unsigned hist[256];
    unsigned wcnt[GP_WAVES];
    unsigned bin, k;
};

// k-th smallest (0-based) of the n keys key_of(i), 8 bits per round.  A wavefront whose matching lanes all fall into
// one bin (the leading bits of a frame's ground heights) adds them with one atomic.
template <class K>
__device__ unsigned long long select_kth(K key_of, int n, unsigned k, SelShared &S) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        S.hist[tid] = 0u;   // GP_THREADS == 256 bins
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += GP_THREADS) {
            const int i = i0 + tid;
            unsigned bin = 0;
            bool act = false;
            if (i < n) {
                const unsigned long long key = key_of(i);
                act = (key & mask) == prefix;
                bin = (unsigned)(key >> shift) & 255u;
            }
            const unsigned long long am = __ballot(act);
            if (am == 0ull) continue;
            const int first = __ffsll((long long)am) - 1;
            const unsigned b0 = __shfl(bin, first);
            const unsigned long long same = __ballot(act && bin == b0);
            if (same == am) {
                if (lane == first) atomicAdd(&S.hist[b0], (unsigned)__popcll(am));
            } else if (act) {
                atomicAdd(&S.hist[bin], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {   // wavefront 0: 4 bins per lane, inclusive scan, the lane whose range holds k
            const unsigned c0 = S.hist[4 * lane], c1 = S.hist[4 * lane + 1], c2 = S.hist[4 * lane + 2], c3 = S.hist[4 * lane + 3];
            const unsigned s = c0 + c1 + c2 + c3;
            unsigned inc = s;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(inc, off);
                if (lane >= off) inc += v;
            }
            const unsigned exc = inc - s;
            if (exc <= k && k < inc) {
                unsigned r = k - exc, b = 4u * (unsigned)lane;
                if (r >= c0) {
                    r -= c0, ++b;
                    if (r >= c1) {
                        r -= c1, ++b;
                        if (r >= c2) r -= c2, ++b;
                    }
                }
                S.bin = b;
                S.k = r;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)S.bin << shift;
        mask |= 255ull << shift;
        k = S.k;
        __syncthreads();
    }
    return prefix;
}

// numpy.median: the middle element, or (a + b) / 2 of the two middle ones
template <class V>
__device__ double median_np(V val_of, int n, SelShared &S) {
    auto key_of = [&](int i) { return d2key(val_of(i)); };
    const double hi = key2d(select_kth(key_of, n, (unsigned)(n / 2), S));
    if (n & 1) return hi;
    const double lo = key2d(select_kth(key_of, n, (unsigned)(n / 2 - 1), S));
    return (lo + hi) / 2.0;
}

struct GpBufs {
    double *cx, *cz, *cy;   // candidates, SoA, at the frame's row offset
    modest_gp_result *res;
    int32_t *trip;          // optional (F, max_trials, 3)
};

__global__ __launch_bounds__(GP_THREADS) void gp_select(const float4 *__restrict__ rows, const modest_gp_frame *__restrict__ frames,
                                                        modest_gp_params P, GpBufs B) {
    __shared__ SelShared S;
    const modest_gp_frame &f = frames[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    modest::RectMats M;
#pragma unroll
    for (int q = 0; q < 12; ++q) M.v[q] = f.v2c[q];
#pragma unroll
    for (int q = 0; q < 9; ++q) M.r[q] = f.r0[q];
    const long long base = f.row_offset;
    const int n = f.n;
    const float4 *p = rows + base;
    double *cx = B.cx + base, *cz = B.cz + base, *cy = B.cy + base;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += GP_THREADS) {
        const int i = i0 + tid;
        bool ok = false;
        double o[3] = {0.0, 0.0, 0.0};
        if (i < n) {
            const float4 r = p[i];
            modest::velo_to_rect(r.x, r.y, r.z, M, o);
            ok = (o[1] > P.min_h) && (o[1] < P.max_h) && (o[2] > -10.0) && (o[2] < 70.0) && (o[0] > -20.0) && (o[0] < 20.0);
        }
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) S.wcnt[w] = (unsigned)__popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < GP_WAVES; ++q) {
            before += q < w ? (int)S.wcnt[q] : 0;
            all += (int)S.wcnt[q];
        }
        if (ok) {
            const int at = cnt + before + (int)__popcll(bal & ((1ull << lane) - 1ull));
            cx[at] = o[0];
            cz[at] = o[2];
            cy[at] = o[1];
        }
        cnt += all;
        __syncthreads();   // wcnt is rewritten by the next chunk
    }
    modest_drain_stores();   // the candidates are read back by other wavefronts of this workgroup below
    __syncthreads();
    double med = 0.0, mad = 0.0;
    if (cnt > GP_SMALL) {
        med = median_np([&](int i) { return cy[i]; }, cnt, S);
        mad = median_np([&](int i) { return fabs(cy[i] - med); }, cnt, S);
    }
    if (tid == 0) {
        modest_gp_result &R = B.res[blockIdx.x];
        R.n_cand = cnt;
        R.median = med;
        R.mad = mad;
        R.n_trials = 0;
        R.n_inliers = 0;
        R.status = MODEST_GP_HOST;
        R.plane[0] = 0.0, R.plane[1] = -1.0, R.plane[2] = 0.0, R.plane[3] = 1.65;
    }
}

// ---- trials -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mt_next(unsigned *key, int &pos) {   // one thread (ransac_host.h: Mt19937::next32)
    if (pos >= 624) {
        const unsigned U = 0x80000000u, L = 0x7fffffffu, A = 0x9908b0dfu;
        for (int kk = 0; kk < 623; ++kk) {
            const unsigned y = (key[kk] & U) | (key[kk + 1] & L);
            key[kk] = key[kk < 624 - 397 ? kk + 397 : kk - 227] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
        }
        const unsigned y = (key[623] & U) | (key[0] & L);
        key[623] = key[396] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
        pos = 0;
    }
    unsigned y = key[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

struct TrialShared {
    unsigned key[624], key0[624];
    double part[GP_WAVES][5];
    double tot[5];
    double model[3];
    int pos, pos0, stop;
};

// block-wide sums of NV doubles in a fixed order (lanes by tree, wavefronts in index order) -> T.tot
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], TrialShared &T) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q)
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NV; ++q) T.part[w][q] = v[q];
    __syncthreads();
    if (tid == 0)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double s = T.part[0][q];
            for (int u = 1; u < GP_WAVES; ++u) s += T.part[u][q];
            T.tot[q] = s;
        }
    __syncthreads();
}

// block-wide minimum and maximum (lo, hi: this thread's; on return the block's, in every thread)
__device__ __forceinline__ void block_minmax(double &lo, double &hi, TrialShared &T) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        lo = fmin(lo, __shfl_down(lo, off));
        hi = fmax(hi, __shfl_down(hi, off));
    }
    if (lane == 0) T.part[w][0] = lo, T.part[w][1] = hi;
    __syncthreads();
    lo = T.part[0][0], hi = T.part[0][1];
    for (int u = 1; u < GP_WAVES; ++u) lo = fmin(lo, T.part[u][0]), hi = fmax(hi, T.part[u][1]);
    __syncthreads();   // T.part is the next block_sums' to write
}

// exact plane y = c0 x + c1 z + b through three candidates: centred 2x2 normal equations (the host mirror states the same
// operations in the same order); false when the triplet is collinear in (x, z) (sklearn's lstsq takes the minimum norm)
__device__ bool triplet_plane(const double *cx, const double *cz, const double *cy, const int *t, double *m) {
    const double x0 = cx[t[0]], x1 = cx[t[1]], x2 = cx[t[2]];
    const double z0 = cz[t[0]], z1 = cz[t[1]], z2 = cz[t[2]];
    const double y0 = cy[t[0]], y1 = cy[t[1]], y2 = cy[t[2]];
    const double mx = (x0 + x1 + x2) / 3.0, mz = (z0 + z1 + z2) / 3.0, my = (y0 + y1 + y2) / 3.0;
    const double a0 = x0 - mx, a1 = x1 - mx, a2 = x2 - mx;
    const double b0 = z0 - mz, b1 = z1 - mz, b2 = z2 - mz;
    const double e0 = y0 - my, e1 = y1 - my, e2 = y2 - my;
    const double sxx = a0 * a0 + a1 * a1 + a2 * a2, szz = b0 * b0 + b1 * b1 + b2 * b2, sxz = a0 * b0 + a1 * b1 + a2 * b2;
    const double sxy = a0 * e0 + a1 * e1 + a2 * e2, szy = b0 * e0 + b1 * e1 + b2 * e2;
    const double det = sxx * szz - sxz * sxz;
    if (!(fabs(det) > 1e-12 * fmax(sxx * szz, 1e-300))) return false;
    m[0] = (sxy * szz - szy * sxz) / det;
    m[1] = (szy * sxx - sxy * sxz) / det;
    m[2] = my - m[0] * mx - m[1] * mz;
    return true;
}

// the prediction X @ coef + intercept as numpy's dgemv rounds it for (n,2) rows: z c1 rounded, x c0 fused onto it, the
// intercept added (tests/test_ground_planes_cpu.py pins this against numpy)
__device__ __forceinline__ double gp_pred(double x, double z, const double *m) { return fma(x, m[0], z * m[1]) + m[2]; }

// one frame's RANSAC fit; the generator is T.key / T.pos (advanced by the executed trials).  Returns the status.
__device__ int fit_frame(const double *cx, const double *cz, const double *cy, int n, double thr, const modest_gp_params &P,
                         int32_t *trip_out, modest_gp_result &R, TrialShared &T) {
    const int tid = threadIdx.x;
    __shared__ int s_trip[3];
    __shared__ double s_best[3];
    __shared__ int s_flag, s_go, s_nbest;
    if (tid == 0) {
        s_go = 1;
        s_flag = 0;
        s_nbest = 1;
    }
    double score_best = -INFINITY, limit = (double)P.max_trials;   // (thread 0's)
    int n_trials = 0;
    bool have = false;
    __syncthreads();
    while (s_go) {
        if (tid == 0) {   // sample_without_replacement(n, 3): tracking selection, randint = masked rejection
            const unsigned rng = (unsigned)n - 1u;
            unsigned mask = rng;
            mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
            int have_t = 0, pos = T.pos;
            while (have_t < 3) {
                unsigned v;
                while ((v = mt_next(T.key, pos) & mask) > rng) {
                }
                const int j = (int)v;
                bool dup = false;
                for (int q = 0; q < have_t; ++q) dup = dup || s_trip[q] == j;
                if (!dup) s_trip[have_t++] = j;
            }
            T.pos = pos;
            if (trip_out)
                for (int q = 0; q < 3; ++q) trip_out[3 * n_trials + q] = s_trip[q];
            if (!triplet_plane(cx, cz, cy, s_trip, T.model)) s_flag = MODEST_GP_HOST;
        }
        __syncthreads();
        if (s_flag) break;
        const double m[3] = {T.model[0], T.model[1], T.model[2]};
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += GP_THREADS) {
            const double y = cy[i], r = y - gp_pred(cx[i], cz[i], m);
            if (fabs(r) <= thr) {
                v[0] += 1.0;
                v[1] += r * r;
                v[2] += y;
                v[3] += y * y;
            }
        }
        block_sums<4>(v, T);
        if (tid == 0) {   // sklearn's sequential accept rule (RANSACRegressor.fit, ransac_host.h: RansacFit::finish_batch)
            ++n_trials;
            const int nk = (int)T.tot[0];
            if (nk >= s_nbest) {
                const double score = modest::ransac_r2_from_sums(nk, T.tot[1], T.tot[2], T.tot[3]);
                if (!(nk == s_nbest && score < score_best)) {
                    s_nbest = nk;
                    score_best = score;
                    have = true;
                    for (int q = 0; q < 3; ++q) s_best[q] = m[q];
                    // _dynamic_max_trials: next to an integer the quotient before the ceil is the host's libm's to round
                    const double eps = 2.220446049250313e-16;
                    const double nom = fmax(eps, 1.0 - P.stop_probability);
                    const double denom = fmax(eps, 1.0 - pow((double)nk / (double)n, 3.0));
                    if (nom != 1.0 && denom != 1.0) {
                        const double q = log(nom) / log(denom);
                        if (fabs(q) < (double)P.max_trials + 1.0 && fabs(q - rint(q)) < 1e-7 * fmax(1.0, fabs(q))) s_flag = MODEST_GP_HOST;
                    }
                    limit = fmin(limit, modest::ransac_dynamic_max_trials(nk, n, P.stop_probability));
                }
            }
            s_go = (double)n_trials < limit && !s_flag;
        }
        __syncthreads();
    }
    if (tid == 0) {
        R.n_trials = n_trials;
        if (!have && !s_flag) s_flag = MODEST_GP_NO_CONSENSUS;
    }
    __syncthreads();
    if (s_flag) return s_flag;
    // refit over the consensus set of the winner: means, then centred moments
    const double m[3] = {s_best[0], s_best[1], s_best[2]};
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, ylo = INFINITY, yhi = -INFINITY;
    for (int i = tid; i < n; i += GP_THREADS) {
        const double x = cx[i], z = cz[i], y = cy[i];
        if (fabs(y - gp_pred(x, z, m)) <= thr) {
            s1[0] += 1.0;
            s1[1] += x;
            s1[2] += z;
            s1[3] += y;
            ylo = fmin(ylo, y), yhi = fmax(yhi, y);
        }
    }
    block_sums<4>(s1, T);
    const double cnt = T.tot[0], mx = T.tot[1] / cnt, mz = T.tot[2] / cnt, my = T.tot[3] / cnt;
    __syncthreads();   // T.tot is rewritten below
    block_minmax(ylo, yhi, T);
    double s2[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += GP_THREADS) {
        const double x = cx[i], z = cz[i], y = cy[i];
        if (fabs(y - gp_pred(x, z, m)) <= thr) {
            const double a = x - mx, b = z - mz, e = y - my;
            s2[0] += a * a;
            s2[1] += a * b;
            s2[2] += b * b;
            s2[3] += a * e;
            s2[4] += b * e;
        }
    }
    block_sums<5>(s2, T);
    if (tid == 0) {
        const double sxx = T.tot[0], sxz = T.tot[1], szz = T.tot[2], sxy = T.tot[3], szy = T.tot[4];
        const double det = sxx * szz - sxz * sxz;
        R.n_inliers = (int)cnt;
        // a consensus set of ONE height has sxy = szy = 0 in exact arithmetic: its slopes are the rounding of the sums, in
        // the order they are added, and {:e} prints them, so the frame is the host's to fit and to print
        if (!(cnt >= 3.0) || !(fabs(det) > 1e-12 * fmax(sxx * szz, 1e-300)) || !(ylo < yhi)) {
            s_flag = MODEST_GP_HOST;
        } else {
            const double c0 = (sxy * szz - szy * sxz) / det;
            const double c1 = (szy * sxx - sxy * sxz) / det;
            const double b = my - c0 * mx - c1 * mz;
            const double norm = sqrt(c0 * c0 + 1.0 + c1 * c1);
            R.plane[0] = c0 / norm;
            R.plane[1] = -1.0 / norm;
            R.plane[2] = c1 / norm;
            R.plane[3] = b / norm;
        }
    }
    __syncthreads();
    return s_flag;
}

__global__ __launch_bounds__(GP_THREADS) void gp_trials(modest_gp_frame *__restrict__ frames, int F, modest_gp_params P, GpBufs B) {
    __shared__ TrialShared T;
    const int tid = threadIdx.x;
    const int f0 = P.chain ? 0 : (int)blockIdx.x, f1 = P.chain ? F : f0 + 1;
    for (int i = tid; i < 624; i += GP_THREADS) T.key[i] = frames[f0].key[i];
    if (tid == 0) {
        T.pos = frames[f0].pos;
        T.stop = 0;
    }
    __syncthreads();
    for (int f = f0; f < f1; ++f) {
        modest_gp_frame &fr = frames[f];
        modest_gp_result &R = B.res[f];
        const int n = R.n_cand;
        if (T.stop) continue;   // (chain) a frame before this one went to the host: status stays MODEST_GP_HOST
        int st;
        if (n < 5) {
            st = MODEST_GP_DEFAULT;
        } else if (n <= GP_SMALL) {
            st = MODEST_GP_HOST;
        } else {
            for (int i = tid; i < 624; i += GP_THREADS) T.key0[i] = T.key[i];
            if (tid == 0) T.pos0 = T.pos;
            __syncthreads();
            const long long base = fr.row_offset;
            st = fit_frame(B.cx + base, B.cz + base, B.cy + base, n, R.mad, P,
                           B.trip ? B.trip + (size_t)f * P.max_trials * 3 : nullptr, R, T);
            if (st == MODEST_GP_HOST) {   // the generator goes back untouched
                for (int i = tid; i < 624; i += GP_THREADS) T.key[i] = T.key0[i];
                if (tid == 0) T.pos = T.pos0;
            }
        }
        __syncthreads();
        for (int i = tid; i < 624; i += GP_THREADS) fr.key[i] = T.key[i];
        if (tid == 0) {
            fr.pos = T.pos;
            R.status = st;
            if (st == MODEST_GP_DEFAULT) {
                R.plane[0] = 0.0, R.plane[1] = -1.0, R.plane[2] = 0.0, R.plane[3] = 1.65;
            }
            if (st == MODEST_GP_HOST) T.stop = P.chain;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int modest_ground_planes(modest_ctx *ctx, const float *rows_dev, modest_gp_frame *frames_host, int n_frames,
                                    const modest_gp_params *params_host, modest_gp_result *results_host, int32_t *triplets_host,
                                    float *gpu_ms_host, void *stream_) {
    MODEST_REQUIRE(ctx != nullptr && frames_host && params_host && results_host, "NULL argument");
    MODEST_REQUIRE(n_frames >= 0 && n_frames <= 65535, "bad n_frames");
    const modest_gp_params P = *params_host;
    MODEST_REQUIRE(P.max_trials >= 1 && P.max_trials <= 4096 && (P.chain == 0 || P.chain == 1), "bad params");
    if (gpu_ms_host) *gpu_ms_host = 0.f;
    if (n_frames == 0) return MODEST_OK;
    long long rows = 0;
    for (int f = 0; f < n_frames; ++f) {
        const modest_gp_frame &fr = frames_host[f];
        MODEST_REQUIRE(fr.n >= 0 && fr.row_offset >= 0, "bad frame rows");
        MODEST_REQUIRE(fr.pos >= 0 && fr.pos <= 624, "bad generator position");
        rows = std::max(rows, (long long)fr.row_offset + fr.n);
    }
    MODEST_REQUIRE(rows == 0 || rows_dev, "NULL rows");
    MODEST_REQUIRE((reinterpret_cast<uintptr_t>(rows_dev) & 15u) == 0, "rows must be 16-byte aligned");
    hipStream_t stream = as_stream(stream_);
    MODEST_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t b_fr = arena_sz(sizeof(modest_gp_frame) * n_frames), b_res = arena_sz(sizeof(modest_gp_result) * n_frames);
    const size_t b_trip = triplets_host ? arena_sz(sizeof(int32_t) * 3 * (size_t)P.max_trials * n_frames) : 0;
    const size_t b_c = arena_sz(sizeof(double) * (size_t)std::max(rows, 1LL));
    int rc = modest_ctx_reserve(ctx, b_fr + b_res + b_trip + 3 * b_c);
    if (rc) return rc;
    rc = modest_ctx_reserve_pinned(ctx, b_fr + b_res + b_trip);
    if (rc) return rc;
    Arena A(ctx->scratch);
    modest_gp_frame *d_fr = A.take<modest_gp_frame>(n_frames);
    GpBufs B;
    B.res = A.take<modest_gp_result>(n_frames);
    B.trip = triplets_host ? A.take<int32_t>(3 * (size_t)P.max_trials * n_frames) : nullptr;
    B.cx = A.take<double>((size_t)std::max(rows, 1LL));
    B.cz = A.take<double>((size_t)std::max(rows, 1LL));
    B.cy = A.take<double>((size_t)std::max(rows, 1LL));
    char *h = ctx->pinned;
    memcpy(h, frames_host, sizeof(modest_gp_frame) * n_frames);
    MODEST_HIP_CHECK(hipMemcpyAsync(d_fr, h, sizeof(modest_gp_frame) * n_frames, hipMemcpyHostToDevice, stream));
    if (B.trip) MODEST_HIP_CHECK(hipMemsetAsync(B.trip, 0xff, b_trip, stream));
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (gpu_ms_host) {
        MODEST_HIP_CHECK(hipEventCreate(&ev[0]));
        MODEST_HIP_CHECK(hipEventCreate(&ev[1]));
        MODEST_HIP_CHECK(hipEventRecord(ev[0], stream));
    }
    gp_select<<<n_frames, GP_THREADS, 0, stream>>>(reinterpret_cast<const float4 *>(rows_dev), d_fr, P, B);
    MODEST_HIP_CHECK(hipGetLastError());
    gp_trials<<<P.chain ? 1 : n_frames, GP_THREADS, 0, stream>>>(d_fr, n_frames, P, B);
    MODEST_HIP_CHECK(hipGetLastError());
    if (gpu_ms_host) MODEST_HIP_CHECK(hipEventRecord(ev[1], stream));
    MODEST_HIP_CHECK(hipMemcpyAsync(h, d_fr, sizeof(modest_gp_frame) * n_frames, hipMemcpyDeviceToHost, stream));
    MODEST_HIP_CHECK(hipMemcpyAsync(h + b_fr, B.res, sizeof(modest_gp_result) * n_frames, hipMemcpyDeviceToHost, stream));
    if (B.trip) MODEST_HIP_CHECK(hipMemcpyAsync(h + b_fr + b_res, B.trip, b_trip, hipMemcpyDeviceToHost, stream));
    MODEST_HIP_CHECK(hipStreamSynchronize(stream));
    if (gpu_ms_host) {
        MODEST_HIP_CHECK(hipEventElapsedTime(gpu_ms_host, ev[0], ev[1]));
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    memcpy(frames_host, h, sizeof(modest_gp_frame) * n_frames);
    memcpy(results_host, h + b_fr, sizeof(modest_gp_result) * n_frames);
    if (triplets_host) memcpy(triplets_host, h + b_fr + b_res, sizeof(int32_t) * 3 * (size_t)P.max_trials * n_frames);
    return MODEST_OK;
}

