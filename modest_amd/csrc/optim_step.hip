// a40: the optimiser step of detector training: clip_grad_norm_ and OptimWrapper.step -- the decoupled
// weight decay plus torch.optim.Adam.step -- as multi-tensor kernels over one device table of the whole parameter set.
//
// Chunks.  A chunk is OPT_CH = 4096 consecutive elements of one tensor; a tensor of n elements owns ceil(n / OPT_CH) chunks and
// the table holds no tensor without elements.  A workgroup of 256 lanes takes chunks blockIdx.x, blockIdx.x + gridDim.x, ...; the
// tensor of a chunk is found by a binary search over the tensors' first chunks (wave-uniform: scalar loads).  Lane l of pass j
// (j = 0 .. 3) owns the elements 1024 j + 4 l .. + 3 of the chunk: one 16-byte access where every pointer the kernel uses on
// that tensor is 16-byte aligned and the four elements exist, dword accesses otherwise.  Which elements a lane owns does not
// depend on the width.
//
// Grad norm.  acc_l = sum over j, then over the four elements, of (double) g * (double) g (exact products, an absent element
// adds +0.0); the 256 acc_l are summed by block_sum: inside a wavefront a[l] += a[l + s] for s = 32, 16, .., 1, then
// ((w0 + w1) + w2) + w3 over the four wavefronts.  That is the chunk's float64 partial.  The partials of the tensors that have a
// gradient, in table order, are summed by every workgroup of the consumer itself (or, with finish_launch, by the one workgroup
// of a finishing launch that leaves the coefficient for the consumer): lane l adds partials l, l + 256, ... in that order, then block_sum.  total_norm = (float) sqrt(sum).  No atomics, no
// ticket.
//
// Clip.  coef = c > 1 ? 1 : c with c = fl(fl(1 / fl(total_norm + 1e-6f)) * max_norm): a NaN stays a NaN as in torch's clamp.
//
// Step, per element, float32, no contraction:
//   p1 = p * dec;  d = g - m;  m = w < 0.5 ? m + w * d : g - d * omw;  v = (v * b2) + (omb2 * (g * g));
//   den = sqrt(v) / bc2s + eps;  p = p1 + nss * (m / den)           -- sqrt and / correctly rounded
// a tensor without a gradient this step only gets p = p * dec.  The fused kernel reads g and uses fl(g * coef) in its place.
#include "common.h"
#include <string.h>

namespace {

constexpr int OPT_CH = 4096;
constexpr int OPT_BLOCK = 256;
constexpr int OPT_PASSES = OPT_CH / (4 * OPT_BLOCK);
constexpr int OPT_GRID_CAP = 2048;          // 256 CUs x 8 workgroups, the rest is strided
constexpr int64_t OPT_MAX_TENSORS = 1 << 20;
constexpr uint32_t OPT_LERP_HIGH = 1u;

struct OptStatic {      // 40 bytes: what changes only when a parameter or a state tensor is replaced
    uint64_t p, m, v;
    int64_t n;
    int32_t first_chunk;
    int32_t pad;
};
struct OptStep {        // 48 bytes: new every step
    uint64_t g;         // 0: no gradient this step
    float dec, w, omw, b2, omb2, bc2s, eps, nss;
    uint32_t flags;
    int32_t norm_first; // the tensor's first partial among the tensors with a gradient; -1 without one
};
static_assert(sizeof(OptStatic) == 40 && sizeof(OptStep) == 48, "the table layout is part of the ABI");

struct OptLayout {
    OptStatic *st;
    OptStep *step;
    double *partials;
    float *result;      // total_norm, coef
};

__device__ __forceinline__ double block_sum(double acc, double *sh) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_down(acc, s, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double resum(const double *partials, int n, double *sh) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += OPT_BLOCK) acc += partials[i];
    return block_sum(acc, sh);
}

__device__ __forceinline__ void norm_coef(double sum, float max_norm, float &norm, float &coef) {
    norm = (float)sqrt(sum);
    const float c = (1.0f / (norm + 1e-6f)) * max_norm;
    coef = c > 1.0f ? 1.0f : c;
}

__device__ __forceinline__ int find_tensor(const OptStatic *st, int n_tensors, int c) {
    int lo = 0, hi = n_tensors - 1;      // the last tensor whose first chunk is <= c
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (st[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(uint64_t a) { return (a & 15u) == 0; }

__device__ __forceinline__ void load4(const float *a, int e, int cnt, bool wide, float x[4]) {
    if (wide && e + 3 < cnt) {
        const float4 q = *reinterpret_cast<const float4 *>(a + e);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = e + k < cnt ? a[e + k] : 0.0f;
    }
}

__device__ __forceinline__ void store4(float *a, int e, int cnt, bool wide, const float x[4]) {
    if (wide && e + 3 < cnt) {
        *reinterpret_cast<float4 *>(a + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < cnt) a[e + k] = x[k];
    }
}

// the chunk c of the table: its tensor, the offset of its first element and how many elements it has
struct Chunk {
    int t;
    int64_t base;
    int cnt;
};
__device__ __forceinline__ Chunk chunk_of(const OptStatic *st, int n_tensors, int c) {
    Chunk k;
    k.t = find_tensor(st, n_tensors, c);
    k.base = (int64_t)(c - st[k.t].first_chunk) * OPT_CH;
    const int64_t left = st[k.t].n - k.base;
    k.cnt = left < OPT_CH ? (int)left : OPT_CH;
    return k;
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_grad_norm_kernel(const OptStatic *__restrict__ st, const OptStep *__restrict__ step,
                                                                    int n_tensors, int n_chunks, double *__restrict__ partials) {
    __shared__ double sh[4];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk k = chunk_of(st, n_tensors, c);
        const uint64_t ga = step[k.t].g;
        if (ga == 0) continue;     // the same in every lane of the workgroup
        const float *g = reinterpret_cast<const float *>(ga) + k.base;
        const bool wide = aligned16(ga);
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < OPT_PASSES; ++j) {
            float x[4];
            load4(g, j * 4 * OPT_BLOCK + 4 * (int)threadIdx.x, k.cnt, wide, x);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += (double)x[q] * (double)x[q];
        }
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[step[k.t].norm_first + (c - st[k.t].first_chunk)] = s;
    }
}

// the one workgroup that finishes a norm nobody consumes in the same call
__global__ __launch_bounds__(OPT_BLOCK) void optim_norm_finish_kernel(const double *__restrict__ partials, int n_partials, float max_norm,
                                                                      float *__restrict__ result, float *__restrict__ norm_out) {
    __shared__ double sh[4];
    float norm, coef;
    norm_coef(resum(partials, n_partials, sh), max_norm, norm, coef);
    if (threadIdx.x == 0) {
        result[0] = norm;
        result[1] = coef;
        *norm_out = norm;
    }
}

// How a consumer gets the coefficient.  OPT_NORM_NONE: there is none.  OPT_NORM_RESUM: every workgroup sums the partials itself and
// workgroup 0 leaves the norm.  OPT_NORM_FINISHED: the finishing launch ahead of it left norm and coef in `result`.  The same
// resum() and norm_coef() either way, so the same bits.
constexpr int OPT_NORM_NONE = 0, OPT_NORM_RESUM = 1, OPT_NORM_FINISHED = 2;

template <int NORM>
__device__ __forceinline__ float consumer_coef(const double *__restrict__ partials, int n_partials, float max_norm, float *result,
                                               float *norm_out) {
    if (NORM == OPT_NORM_NONE) return 1.0f;
    if (NORM == OPT_NORM_FINISHED) return result[1];
    __shared__ double sh[4];
    float norm, coef;
    norm_coef(resum(partials, n_partials, sh), max_norm, norm, coef);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = norm;
        result[1] = coef;
        *norm_out = norm;
    }
    return coef;
}

template <int NORM>
__global__ __launch_bounds__(OPT_BLOCK) void optim_clip_kernel(const OptStatic *__restrict__ st, const OptStep *__restrict__ step, int n_tensors,
                                                               int n_chunks, const double *__restrict__ partials, int n_partials,
                                                               float max_norm, float *result, float *norm_out) {
    const float coef = consumer_coef<NORM>(partials, n_partials, max_norm, result, norm_out);
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk k = chunk_of(st, n_tensors, c);
        const uint64_t ga = step[k.t].g;
        if (ga == 0) continue;
        float *g = reinterpret_cast<float *>(ga) + k.base;
        const bool wide = aligned16(ga);
#pragma unroll
        for (int j = 0; j < OPT_PASSES; ++j) {
            const int e = j * 4 * OPT_BLOCK + 4 * (int)threadIdx.x;
            if (e >= k.cnt) break;
            float x[4];
            load4(g, e, k.cnt, wide, x);
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = x[q] * coef;
            store4(g, e, k.cnt, wide, x);
        }
    }
}

template <int NORM>
__global__ __launch_bounds__(OPT_BLOCK) void optim_step_kernel(const OptStatic *__restrict__ st, const OptStep *__restrict__ step, int n_tensors,
                                                               int n_chunks, const double *__restrict__ partials, int n_partials,
                                                               float max_norm, float *result, float *norm_out) {
    const float coef = consumer_coef<NORM>(partials, n_partials, max_norm, result, norm_out);
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk k = chunk_of(st, n_tensors, c);
        const OptStatic ss = st[k.t];
        const OptStep sp = step[k.t];
        float *p = reinterpret_cast<float *>(ss.p) + k.base;
        if (sp.g == 0) {          // decay alone
            const bool wide = aligned16(ss.p);
#pragma unroll
            for (int j = 0; j < OPT_PASSES; ++j) {
                const int e = j * 4 * OPT_BLOCK + 4 * (int)threadIdx.x;
                if (e >= k.cnt) break;
                float x[4];
                load4(p, e, k.cnt, wide, x);
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = x[q] * sp.dec;
                store4(p, e, k.cnt, wide, x);
            }
            continue;
        }
        float *m = reinterpret_cast<float *>(ss.m) + k.base;
        float *v = reinterpret_cast<float *>(ss.v) + k.base;
        const float *g = reinterpret_cast<const float *>(sp.g) + k.base;
        const bool wide = aligned16(ss.p | ss.m | ss.v | sp.g);
        const bool high = (sp.flags & OPT_LERP_HIGH) != 0;
#pragma unroll
        for (int j = 0; j < OPT_PASSES; ++j) {
            const int e = j * 4 * OPT_BLOCK + 4 * (int)threadIdx.x;
            if (e >= k.cnt) break;
            float xp[4], xm[4], xv[4], xg[4];
            load4(p, e, k.cnt, wide, xp);
            load4(m, e, k.cnt, wide, xm);
            load4(v, e, k.cnt, wide, xv);
            load4(g, e, k.cnt, wide, xg);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float gq = NORM != OPT_NORM_NONE ? xg[q] * coef : xg[q];
                const float p1 = xp[q] * sp.dec;
                const float d = gq - xm[q];
                xm[q] = high ? gq - d * sp.omw : xm[q] + sp.w * d;
                xv[q] = (xv[q] * sp.b2) + (sp.omb2 * (gq * gq));
                const float den = sqrtf(xv[q]) / sp.bc2s + sp.eps;
                xp[q] = p1 + sp.nss * (xm[q] / den);
            }
            store4(p, e, k.cnt, wide, xp);
            store4(m, e, k.cnt, wide, xm);
            store4(v, e, k.cnt, wide, xv);
        }
    }
}

int64_t opt_workspace_bytes(int64_t n_tensors, int64_t n_chunks) {
    return (int64_t)(arena_sz((size_t)n_tensors * sizeof(OptStatic)) + arena_sz((size_t)n_tensors * sizeof(OptStep)) +
                     arena_sz((size_t)n_chunks * sizeof(double)) + 256);
}

bool opt_sizes_ok(int64_t n_tensors, int64_t n_chunks) {
    return n_tensors >= 1 && n_tensors <= OPT_MAX_TENSORS && n_chunks >= n_tensors && n_chunks <= 2147483647;
}

// Every bound the kernels rely on, checked on the host copies of the two tables; then the tables go up through the context's
// ring of pinned slots (a slot is waited for only when the host has run a whole ring ahead).  with_state: the call reads p, m, v.
int opt_prepare(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host, const void *step_host, int upload_static,
                int with_state, void *workspace_dev, int64_t workspace_bytes, hipStream_t stream, OptLayout *lay, int *n_partials) {
    MODEST_REQUIRE(ctx != nullptr, "no context");
    MODEST_REQUIRE(opt_sizes_ok(n_tensors, n_chunks), "1 <= tensors <= 2^20, tensors <= chunks <= 2^31 - 1");
    MODEST_REQUIRE(static_host != nullptr && step_host != nullptr, "the two host tables are required");
    MODEST_REQUIRE(workspace_dev != nullptr && (reinterpret_cast<uintptr_t>(workspace_dev) & 255) == 0, "a 256-byte aligned workspace");
    MODEST_REQUIRE(workspace_bytes >= opt_workspace_bytes(n_tensors, n_chunks), "workspace smaller than modest_optim_workspace_bytes");
    const OptStatic *ss = static_cast<const OptStatic *>(static_host);
    const OptStep *sp = static_cast<const OptStep *>(step_host);
    int64_t chunk = 0, part = 0;
    for (int64_t t = 0; t < n_tensors; ++t) {
        MODEST_REQUIRE(ss[t].n >= 1, "a tensor without elements in the table");
        MODEST_REQUIRE(ss[t].first_chunk == chunk, "first_chunk is not the running sum of the chunks");
        const int64_t own = (ss[t].n + OPT_CH - 1) / OPT_CH;
        chunk += own;
        MODEST_REQUIRE(chunk <= n_chunks, "more chunks than n_chunks");
        MODEST_REQUIRE((sp[t].g & 3) == 0, "a gradient that is not 4-byte aligned");
        if (with_state) {
            MODEST_REQUIRE(ss[t].p != 0 && (ss[t].p & 3) == 0, "a parameter pointer that is null or not 4-byte aligned");
            if (sp[t].g != 0)
                MODEST_REQUIRE(ss[t].m != 0 && ss[t].v != 0 && ((ss[t].m | ss[t].v) & 3) == 0,
                               "a state pointer that is null or not 4-byte aligned on a tensor with a gradient");
        }
        if (sp[t].g != 0) {
            MODEST_REQUIRE(sp[t].norm_first == part, "norm_first is not the running sum over the tensors with a gradient");
            part += own;
        } else {
            MODEST_REQUIRE(sp[t].norm_first == -1, "norm_first of a tensor without a gradient must be -1");
        }
    }
    MODEST_REQUIRE(chunk == n_chunks, "n_chunks is not the sum of the tensors' chunks");
    Arena a(static_cast<char *>(workspace_dev));
    lay->st = a.take<OptStatic>((size_t)n_tensors);
    lay->step = a.take<OptStep>((size_t)n_tensors);
    lay->partials = a.take<double>((size_t)n_chunks);
    lay->result = a.take<float>(2);
    *n_partials = (int)part;
    const size_t sb = upload_static ? (size_t)n_tensors * sizeof(OptStatic) : 0, pb = (size_t)n_tensors * sizeof(OptStep);
    void *slot = nullptr;
    int rc = modest_ctx_stage_slot(ctx, arena_sz(sb) + pb, &slot);
    if (rc != MODEST_OK) return rc;
    char *h = static_cast<char *>(slot);
    if (sb) {
        memcpy(h, ss, sb);
        MODEST_HIP_CHECK(hipMemcpyAsync(lay->st, h, sb, hipMemcpyHostToDevice, stream));
    }
    memcpy(h + arena_sz(sb), sp, pb);
    MODEST_HIP_CHECK(hipMemcpyAsync(lay->step, h + arena_sz(sb), pb, hipMemcpyHostToDevice, stream));
    return modest_ctx_stage_commit(ctx, stream);
}

int opt_grid(int64_t n_chunks) { return (int)(n_chunks < OPT_GRID_CAP ? n_chunks : OPT_GRID_CAP); }

}  // namespace

extern "C" int modest_optim_chunk(void) { return OPT_CH; }

extern "C" int64_t modest_optim_workspace_bytes(int64_t n_tensors, int64_t n_chunks) {
    if (!opt_sizes_ok(n_tensors, n_chunks)) {
        modest_set_error("modest_optim_workspace_bytes: 1 <= tensors <= 2^20 and tensors <= chunks <= 2^31 - 1 are required");
        return MODEST_ERR_ARG;
    }
    return opt_workspace_bytes(n_tensors, n_chunks);
}

extern "C" int modest_optim_grad_norm(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                                      const void *step_host, int upload_static, float *norm_out_dev, void *workspace_dev,
                                      int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(norm_out_dev != nullptr, "no output");
    OptLayout L;
    int parts = 0;
    hipStream_t s = as_stream(stream);
    int rc = opt_prepare(ctx, n_tensors, n_chunks, static_host, step_host, upload_static, 0, workspace_dev, workspace_bytes, s, &L, &parts);
    if (rc != MODEST_OK) return rc;
    optim_grad_norm_kernel<<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials);
    optim_norm_finish_kernel<<<1, OPT_BLOCK, 0, s>>>(L.partials, parts, 1.0f, L.result, norm_out_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_optim_clip(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host, const void *step_host,
                                 int upload_static, float max_norm, int finish_launch, float *norm_out_dev, void *workspace_dev,
                                 int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(norm_out_dev != nullptr, "no output");
    OptLayout L;
    int parts = 0;
    hipStream_t s = as_stream(stream);
    int rc = opt_prepare(ctx, n_tensors, n_chunks, static_host, step_host, upload_static, 0, workspace_dev, workspace_bytes, s, &L, &parts);
    if (rc != MODEST_OK) return rc;
    optim_grad_norm_kernel<<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials);
    if (finish_launch) {
        optim_norm_finish_kernel<<<1, OPT_BLOCK, 0, s>>>(L.partials, parts, max_norm, L.result, norm_out_dev);
        optim_clip_kernel<OPT_NORM_FINISHED><<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials,
                                                                                      parts, max_norm, L.result, norm_out_dev);
    } else {
        optim_clip_kernel<OPT_NORM_RESUM><<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials,
                                                                                   parts, max_norm, L.result, norm_out_dev);
    }
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_optim_step(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host, const void *step_host,
                                 int upload_static, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    OptLayout L;
    int parts = 0;
    hipStream_t s = as_stream(stream);
    int rc = opt_prepare(ctx, n_tensors, n_chunks, static_host, step_host, upload_static, 1, workspace_dev, workspace_bytes, s, &L, &parts);
    if (rc != MODEST_OK) return rc;
    optim_step_kernel<OPT_NORM_NONE><<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials, 0, 0.0f,
                                                                      L.result, L.result);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_optim_norm_step(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                                      const void *step_host, int upload_static, float max_norm, int finish_launch,
                                      float *norm_out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    MODEST_REQUIRE(norm_out_dev != nullptr, "no output");
    OptLayout L;
    int parts = 0;
    hipStream_t s = as_stream(stream);
    int rc = opt_prepare(ctx, n_tensors, n_chunks, static_host, step_host, upload_static, 1, workspace_dev, workspace_bytes, s, &L, &parts);
    if (rc != MODEST_OK) return rc;
    optim_grad_norm_kernel<<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials);
    if (finish_launch) {
        optim_norm_finish_kernel<<<1, OPT_BLOCK, 0, s>>>(L.partials, parts, max_norm, L.result, norm_out_dev);
        optim_step_kernel<OPT_NORM_FINISHED><<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials,
                                                                                      parts, max_norm, L.result, norm_out_dev);
    } else {
        optim_step_kernel<OPT_NORM_RESUM><<<opt_grid(n_chunks), OPT_BLOCK, 0, s>>>(L.st, L.step, (int)n_tensors, (int)n_chunks, L.partials,
                                                                                   parts, max_norm, L.result, norm_out_dev);
    }
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
