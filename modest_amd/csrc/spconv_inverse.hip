// Inverse sparse 3-D convolution (spconv 1.2's SparseInverseConv3d) on gfx950: what the forward of spconv.hip lacks.
// Three entry points (include/modest_hip.h, "a29"); the contract is DESIGN.md section 7k:
//   * modest_spconv_class_order_workspace_bytes / modest_spconv_class_order -- the fine rows stably ordered by class
//   * modest_spconv_gather_gemm_classes                                       -- the forward on tiles of one class
//
// An inverse convolution runs the rulebook of a strided convolution backwards: its output rows are that convolution's
// input sites, out[i] += x[o] * W[k] for every pair (i, k, o), a gather through nbr_t (K, N_in).  Fine site i is read at
// offset k only where k_j == (i_j + p_j) mod s_j (mod s_j) on every axis: the class of the row, the mixed-radix number of
// these three residues, fixes the offsets that can be present -- at most 8 of 27 for kernel 3, stride 2.  A tile of 64
// consecutive rows has every class in it and skips almost nothing; a tile of 64 rows of ONE class visits its class's
// offsets only.  The rows of a class are 64 consecutive entries of perm, the stable order by class (sort64.hip, one pass
// for up to 256 classes); class_start holds the exclusive counts.  Nothing travels to the host.
//
// Arithmetic: that of spconv.hip's gather-GEMM, accumulator by accumulator -- k ascending over the present offsets, ci
// ascending, product and sum rounded separately, + bias -- so the bits do not depend on which tile a row is in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "modest_hip.h"
#include "sort64.h"

namespace {

constexpr int64_t SPI_MAX_ROWS = 2147483647 - 4096;
constexpr int SPI_KSIZE_MAX = 7;
constexpr int SPI_CH_MAX = 128;
constexpr int SPI_STRIDE_MAX = 64;
constexpr int SPI_CLASSES_MAX = SPI_STRIDE_MAX * SPI_STRIDE_MAX * SPI_STRIDE_MAX;   // of the class order
constexpr int SPI_TILE_CLASSES_MAX = 64;                                            // of the class-tiled gather-GEMM
constexpr int SPI_TM = 64, SPI_CK = 32;                                             // the tile of spconv.hip

struct SpiGeom {
    int k[3], s[3], p[3];   // axis order z, y, x
    int kvol, classes;
};

struct SpiLayout {
    size_t key_a, key_b, idx_a, idx_b, table, bytes;
};

// a function of the rows alone (the class count only bounds the sort's passes)
inline SpiLayout spi_layout(int64_t n) {
    SpiLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += arena_sz(bytes);
        return at;
    };
    L.key_a = take(sizeof(uint64_t) * (size_t)n);
    L.key_b = take(sizeof(uint64_t) * (size_t)n);
    L.idx_a = take(sizeof(uint32_t) * (size_t)n);
    L.idx_b = take(sizeof(uint32_t) * (size_t)n);
    L.table = take(sizeof(uint32_t) * sort64_table_words(n));
    L.bytes = off;
    return L;
}

int spi_geom(const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3, SpiGeom *g) {
    MODEST_REQUIRE(stride3, "NULL geometry");
    g->kvol = 1;
    int64_t classes = 1;
    for (int j = 0; j < 3; ++j) {
        MODEST_REQUIRE(stride3[j] >= 1 && stride3[j] <= SPI_STRIDE_MAX, "stride out of range (1 .. 64)");
        g->s[j] = stride3[j];
        g->k[j] = 1;
        g->p[j] = 0;
        if (kernel3) {
            MODEST_REQUIRE(kernel3[j] >= 1 && kernel3[j] <= SPI_KSIZE_MAX, "kernel size out of range (1 .. 7)");
            g->k[j] = kernel3[j];
        }
        if (pad3) {
            MODEST_REQUIRE(pad3[j] >= 0 && pad3[j] <= 64, "padding out of range");
            g->p[j] = pad3[j];
        }
        g->kvol *= g->k[j];
        classes *= stride3[j];
    }
    g->classes = (int)classes;
    return MODEST_OK;
}

// ---------------------------------------------------------------- class order -------------------------------------------
__global__ __launch_bounds__(256) void spi_class_keys(const int32_t *__restrict__ ind, int n, SpiGeom g,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned cls = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        int r = (ind[i * 4 + 1 + j] + g.p[j]) % g.s[j];
        if (r < 0) r += g.s[j];   // (a negative coordinate: the rulebook has rejected it, the class stays in range)
        cls = cls * (unsigned)g.s[j] + (unsigned)r;
    }
    keys[i] = cls;
    idx[i] = (uint32_t)i;
}

// perm = the sorted payload; class_start[c] = the first position whose class is >= c, class_start[classes] = n.  Position
// p writes the entries of the classes in (class of p - 1, class of p]; the last one also those above its own.
__global__ __launch_bounds__(256) void spi_class_finish(const uint64_t *__restrict__ sk, const uint32_t *__restrict__ sidx,
                                                        int n, int classes, int32_t *__restrict__ perm,
                                                        int32_t *__restrict__ class_start) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    perm[p] = (int32_t)sidx[p];
    const int64_t last = classes - 1;
    int64_t cur = (int64_t)sk[p];
    if (cur > last) cur = last;
    int64_t prev = -1;
    if (p > 0) {
        prev = (int64_t)sk[p - 1];
        if (prev > last) prev = last;
    }
    for (int64_t c = prev + 1; c <= cur; ++c) class_start[c] = (int32_t)p;
    if (p == n - 1)
        for (int64_t c = cur + 1; c <= classes; ++c) class_start[c] = n;
}

// ---------------------------------------------------------------- class-tiled gather-GEMM -------------------------------
// out[perm[q]][n] for 64 consecutive q of one class.  Workgroup g walks class_start to its class and first position (the
// grid is the host's bound N / 64 + classes on the tiles; the surplus exits before any barrier).  The tile's offsets are
// k_j = r_j, r_j + s_j, ... < K_j on every axis, walked z-major: ascending k.  The rest is sp_gather_gemm's tile: a lane
// owns RPT rows x 4 columns in registers, weights and gathered rows go through LDS in chunks of 32 input channels.
template <int NP>
__global__ __launch_bounds__(256) void spi_class_gemm(const float *__restrict__ in, int n_in, int m_dim,
                                                      const float *__restrict__ w, SpiGeom g, int w_cout,
                                                      const float *__restrict__ bias, const int32_t *__restrict__ map,
                                                      int n_out, const int32_t *__restrict__ perm,
                                                      const int32_t *__restrict__ class_start, float *__restrict__ out) {
    constexpr int CG = NP / 4, RG = 256 / CG, RPT = SPI_TM / RG;
    __shared__ __attribute__((aligned(16))) float sW[SPI_CK][NP];
    __shared__ float sX[SPI_TM][SPI_CK + 1];
    __shared__ int sRow[SPI_TM];
    __shared__ int sOut[SPI_TM];
    const int tid = threadIdx.x, cg = tid % CG, rg = tid / CG, c0 = cg * 4, r0 = rg * RPT;
    const int n_dim = w_cout;
    // which class, which 64 positions: the same walk in every lane
    int cls = -1, first = 0, end = 0;
    {
        int64_t tiles = 0;
        int lo = class_start[0];
        for (int c = 0; c < g.classes; ++c) {
            const int hi = class_start[c + 1];
            const int64_t t = hi > lo ? ((int64_t)hi - lo + SPI_TM - 1) / SPI_TM : 0;
            if ((int64_t)blockIdx.x < tiles + t) {
                cls = c;
                first = lo + (int)((int64_t)blockIdx.x - tiles) * SPI_TM;
                end = hi;
                break;
            }
            tiles += t;
            lo = hi;
        }
    }
    if (cls < 0 || first < 0 || end > n_out || first >= end) return;   // a surplus workgroup (or counts that are no counts)
    int res[3], cnt[3];
    {
        int c = cls;
#pragma unroll
        for (int j = 2; j >= 0; --j) {
            res[j] = c % g.s[j];
            c /= g.s[j];
            cnt[j] = res[j] < g.k[j] ? (g.k[j] - res[j] + g.s[j] - 1) / g.s[j] : 0;
        }
    }
    if (tid < SPI_TM) {
        int o = -1;
        if (first + tid < end) o = perm[first + tid];
        if (o < 0 || o >= n_out) o = -1;
        sOut[tid] = o;
    }
    float acc[RPT][4];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
    const int visits = cnt[0] * cnt[1] * cnt[2];
    for (int v = 0; v < visits; ++v) {
        const int ax = v % cnt[2], azy = v / cnt[2], ay = azy % cnt[1], az = azy / cnt[1];
        const int k = ((res[0] + az * g.s[0]) * g.k[1] + res[1] + ay * g.s[1]) * g.k[2] + res[2] + ax * g.s[2];
        __syncthreads();   // sOut is written; the rows of the previous offset have been read
        int row = -1;
        if (tid < SPI_TM) {
            const int o = sOut[tid];
            if (o >= 0) row = map[(int64_t)k * n_out + o];
            if (row < 0 || row >= n_in) row = -1;
            sRow[tid] = row;
        }
        if (!__syncthreads_or(row >= 0)) continue;   // no row of this tile has a neighbour at k
        unsigned present = 0;
#pragma unroll
        for (int r = 0; r < RPT; ++r) present |= (sRow[r0 + r] >= 0 ? 1u : 0u) << r;
        for (int m0 = 0; m0 < m_dim; m0 += SPI_CK) {
            const int mc = m_dim - m0 < SPI_CK ? m_dim - m0 : SPI_CK;
            __syncthreads();   // the previous chunk has been consumed
            for (int e = tid; e < SPI_CK * NP; e += 256) {
                const int mm = e / NP, n = e % NP;
                sW[mm][n] = (mm < mc && n < n_dim) ? w[((int64_t)k * m_dim + m0 + mm) * w_cout + n] : 0.f;
            }
            for (int e = tid; e < SPI_TM * SPI_CK; e += 256) {
                const int r = e / SPI_CK, mm = e % SPI_CK;
                const int src = sRow[r];
                sX[r][mm] = (src >= 0 && mm < mc) ? in[(int64_t)src * m_dim + m0 + mm] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int mm = 0; mm < mc; ++mm) {
                const float4 wv = *reinterpret_cast<const float4 *>(&sW[mm][c0]);
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    if ((present >> r) & 1u) {
                        const float xv = sX[r0 + r][mm];
                        acc[r][0] = acc[r][0] + xv * wv.x;
                        acc[r][1] = acc[r][1] + xv * wv.y;
                        acc[r][2] = acc[r][2] + xv * wv.z;
                        acc[r][3] = acc[r][3] + xv * wv.w;
                    }
                }
            }
        }
    }
    __syncthreads();   // sOut is written (a class without offsets never reached the loop's barrier)
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int o = sOut[r0 + r];
        if (o >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = c0 + j;
                if (n < n_dim) out[(int64_t)o * n_dim + n] = bias ? acc[r][j] + bias[n] : acc[r][j];
            }
        }
    }
}

}  // namespace

extern "C" int64_t modest_spconv_class_order_workspace_bytes(int64_t n_rows, int n_classes) {
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= SPI_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(n_classes >= 1 && n_classes <= SPI_CLASSES_MAX, "class count out of range");
    return (int64_t)spi_layout(n_rows).bytes;
}

extern "C" int modest_spconv_class_order(const int32_t *indices_dev, int64_t n_rows, const int32_t *stride3_host,
                                         const int32_t *pad3_host, void *workspace_dev, int64_t workspace_bytes,
                                         int32_t *perm_dev, int32_t *class_start_dev, void *stream) {
    SpiGeom g;
    MODEST_REQUIRE(pad3_host, "NULL geometry");
    if (int rc = spi_geom(nullptr, stride3_host, pad3_host, &g)) return rc;
    MODEST_REQUIRE(n_rows >= 0 && n_rows <= SPI_MAX_ROWS, "row count out of range");
    MODEST_REQUIRE(class_start_dev, "NULL buffer");
    const hipStream_t st = as_stream(stream);
    if (n_rows == 0) {
        MODEST_HIP_CHECK(hipMemsetAsync(class_start_dev, 0, sizeof(int32_t) * ((size_t)g.classes + 1), st));
        return MODEST_OK;
    }
    const SpiLayout L = spi_layout(n_rows);
    MODEST_REQUIRE(indices_dev && workspace_dev && perm_dev, "NULL buffer");
    MODEST_REQUIRE(workspace_bytes >= (int64_t)L.bytes, "workspace smaller than modest_spconv_class_order_workspace_bytes");
    MODEST_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "workspace must be 256-byte aligned");
    char *ws = static_cast<char *>(workspace_dev);
    uint64_t *key[2] = {reinterpret_cast<uint64_t *>(ws + L.key_a), reinterpret_cast<uint64_t *>(ws + L.key_b)};
    uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + L.idx_a), reinterpret_cast<uint32_t *>(ws + L.idx_b)};
    uint32_t *table = reinterpret_cast<uint32_t *>(ws + L.table);
    const int n = (int)n_rows;
    const unsigned blocks = (unsigned)((n_rows + 255) / 256);
    spi_class_keys<<<blocks, 256, 0, st>>>(indices_dev, n, g, key[0], idx[0]);
    const int fin = sort64(key, idx, n, sort64_bit_length((uint64_t)(g.classes - 1)), table, st);   // one class: no pass
    spi_class_finish<<<blocks, 256, 0, st>>>(key[fin], idx[fin], n, g.classes, perm_dev, class_start_dev);
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}

extern "C" int modest_spconv_gather_gemm_classes(const float *in_dev, int64_t n_in, int in_channels, const float *weight_dev,
                                                 const int32_t *kernel3_host, const int32_t *stride3_host, int w_cout,
                                                 const float *bias_dev, const int32_t *map_dev, int64_t n_out,
                                                 const int32_t *perm_dev, const int32_t *class_start_dev, float *out_dev,
                                                 void *stream) {
    SpiGeom g;
    MODEST_REQUIRE(kernel3_host, "NULL geometry");
    if (int rc = spi_geom(kernel3_host, stride3_host, nullptr, &g)) return rc;
    MODEST_REQUIRE((int64_t)stride3_host[0] * stride3_host[1] * stride3_host[2] <= SPI_TILE_CLASSES_MAX,
                   "more than 64 classes: use modest_spconv_gather_gemm on the rows");
    MODEST_REQUIRE(in_channels >= 1 && in_channels <= SPI_CH_MAX && w_cout >= 1 && w_cout <= SPI_CH_MAX,
                   "channels out of range (1 .. 128)");
    MODEST_REQUIRE(n_in >= 0 && n_in <= SPI_MAX_ROWS && n_out >= 0 && n_out <= SPI_MAX_ROWS, "row count out of range");
    if (n_out == 0) return MODEST_OK;
    MODEST_REQUIRE(weight_dev && map_dev && perm_dev && class_start_dev && out_dev && (n_in == 0 || in_dev), "NULL buffer");
    // sum over the classes of ceil(n_c / 64) <= floor(N / 64) + classes: no count is read on the host
    const unsigned blocks = (unsigned)(n_out / SPI_TM + g.classes);
    const hipStream_t st = as_stream(stream);
#define SPI_GEMM(NP)                                                                                                         \
    spi_class_gemm<NP><<<blocks, 256, 0, st>>>(in_dev, (int)n_in, in_channels, weight_dev, g, w_cout, bias_dev, map_dev,     \
                                               (int)n_out, perm_dev, class_start_dev, out_dev)
    if (w_cout <= 16) SPI_GEMM(16);
    else if (w_cout <= 32) SPI_GEMM(32);
    else if (w_cout <= 64) SPI_GEMM(64);
    else SPI_GEMM(128);
#undef SPI_GEMM
    MODEST_HIP_CHECK(hipGetLastError());
    return MODEST_OK;
}
