// Stable LSD radix sort of 64-bit keys with an optional 32-bit payload on gfx950 (sort64.h), 8 bits per pass over the
// bits in use only.  Per pass: digit counts per tile (LDS counters: a count does not depend on arrival order), one
// exclusive scan of the digit-major (digit, tile) table, and a scatter whose ranks inside a tile come from ballots (the
// lanes of a 64-row sub-block that share a digit) and per-wavefront running counts -- every wavefront walks its own
// contiguous part of the tile in order.  Nothing in it depends on the order in which atomics land.
#include "sort64.h"

namespace {

constexpr int SORT64_WAVES = SORT64_T / 64;

__global__ __launch_bounds__(SORT64_T) void s64_count(const uint64_t *__restrict__ keys, int n, int shift,
                                                      uint32_t *__restrict__ table, int64_t tiles) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT64_TILE;
#pragma unroll
    for (int u = 0; u < SORT64_ITEMS; ++u) {
        const int64_t i = base + u * SORT64_T + tid;
        if (i < n) atomicAdd(&h[(unsigned)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(int64_t)tid * tiles + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__(SORT64_SCAN_T) void s64_scan(uint32_t *__restrict__ t, int64_t entries) {
    __shared__ unsigned ws[SORT64_SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned carry = 0;
    for (int64_t t0 = 0; t0 < entries; t0 += SORT64_SCAN_T) {
        const int64_t i = t0 + tid;
        const unsigned v = i < entries ? t[i] : 0u;
        unsigned inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) ws[w] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int q = 0; q < SORT64_SCAN_T / 64; ++q) {
            if (q < w) before += ws[q];
            total += ws[q];
        }
        if (i < entries) t[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) t[entries] = carry;
}

template <bool WITH_IDX>   // false: keys only, idx_in and idx_out are never touched
__global__ __launch_bounds__(SORT64_T) void s64_scatter(const uint64_t *__restrict__ keys_in,
                                                        const uint32_t *__restrict__ idx_in,
                                                        uint64_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out,
                                                        int n, int shift, const uint32_t *__restrict__ table, int64_t tiles) {
    __shared__ unsigned wh[SORT64_WAVES][256];   // running count per wavefront and digit, then the wavefront's base
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int q = 0; q < SORT64_WAVES; ++q) wh[q][tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t base = (int64_t)blockIdx.x * SORT64_TILE + (int64_t)w * (64 * SORT64_ITEMS);
    uint64_t key[SORT64_ITEMS];
    uint32_t id[SORT64_ITEMS];
    unsigned rank[SORT64_ITEMS];
#pragma unroll
    for (int u = 0; u < SORT64_ITEMS; ++u) {
        const int64_t i = base + u * 64 + lane;
        const bool valid = i < n;
        key[u] = valid ? keys_in[i] : 0ull;
        if constexpr (WITH_IDX) id[u] = valid ? idx_in[i] : 0u;
        const unsigned d = (unsigned)(key[u] >> shift) & 255u;
        unsigned long long same = __ballot(valid);   // the lanes of this sub-block with my digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(one);
            same &= one ? bal : ~bal;
        }
        // only this wavefront touches wh[w]: its lanes read before the group's first lane writes (program order)
        const unsigned prev = wh[w][d];
        rank[u] = prev + __popcll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (valid && (same & below) == 0ull) wh[w][d] = prev + __popcll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread d: where digit d of this tile starts, then of each wavefront's part
        unsigned run = table[(int64_t)tid * tiles + blockIdx.x];
#pragma unroll
        for (int q = 0; q < SORT64_WAVES; ++q) {
            const unsigned cnt = wh[q][tid];
            wh[q][tid] = run;
            run += cnt;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SORT64_ITEMS; ++u) {
        const int64_t i = base + u * 64 + lane;
        if (i < n) {
            const unsigned d = (unsigned)(key[u] >> shift) & 255u;
            const unsigned pos = wh[w][d] + rank[u];
            if (pos < (unsigned)n) {   // (always: the table counts exactly these rows)
                keys_out[pos] = key[u];
                if constexpr (WITH_IDX) idx_out[pos] = id[u];
            }
        }
    }
}

}  // namespace

void sort64_scan(uint32_t *t, int64_t entries, hipStream_t st) { s64_scan<<<1, SORT64_SCAN_T, 0, st>>>(t, entries); }

int sort64(uint64_t *const key[2], uint32_t *const idx[2], int n, int bits, uint32_t *table, hipStream_t st) {
    const int64_t tiles = sort64_tiles(n);
    for (int ps = 0; 8 * ps < bits; ++ps) {
        const int in = ps & 1, out = in ^ 1;
        s64_count<<<(unsigned)tiles, SORT64_T, 0, st>>>(key[in], n, 8 * ps, table, tiles);
        sort64_scan(table, 256 * tiles, st);
        if (idx)
            s64_scatter<true><<<(unsigned)tiles, SORT64_T, 0, st>>>(key[in], idx[in], key[out], idx[out], n, 8 * ps, table, tiles);
        else
            s64_scatter<false><<<(unsigned)tiles, SORT64_T, 0, st>>>(key[in], nullptr, key[out], nullptr, n, 8 * ps, table, tiles);
    }
    return sort64_result(bits);
}
