// Stable LSD radix sort of 64-bit keys with an optional 32-bit payload, and the one-workgroup scan it is built on
// (sort64.hip).  Internal to the library: called by voxelize.hip and spconv.hip, not part of include/modest_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int SORT64_T = 256, SORT64_ITEMS = 8;        // threads of a sort workgroup, rows per thread
constexpr int SORT64_TILE = SORT64_T * SORT64_ITEMS;   // rows per sort tile; a wavefront owns 64 * SORT64_ITEMS consecutive ones
constexpr int SORT64_SCAN_T = 1024;                    // threads of the scan's one workgroup

// what a caller's workspace layout and the kernels must agree on
inline int64_t sort64_tiles(int64_t n) { return (n + SORT64_TILE - 1) / SORT64_TILE; }
inline size_t sort64_table_words(int64_t n) { return 256 * (size_t)sort64_tiles(n) + 1; }   // digit-major (digit, tile) + total
inline int sort64_result(int bits) { return ((bits + 7) / 8) & 1; }                         // passes ping-pong from buffer 0

inline int sort64_bit_length(uint64_t v) {
    int b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// Sorts n > 0 rows by the low `bits` bits of their keys, 8 bits per pass, from key[0] (and idx[0]) back and forth
// between the two buffers; idx == nullptr sorts keys only.  table: sort64_table_words(n) words.  Enqueue only; returns
// sort64_result(bits), the index of the buffer that holds the result.
int sort64(uint64_t *const key[2], uint32_t *const idx[2], int n, int bits, uint32_t *table, hipStream_t st);

// exclusive scan in place of t[0 .. entries), the total in t[entries]; one workgroup, enqueue only
void sort64_scan(uint32_t *t, int64_t entries, hipStream_t st);

// base + the number of flagged threads of this workgroup below the caller; ws: one word per wavefront.  Holds a barrier.
__device__ __forceinline__ unsigned sort64_block_rank(bool f, const uint32_t *__restrict__ base, unsigned *ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) ws[w] = __popcll(bal);
    __syncthreads();
    unsigned before = *base;
    for (int q = 0; q < w; ++q) before += ws[q];
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}
