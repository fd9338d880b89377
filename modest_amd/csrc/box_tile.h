// A workgroup's tile of consecutive rows, moved between global memory and LDS as consecutive dwords per lane (DESIGN.md
// section 7s).  A row of a box tensor is 7 to 16 floats, so a lane per row with row-strided accesses would touch every cache
// line of the tile once per column; here lane t moves dwords t, t + 256, ... of the tile (16 bytes at a time where the tile's
// base is 16-byte aligned, with a dword tail), and the row a lane computes is read from and written to LDS.
// LDS index: dword i of the tile lies at i + i / 32, one pad dword per 32, so that the lanes of a wavefront that read column k
// of 32 consecutive rows of an even width meet 32 different banks (width 8: rows r and r + 4 are 32 dwords apart and land one
// bank further; an odd width is conflict-free with or without the pad).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace modest {
namespace tile {

constexpr int LANES = 256;         // lanes = rows of a tile
constexpr int MAX_COLS = 16;       // widest row moved through a tile

__host__ __device__ __forceinline__ int at(int i) { return i + (i >> 5); }
// LDS floats of a tile of LANES rows of `cols` columns
__host__ __device__ __forceinline__ int floats_of(int cols) { return at(LANES * cols) + 1; }

// global g[0 .. count) -> LDS tile s; count <= LANES * MAX_COLS
__device__ __forceinline__ void load(const float *__restrict__ g, float *s, int count) {
    const int tid = threadIdx.x;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int quads = count >> 2;
        for (int q = tid; q < quads; q += LANES) {
            const float4 v = reinterpret_cast<const float4 *>(g)[q];
            const int j = at(q << 2);              // the four dwords of a quad share their pad
            s[j] = v.x; s[j + 1] = v.y; s[j + 2] = v.z; s[j + 3] = v.w;
        }
        done = quads << 2;
    }
    for (int i = done + tid; i < count; i += LANES) s[at(i)] = g[i];
}

// LDS tile s -> global g[0 .. count)
__device__ __forceinline__ void store(float *__restrict__ g, const float *s, int count) {
    const int tid = threadIdx.x;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int quads = count >> 2;
        for (int q = tid; q < quads; q += LANES) {
            const int j = at(q << 2);
            reinterpret_cast<float4 *>(g)[q] = make_float4(s[j], s[j + 1], s[j + 2], s[j + 3]);
        }
        done = quads << 2;
    }
    for (int i = done + tid; i < count; i += LANES) g[i] = s[at(i)];
}

}  // namespace tile
}  // namespace modest
