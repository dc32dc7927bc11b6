// thin_picture.h -- the 3 x 3 x 3 neighbourhood of a voxel as a 27-bit PICTURE, bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1), cut out
// of nine row words and the side bits of their neighbouring words (thin.hip thins and counts neighbours with it, branches.hip
// splits a skeleton into regular and node voxels and finds the attachments of its branches).  A wave is one word, a lane a bit.
#pragma once
#include "geo_tiles.h"

#define THIN_CENTRE (1u << 13)

// The 27 words around word bx of row (z, y), one per lane 0 .. 26: lane 9 a + 3 b + c holds word bx + c - 1 of row
// (z + a - 1, y + b - 1), its tail bits clear, 0 outside the stack.  No __restrict__: the volume is written while it is read.
__device__ static inline u64 thin_load(const u64 *bits, int nz, int ny, int nx, int wx, int z, int y, int bx, int lane)
{
    if (lane >= 27) return 0ull;
    const int zz = z + lane / 9 - 1, yy = y + (lane / 3) % 3 - 1, ww = bx + lane % 3 - 1;
    if (zz < 0 || zz >= nz || yy < 0 || yy >= ny || ww < 0 || ww >= wx) return 0ull;
    return geo_word(bits + ((int64_t)zz * ny + yy) * wx, nx, wx, ww);
}

// the picture of bit `lane` of the middle word from the wave-uniform words of thin_load: per row of the cube the three bits
// at x - 1, x, x + 1, the outer ones from the side words at lanes 0 and 63
__device__ static inline u32 thin_picture(u64 mine, int lane)
{
    u32 pic = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const u64 l = __shfl(mine, 3 * r, 64), m = __shfl(mine, 3 * r + 1, 64), h = __shfl(mine, 3 * r + 2, 64);
        const u32 lo = lane > 0 ? (u32)(m >> (lane - 1)) & 1u : (u32)(l >> 63);
        const u32 hi = lane < 63 ? (u32)(m >> (lane + 1)) & 1u : (u32)(h & 1ull);
        pic |= (lo | (((u32)(m >> lane) & 1u) << 1) | (hi << 2)) << (3 * r);
    }
    return pic;
}
