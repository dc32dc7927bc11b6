// geo_tiles.h -- the tiles of the fixed-point sweeps (geodesic.hip, reconstruct.hip): sizes, the tile grid of a volume and the
// masked word of a row.  A tile is GEO_TZ x GEO_TY x 64 voxels, one 64-bit word of the bit volume wide; the box in LDS is the
// tile with a one-voxel halo.  Contract: include/tomo_hip.h.
#pragma once
#include "tomo_common.h"

#define GEO_THREADS 256
#define GEO_TZ 8
#define GEO_TY 8
#define GEO_ROWS (GEO_TZ * GEO_TY)                 // rows of the interior
#define GEO_PER (GEO_ROWS / 4)                     // voxels per thread: 4 waves
#define GEO_HZ (GEO_TZ + 2)
#define GEO_HY (GEO_TY + 2)
#define GEO_HX 66
#define GEO_HROWS (GEO_HZ * GEO_HY)
#define GEO_BOX (GEO_HROWS * GEO_HX)
#define GEO_ROUNDS (GEO_ROWS * 64)                 // the bound of the inner loop: the interior voxels

struct GeoGrid {
    int64_t tz, ty, wx, tiles, words;
};

static int geo_grid(int nz, int ny, int nx, GeoGrid *g)
{
    if (nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    g->tz = ((int64_t)nz + GEO_TZ - 1) / GEO_TZ;
    g->ty = ((int64_t)ny + GEO_TY - 1) / GEO_TY;
    g->wx = tomo_words_per_row(nx);
    g->words = (int64_t)nz * ny * g->wx;
    if (g->words >= ((int64_t)1 << 31)) return TOMO_E_SIZE;      // then tz * ty * wx < 2^31 as well
    g->tiles = g->tz * g->ty * g->wx;
    if (g->tiles >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    return TOMO_OK;
}

// the set voxels of word w of a row, whatever the buffer holds in the tail bits
__device__ static inline u64 geo_word(const u64 *__restrict__ row, int nx, int wx, int w)
{
    const int r = nx - 64 * (wx - 1);
    const u64 tail = (w == wx - 1 && r < 64) ? ((1ull << r) - 1) : ~0ull;
    return row[w] & tail;
}
