// geo_tiles.h -- the tiles of the fixed-point operators (geodesic.hip, reconstruct.hip, thin.hip): sizes, the tile grid of a
// volume, the masked word of a row, and the skeleton of a tile sweep.  A tile is GEO_TZ x GEO_TY x 64 voxels, one 64-bit word of
// the bit volume wide; the box in LDS is the tile with a one-voxel halo.  Contract: include/tomo_hip.h.
//
// The skeleton of a sweep (geo_sweep_kernel, zone_sweep_kernel, recon_sweep_kernel), in the order a kernel calls it:
//   geo_enter        a workgroup whose flag in dirty_cur is clear leaves at once; otherwise it clears the flag, which only it reads
//   geo_halo_masks   the set voxels of the 100 halo rows: the word of the tile's column and the two voxels beside it
//   geo_halo_set     "is this cell of the halo box a set voxel", for the kernel's own load of its box
//   ...              the kernel's rounds against the fixed halo, and its store of the changed voxels, which collects per voxel
//   geo_marks        the neighbouring tiles next to a changed face, edge or corner voxel, one bit per (dz, dy, dx)
//   geo_leave        the marks of the workgroup meet in LDS; one that changed nothing stores nothing and marks nobody; otherwise
//                    counters[0] counts it once, it marks itself when it hit the round bound, and sets the flags of the marked
//                    tiles in dirty_next (every writer stores the same 1: no atomics).
// The LDS arrays are the kernel's own and are handed in.  Why stale reads are safe and nothing waits on another workgroup is the
// operator's argument and stands at the top of its file.  thin_pass_kernel shares the tile and the marks; it raises stamps
// where the sweeps set flags, the tile itself among them, and keeps that walk.
#pragma once
#include "tomo_common.h"
#include <math.h>

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

// one kernel in two instances, chosen by the connectivity (6 or 26, checked by the caller); workgroups of GEO_THREADS
template <auto K6, auto K26, typename... Args>
static void geo_launch(int connectivity, dim3 grid, void *stream, Args... args)
{
    if (connectivity == 6) hipLaunchKernelGGL(K6, grid, dim3(GEO_THREADS), 0, (hipStream_t)stream, args...);
    else hipLaunchKernelGGL(K26, grid, dim3(GEO_THREADS), 0, (hipStream_t)stream, args...);
}

// the set voxels of word w of a row, whatever the buffer holds in the tail bits
__device__ static inline u64 geo_word(const u64 *__restrict__ row, int nx, int wx, int w)
{
    const int r = nx - 64 * (wx - 1);
    const u64 tail = (w == wx - 1 && r < 64) ? ((1ull << r) - 1) : ~0ull;
    return row[w] & tail;
}

// ---------------------------------------------------------------------------------------------- a wave is a word
// The kernels with one thread per voxel of the padded rows: a wave is one word of a row -- word, row and w are the same for
// its 64 lanes -- and a lane is bit b of it, voxel x of the row (x may lie at or beyond nx in the last word).
struct GeoLane {
    int64_t word, row;
    int w, b, x;
};

// false: the wave lies beyond the volume and leaves
__device__ static inline bool geo_lane(int64_t nwords, int wx, GeoLane *p)
{
    const int64_t t = (int64_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    p->word = t >> 6;
    if (p->word >= nwords) return false;
    p->row = p->word / wx;
    p->w = (int)(p->word - p->row * wx);
    p->b = (int)(t & 63);
    p->x = 64 * p->w + p->b;
    return true;
}

// ---------------------------------------------------------------------------------------------- a workgroup is a tile
struct GeoTile {
    int bx, by, bz;                                // the tile in the grid: word column, tile row, tile slice
    int z0, y0;                                    // the halo box starts here: one voxel before the tile
};

__device__ static inline GeoTile geo_tile(int64_t tile, int wx, int ty)
{
    GeoTile t;
    t.bx = (int)(tile % wx);
    const int64_t rest = tile / wx;
    t.by = (int)(rest % ty);
    t.bz = (int)(rest / ty);
    t.z0 = t.bz * GEO_TZ - 1;
    t.y0 = t.by * GEO_TY - 1;
    return t;
}

// A thread owns voxel `lane` of the interior rows r = wave + 4 k: slice lz = r / TY and row ly = r % TY of the tile.  Its row of
// the halo box, and the place of the voxel in a box.  The place is formed on the pointer, the row spelled out: as an int, or
// through geo_halo_row(), zone_sweep_kernel takes up to 252 registers instead of 134 (profiles/r37_sweep_skeleton.md).
__device__ static inline int geo_halo_row(int lz, int ly) { return (lz + 1) * GEO_HY + (ly + 1); }

template <typename T>
__device__ static inline T *geo_box_at(T *box, int lz, int ly, int lane)
{
    return box + ((lz + 1) * GEO_HY + (ly + 1)) * GEO_HX + lane + 1;
}

// ... and the place of its voxel `lane` in a map of the volume
__device__ static inline int64_t geo_voxel(const GeoTile &t, int lz, int ly, int lane, int ny, int nx)
{
    return ((int64_t)(t.z0 + 1 + lz) * ny + (t.y0 + 1 + ly)) * nx + (64 * t.bx + lane);
}

// ... and of cell xx of row hr of the halo box, where that is a set voxel
__device__ static inline int64_t geo_halo_voxel(const GeoTile &t, int hr, int xx, int ny, int nx)
{
    return ((int64_t)(t.z0 + hr / GEO_HY) * ny + (t.y0 + hr % GEO_HY)) * nx + (64 * t.bx + xx - 1);
}

// false, for every thread: the tile is not due.  Every thread has read the flag before it is cleared.
__device__ static inline bool geo_enter(u32 *dirty_cur, int64_t tile, u32 *snb)
{
    if (!__syncthreads_or((int)dirty_cur[tile])) return false;
    if (threadIdx.x == 0) {
        dirty_cur[tile] = 0u;
        *snb = 0u;
    }
    return true;
}

// smid: the word of a halo row, 0 outside the stack; sside bit 0: the voxel left of the word is set, bit 1: right.  The caller
// passes a barrier before it reads them.
__device__ static inline void geo_halo_masks(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx, const GeoTile &t, u64 *smid,
                                             u32 *sside)
{
    const int tid = threadIdx.x;
    if (tid >= GEO_HROWS) return;
    const int z = t.z0 + tid / GEO_HY, y = t.y0 + tid % GEO_HY;
    u64 mid = 0;
    u32 side = 0;
    if (z >= 0 && z < nz && y >= 0 && y < ny) {
        const u64 *r = bits + ((int64_t)z * ny + y) * wx;
        mid = geo_word(r, nx, wx, t.bx);
        if (t.bx > 0 && (geo_word(r, nx, wx, t.bx - 1) >> 63)) side |= 1u;
        if (t.bx + 1 < wx && (geo_word(r, nx, wx, t.bx + 1) & 1)) side |= 2u;
    }
    smid[tid] = mid;
    sside[tid] = side;
}

// the z weights of the tile's nine slice boundaries, by threads 128 .. 163: boundary b lies between halo slices b and b + 1 and
// has four weights (z, zx, zy, zyx); +inf where a slice lies outside the stack
__device__ static inline void geo_z_weights(const float *__restrict__ wz, int nz, const GeoTile &t, float *swz)
{
    const int i = (int)threadIdx.x - 128;
    if (i < 0 || i >= (GEO_TZ + 1) * 4) return;
    const int z = t.z0 + (i >> 2);                           // the boundary between slices z and z + 1
    swz[i] = (z >= 0 && z + 1 < nz) ? wz[4 * (int64_t)z + (i & 3)] : INFINITY;
}

// cell xx of row hr of the halo box is a set voxel: it then lies inside the stack and below nx
__device__ static inline bool geo_halo_set(const u64 *smid, const u32 *sside, int hr, int xx)
{
    if (xx == 0) return sside[hr] & 1u;
    if (xx == GEO_HX - 1) return (sside[hr] >> 1) & 1u;
    return (smid[hr] >> (xx - 1)) & 1;
}

// the steps that leave the tile from place l of n along an axis; bit 0 / 1 / 2: step -1 / 0 / +1
__device__ static inline u32 geo_steps(int l, int n) { return 2u | (l == 0 ? 1u : 0u) | (l == n - 1 ? 4u : 0u); }

// the tiles reached by a step of each of the three sets: bit 9 a + 3 b + c for the steps (a - 1, b - 1, c - 1) in z, y, x.  Bit 13
// is the tile itself.  The sweeps form xs per lane, thinning per wave from its ballot.
__device__ static inline u32 geo_marks(u32 zs, u32 ys, u32 xs)
{
    u32 nb = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            if (((zs >> a) & 1) && ((ys >> b) & 1)) nb |= xs << (9 * a + 3 * b);
    return nb;
}

// the tile that bit k of geo_marks stands for, -1 where it lies outside the grid of tzn x ty x wx tiles
__device__ static inline int64_t geo_tile_beside(const GeoTile &t, int k, int tzn, int ty, int wx)
{
    const int nbz = t.bz + k / 9 - 1, nby = t.by + (k / 3) % 3 - 1, nbx = t.bx + k % 3 - 1;
    if (nbz < 0 || nbz >= tzn || nby < 0 || nby >= ty || nbx < 0 || nbx >= wx) return -1;
    return ((int64_t)nbz * ty + nby) * wx + nbx;
}

// nb: the marks of the thread's changed voxels; more: the last round still changed something, so the round bound was hit.
// Under CONN == 6 a change reaches another tile through a face only.
template <int CONN>
__device__ static inline void geo_leave(u32 nb, int more, u32 *snb, int64_t tile, const GeoTile &t, int nz, int ty, int wx,
                                        u32 *dirty_next, unsigned long long *counters)
{
    const int tid = threadIdx.x;
    if (nb) atomicOr(snb, nb);                               // an LDS atomic
    __syncthreads();
    const u32 all = *snb;
    if (!(all || more)) return;                              // nothing changed: nothing is stored, nothing is marked
    if (tid == 0) {
        atomicAdd(counters, 1ull);                           // once per workgroup that changed something
        if (more) dirty_next[tile] = 1u;
    }
    if (tid < 27 && tid != 13 && ((all >> tid) & 1)) {
        const int steps = (tid / 9 != 1) + ((tid / 3) % 3 != 1) + (tid % 3 != 1);
        const int64_t to = geo_tile_beside(t, tid, (nz + GEO_TZ - 1) / GEO_TZ, ty, wx);
        if ((CONN == 26 || steps == 1) && to >= 0) dirty_next[to] = 1u;
    }
}
