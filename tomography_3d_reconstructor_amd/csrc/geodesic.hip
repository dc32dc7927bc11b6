// geodesic.hip -- geodesic distance inside the set voxels of the resident bit volume, in millimetres (no counterpart in the
// reference).  Contract, metric and the fixed-point argument: include/tomo_hip.h.
//
// The map is float32 (nz, ny, nx).  dist(p) = min over the set neighbours q of p of fl32(dist(q) + w(q, p)) -- additions and
// minima only, the file is built with -ffp-contract=off.  Rounded addition is monotone in dist(q), so the relaxation has ONE
// least fixed point below the seeded map, and every order of relaxations ends there: the kernel is free to relax tile by tile,
// in any order, with stale neighbours.
//
// Tiles.  A tile is GEO_TZ x GEO_TY x 64 voxels, one 64-bit word of the bit volume wide: the mask of a tile row is one word plus
// bit 63 / bit 0 of the two neighbouring words.  One workgroup of 256 threads per tile; lane = x, so every LDS access of a wave is
// 64 consecutive floats (no bank conflict, the x - 1 / x + 1 reads included), and a thread owns the 16 rows wave + 4 k of its
// column in registers.  LDS: the (TZ + 2) x (TY + 2) x 66 halo box of floats, 26 400 bytes, the row masks and the z weights.
//
// One sweep (tomo_geo_sweep), on the skeleton of geo_tiles.h.  A workgroup whose flag in dirty_cur is clear leaves at once;
// otherwise it clears the flag (only it reads it), loads its box -- unset voxels and everything outside the stack are +inf -- and relaxes the interior against the
// FIXED halo until a round changes nothing.  A round is race free: every thread forms the candidates of its voxels from the
// published LDS copy, all pass a barrier, the changed values are published, __syncthreads_or ends the round.  The rounds are
// bounded by GEO_ROUNDS, the number of interior voxels (a shortest path inside the tile has fewer steps); a tile that hits the
// bound marks itself in dirty_next.  Only the changed voxels are stored back, by their owner alone: dist needs no atomics.  A
// neighbouring tile may read such a voxel while it is written: it gets the old or the new value (aligned 32-bit accesses do not
// tear), both are upper bounds of the fixed point, and the writer marks every neighbouring tile next to a changed face, edge or
// corner voxel in dirty_next, so the reader runs again in the next sweep, after the kernel boundary has published the store.
// Nothing waits on another workgroup: no grid barrier, no persistent grid, no spin.  The host stops when a sweep changed nothing.
//
// Zones of markers (tomo_zone_seed_labels, tomo_zone_sweep, tomo_zone_cut) sit further down: a second phase over the FINAL map that
// says which marker reached a voxel, on the same tiles and flags, and the cut between zones.  The kernels above are not touched.
#include "geo_tiles.h"                             // the tiles and the skeleton of a sweep, shared with reconstruct.hip and thin.hip
#include <math.h>

#define GEO_F_SEED 4ull                            // counters[1]: a seed index outside the volume or on an unset voxel

TOMO_API int64_t tomo_geo_tiles(int nz, int ny, int nx)
{
    GeoGrid g;
    const int r = geo_grid(nz, ny, nx, &g);
    return r != TOMO_OK ? r : g.tiles;
}

// ---------------------------------------------------------------------------------------------- seeding
// A seed is a change nobody relaxed: its own tile is dirty, and so is every neighbouring tile next to it when it lies on a face,
// an edge or a corner of its tile -- the sweep marks neighbours only for voxels IT lowered, and a seed is at its minimum already.
// Every writer stores the same 1.
__device__ static inline void geo_mark_seed(u32 *__restrict__ dirty, int z, int y, int x, int nz, int ty, int wx)
{
    const int bz = z / GEO_TZ, by = y / GEO_TY, bx = x >> 6;
    const int lz = z % GEO_TZ, ly = y % GEO_TY, lx = x & 63;
    const int tz = (nz + GEO_TZ - 1) / GEO_TZ;
    for (int dz = -1; dz <= 1; dz++) {
        if ((dz < 0 && lz != 0) || (dz > 0 && lz != GEO_TZ - 1) || bz + dz < 0 || bz + dz >= tz) continue;
        for (int dy = -1; dy <= 1; dy++) {
            if ((dy < 0 && ly != 0) || (dy > 0 && ly != GEO_TY - 1) || by + dy < 0 || by + dy >= ty) continue;
            for (int dx = -1; dx <= 1; dx++) {
                if ((dx < 0 && lx != 0) || (dx > 0 && lx != 63) || bx + dx < 0 || bx + dx >= wx) continue;
                dirty[((int64_t)(bz + dz) * ty + (by + dy)) * wx + (bx + dx)] = 1u;
            }
        }
    }
}

// a wave is one word of a row, a lane one voxel: dist = 0.0 at a set seed, +inf elsewhere
__global__ __launch_bounds__(GEO_THREADS) void geo_seed_bits_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ seeds,
                                                                    int64_t nwords, int nz, int ny, int nx, int wx, int ty,
                                                                    float *__restrict__ dist, u32 *__restrict__ dirty)
{
    GeoLane p;
    if (!geo_lane(nwords, wx, &p)) return;
    const u64 m = geo_word(bits + p.row * wx, nx, wx, p.w) & seeds[p.word];
    const bool seed = (m >> p.b) & 1;                        // below nx: the tail bits of m are zero
    if (p.x < nx) dist[p.row * nx + p.x] = seed ? 0.0f : INFINITY;
    if (seed) {
        const int z = (int)(p.row / ny), y = (int)(p.row - (int64_t)z * ny);
        if (p.b == 0 || p.b == 63 || p.b == __ffsll((long long)m) - 1)      // one lane for the tile itself, the two ends for the x faces
            geo_mark_seed(dirty, z, y, p.x, nz, ty, wx);
    }
}

// one thread per entry: 0.0 at flat index index[c] where sel is NULL or sel[c] is set; all ones: skipped
__global__ __launch_bounds__(GEO_THREADS) void geo_seed_index_kernel(const u64 *__restrict__ bits, int64_t total, int nz, int ny, int nx,
                                                                     int wx, int ty, const u64 *__restrict__ index,
                                                                     const uint8_t *__restrict__ sel, int64_t n,
                                                                     float *__restrict__ dist, u32 *__restrict__ dirty,
                                                                     unsigned long long *counters)
{
    const int64_t c = (int64_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (c >= n || (sel && !sel[c])) return;
    const u64 at = index[c];
    if (at == ~0ull) return;
    if (at >= (u64)total) {
        atomicOr(counters + 1, GEO_F_SEED);
        return;
    }
    const int64_t row = (int64_t)(at / (u64)nx);
    const int x = (int)((int64_t)at - row * nx);
    if (!((geo_word(bits + row * wx, nx, wx, x >> 6) >> (x & 63)) & 1)) {
        atomicOr(counters + 1, GEO_F_SEED);
        return;
    }
    const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
    dist[at] = 0.0f;                                         // a plain vector store; equal entries store the same value
    geo_mark_seed(dirty, z, y, x, nz, ty, wx);
}

// ---------------------------------------------------------------------------------------------- one sweep
// the 13 neighbours behind a voxel and the 13 in front of it are visited by their offset into the halo box; class of the step:
// 0 x, 1 y, 2 xy (wxy), then 0 z, 1 zx, 2 zy, 3 zyx (a row of wz)
template <int CONN>
__device__ static inline float geo_relax(const float *__restrict__ p, float d, const float wx_, const float wy_, const float wxy_,
                                         const float *__restrict__ wlo, const float *__restrict__ whi)
{
    // p points at the voxel inside the halo box; strides: x 1, y GEO_HX, z GEO_HY * GEO_HX
    const int sy = GEO_HX, sz = GEO_HY * GEO_HX;
    float c = d;
    c = fminf(c, p[-1] + wx_);
    c = fminf(c, p[1] + wx_);
    c = fminf(c, p[-sy] + wy_);
    c = fminf(c, p[sy] + wy_);
    c = fminf(c, p[-sz] + wlo[0]);
    c = fminf(c, p[sz] + whi[0]);
    if (CONN == 26) {
        c = fminf(c, p[-sy - 1] + wxy_);
        c = fminf(c, p[-sy + 1] + wxy_);
        c = fminf(c, p[sy - 1] + wxy_);
        c = fminf(c, p[sy + 1] + wxy_);
#pragma unroll
        for (int s = -1; s <= 1; s += 2) {
            const float *q = p + s * sz;
            const float *w = s < 0 ? wlo : whi;
            c = fminf(c, q[-1] + w[1]);
            c = fminf(c, q[1] + w[1]);
            c = fminf(c, q[-sy] + w[2]);
            c = fminf(c, q[sy] + w[2]);
            c = fminf(c, q[-sy - 1] + w[3]);
            c = fminf(c, q[-sy + 1] + w[3]);
            c = fminf(c, q[sy - 1] + w[3]);
            c = fminf(c, q[sy + 1] + w[3]);
        }
    }
    return c;
}

// Two workgroups per CU at least: unbounded, the 26-neighbour variant unrolls into 256 VGPRs and one workgroup per CU; bounded it
// takes 170, spills nothing, and a sweep takes 0.6 of the time (profiles/r31_geodesic.md).  The 6-neighbour variant takes 127.
template <int CONN>
__global__ __launch_bounds__(GEO_THREADS, 2) void geo_sweep_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx, int ty,
                                                                const float *__restrict__ wxy, const float *__restrict__ wz,
                                                                float *dist, u32 *dirty_cur, u32 *dirty_next,
                                                                unsigned long long *counters)
{
    __shared__ float box[GEO_BOX];
    __shared__ u64 smid[GEO_HROWS];                          // the word of a halo row; 0 outside the stack
    __shared__ u32 sside[GEO_HROWS];                         // bit 0: the voxel left of the word is set, bit 1: right
    __shared__ float swz[(GEO_TZ + 1) * 4];                  // boundary b: between halo slices b and b + 1
    __shared__ u32 snb;                                      // the neighbouring tiles to mark, one bit per (dz, dy, dx)

    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (!geo_enter(dirty_cur, tile, &snb)) return;
    const GeoTile t = geo_tile(tile, wx, ty);
    geo_halo_masks(bits, nz, ny, nx, wx, t, smid, sside);
    geo_z_weights(wz, nz, t, swz);
    __syncthreads();

    // the box: dist under the mask, +inf at unset voxels and outside the stack
    for (int i = tid; i < GEO_BOX; i += GEO_THREADS) {
        const int hr = i / GEO_HX, xx = i - hr * GEO_HX;
        box[i] = geo_halo_set(smid, sside, hr, xx) ? dist[geo_halo_voxel(t, hr, xx, ny, nx)] : INFINITY;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const float w_x = wxy[0], w_y = wxy[1], w_xy = wxy[2];
    float d[GEO_PER];
    u32 mine = 0, moved = 0;                                 // bit k: voxel k is set / has changed since the load
#pragma unroll
    for (int k = 0; k < GEO_PER; k++) {
        const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
        d[k] = *geo_box_at(box, lz, ly, lane);
        if ((smid[geo_halo_row(lz, ly)] >> lane) & 1) mine |= 1u << k;
    }

    int more = 1, round = 0;
    for (; round < GEO_ROUNDS && more; round++) {            // bounded: a tile that needs more marks itself in geo_leave
        u32 now = 0;
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            if (!((mine >> k) & 1)) continue;
            const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
            const float c = geo_relax<CONN>(geo_box_at(box, lz, ly, lane), d[k], w_x, w_y, w_xy, swz + 4 * lz, swz + 4 * (lz + 1));
            if (c < d[k]) {
                d[k] = c;
                now |= 1u << k;
            }
        }
        __syncthreads();                                     // every candidate of the round is formed: publish
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            const int r = wave + 4 * k;
            if ((now >> k) & 1) *geo_box_at(box, r / GEO_TY, r % GEO_TY, lane) = d[k];
        }
        moved |= now;
        more = __syncthreads_or((int)now);
    }

    // store what changed, and name the neighbouring tiles next to a changed face, edge or corner voxel
    u32 nb = 0;
#pragma unroll
    for (int k = 0; k < GEO_PER; k++) {
        if (!((moved >> k) & 1)) continue;
        const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
        dist[geo_voxel(t, lz, ly, lane, ny, nx)] = d[k];
        nb |= geo_marks(geo_steps(lz, GEO_TZ), geo_steps(ly, GEO_TY), geo_steps(lane, 64));
    }
    geo_leave<CONN>(nb, more, &snb, tile, t, nz, ty, wx, dirty_next, counters);
}

// ---------------------------------------------------------------------------------------------- reach
// out word = the set voxels with dist <= max_mm (max_mm = +inf: with a finite dist); a wave is one word, tail bits zero
__global__ __launch_bounds__(GEO_THREADS) void geo_reach_kernel(const u64 *__restrict__ bits, const float *__restrict__ dist,
                                                                int64_t nwords, int nx, int wx, double max_mm, int finite,
                                                                u64 *__restrict__ out)
{
    GeoLane p;
    if (!geo_lane(nwords, wx, &p)) return;
    bool bit = false;
    if (p.x < nx && ((bits[p.word] >> p.b) & 1)) {
        const float v = dist[p.row * nx + p.x];
        bit = finite ? v < INFINITY : (double)v <= max_mm;
    }
    const u64 m = __ballot(bit);
    if (p.b == 0) out[p.word] = m;
}

// ---------------------------------------------------------------------------------------------- zones of markers
// Which marker reached a voxel (contract: include/tomo_hip.h).  Two phases: the distance sweeps above run to their fixed point
// first, untouched; then labels fall along the TIGHT edges of the final map -- q -> p with fl32(dist(q) + w) == dist(p), the add
// geo_relax makes -- until zone(p) = the smallest label that reaches p.  The graph is fixed in this phase, so the least fixed
// point is unique and the argument of the distance sweep carries over word for word: labels only fall, a stale read is an upper
// bound, the writer marks the reader.
// The map holds 0 for "no zone" throughout; the kernels order labels by the key (u32)(zone - 1), which makes 0 the largest.
#define ZONE_NONE 0xffffffffu

__device__ static inline u32 zone_key(int zone) { return (u32)zone - 1u; }

// a wave is one word of a row, a lane one voxel: a positive marker entry on a set voxel seeds dist = 0.0 and zone = the label
__global__ __launch_bounds__(GEO_THREADS) void zone_seed_kernel(const u64 *__restrict__ bits, const int *__restrict__ markers,
                                                                int64_t nwords, int nz, int ny, int nx, int wx, int ty,
                                                                float *__restrict__ dist, int *__restrict__ zone, u32 *__restrict__ dirty)
{
    GeoLane p;
    if (!geo_lane(nwords, wx, &p)) return;
    int label = 0;
    if ((geo_word(bits + p.row * wx, nx, wx, p.w) >> p.b) & 1) {      // below nx: the tail bits are masked
        const int v = markers[p.row * nx + p.x];
        if (v > 0) label = v;
    }
    const u64 m = __ballot(label > 0);
    if (p.x < nx) {
        dist[p.row * nx + p.x] = label > 0 ? 0.0f : INFINITY;
        zone[p.row * nx + p.x] = label;
    }
    if (label > 0) {
        const int z = (int)(p.row / ny), y = (int)(p.row - (int64_t)z * ny);
        if (p.b == 0 || p.b == 63 || p.b == __ffsll((long long)m) - 1)
            geo_mark_seed(dirty, z, y, p.x, nz, ty, wx);
    }
}

// the neighbours of a voxel of the halo box in ONE order: f(j, offset into the box, weight of the step), j = 0 .. CONN - 1
template <int CONN, typename F>
__device__ static inline void zone_neighbours(const float wx_, const float wy_, const float wxy_, const float *__restrict__ wlo,
                                              const float *__restrict__ whi, F f)
{
    const int sy = GEO_HX, sz = GEO_HY * GEO_HX;
    f(0, -1, wx_);
    f(1, 1, wx_);
    f(2, -sy, wy_);
    f(3, sy, wy_);
    f(4, -sz, wlo[0]);
    f(5, sz, whi[0]);
    if (CONN == 26) {
        f(6, -sy - 1, wxy_);
        f(7, -sy + 1, wxy_);
        f(8, sy - 1, wxy_);
        f(9, sy + 1, wxy_);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int o = s ? sz : -sz, j = 10 + 8 * s;
            const float *w = s ? whi : wlo;
            f(j + 0, o - 1, w[1]);
            f(j + 1, o + 1, w[1]);
            f(j + 2, o - sy, w[2]);
            f(j + 3, o + sy, w[2]);
            f(j + 4, o - sy - 1, w[3]);
            f(j + 5, o - sy + 1, w[3]);
            f(j + 6, o + sy - 1, w[3]);
            f(j + 7, o + sy + 1, w[3]);
        }
    }
}

// One label sweep, on the same skeleton as geo_sweep_kernel (geo_tiles.h): tiles, flags, rounds and marks.  dist is read only: the tight edges into
// a thread's 16 voxels are found ONCE per visit (a bit per neighbour, in registers), the rounds then only take minima of keys
// over those bits.  Two boxes in LDS, 54 148 bytes with the masks: two workgroups per CU (160 KiB), which the launch bound asks
// of the registers as well.
template <int CONN>
__global__ __launch_bounds__(GEO_THREADS, 2) void zone_sweep_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx, int ty,
                                                                 const float *__restrict__ wxy, const float *__restrict__ wz,
                                                                 const float *__restrict__ dist, int *zone, u32 *dirty_cur,
                                                                 u32 *dirty_next, unsigned long long *counters)
{
    __shared__ float box[GEO_BOX];                           // dist: +inf at unset voxels and outside the stack
    __shared__ u32 zbox[GEO_BOX];                            // keys: ZONE_NONE there
    __shared__ u64 smid[GEO_HROWS];
    __shared__ u32 sside[GEO_HROWS];
    __shared__ float swz[(GEO_TZ + 1) * 4];
    __shared__ u32 snb;

    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (!geo_enter(dirty_cur, tile, &snb)) return;
    const GeoTile t = geo_tile(tile, wx, ty);
    geo_halo_masks(bits, nz, ny, nx, wx, t, smid, sside);
    geo_z_weights(wz, nz, t, swz);
    __syncthreads();

    for (int i = tid; i < GEO_BOX; i += GEO_THREADS) {
        const int hr = i / GEO_HX, xx = i - hr * GEO_HX;
        float v = INFINITY;
        u32 key = ZONE_NONE;
        if (geo_halo_set(smid, sside, hr, xx)) {
            const int64_t at = geo_halo_voxel(t, hr, xx, ny, nx);
            v = dist[at];
            key = zone_key(zone[at]);
        }
        box[i] = v;
        zbox[i] = key;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const float w_x = wxy[0], w_y = wxy[1], w_xy = wxy[2];
    u32 key[GEO_PER], tight[GEO_PER];                        // tight[k] bit j: the edge from neighbour j into voxel k is tight
    u32 live = 0, moved = 0;                                 // bit k: voxel k has a tight edge / has changed since the load
#pragma unroll
    for (int k = 0; k < GEO_PER; k++) {
        const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
        const float *p = geo_box_at(box, lz, ly, lane);
        const float d = *p;
        key[k] = zbox[p - box];                              // the two boxes have one layout
        u32 m = 0;
        if (d < INFINITY)                                    // an unset or unreached voxel takes no part
            zone_neighbours<CONN>(w_x, w_y, w_xy, swz + 4 * lz, swz + 4 * (lz + 1), [&](int j, int off, float w) {
                if (p[off] + w == d) m |= 1u << j;           // the add of geo_relax; +inf + w is no finite d
            });
        tight[k] = m;
        if (m) live |= 1u << k;
    }

    int more = 1, round = 0;
    for (; round < GEO_ROUNDS && more; round++) {            // bounded: a tile that needs more marks itself in geo_leave
        u32 now = 0;
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            if (!((live >> k) & 1)) continue;
            const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
            const u32 *q = geo_box_at(zbox, lz, ly, lane);
            u32 loose = ~tight[k];
            asm volatile("" : "+v"(loose));                  // opaque per round: the per-bit tests are not hoisted out of the loop
            u32 c = key[k];                                  // (hoisted, 416 lane masks spill the scalar registers)
            zone_neighbours<CONN>(w_x, w_y, w_xy, swz + 4 * lz, swz + 4 * (lz + 1), [&](int j, int off, float) {
                c = min(c, q[off] | (u32)((int)(loose << (31 - j)) >> 31));      // a loose edge reads ZONE_NONE
            });
            if (c < key[k]) {
                key[k] = c;
                now |= 1u << k;
            }
        }
        __syncthreads();                                     // every candidate of the round is formed: publish
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            const int r = wave + 4 * k;
            if ((now >> k) & 1) *geo_box_at(zbox, r / GEO_TY, r % GEO_TY, lane) = key[k];
        }
        moved |= now;
        more = __syncthreads_or((int)now);
    }

    // store what changed, and name the neighbouring tiles next to a changed face, edge or corner voxel
    u32 nb = 0;
#pragma unroll
    for (int k = 0; k < GEO_PER; k++) {
        if (!((moved >> k) & 1)) continue;
        const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
        zone[geo_voxel(t, lz, ly, lane, ny, nx)] = (int)(key[k] + 1u);
        nb |= geo_marks(geo_steps(lz, GEO_TZ), geo_steps(ly, GEO_TY), geo_steps(lane, 64));
    }
    geo_leave<CONN>(nb, more, &snb, tile, t, nz, ty, wx, dirty_next, counters);
}

// The cut: a wave takes ZONE_CUT_WORDS consecutive words one after the other, a lane is one voxel of the word.  A set voxel p goes
// when a SET neighbour q has 0 < zone(q) < zone(p) -- the bits of q are tested, so a map handed in with entries on unset voxels
// cuts nothing there.  out word = the survivors, tail bits zero.  The cleared voxels of a wave's words are added up in a register
// and sent with ONE atomic per wave: one per word put 2.1 million atomics on one address at 512^3 and took 25 ms on 50 % noise.
#define ZONE_CUT_WORDS 32

template <int CONN>
__global__ __launch_bounds__(GEO_THREADS) void zone_cut_kernel(const u64 *__restrict__ bits, const int *__restrict__ zone, int64_t nwords,
                                                               int nz, int ny, int nx, int wx, u64 *__restrict__ out,
                                                               unsigned long long *counter)
{
    const int64_t t = (int64_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    const int64_t first = (t >> 6) * ZONE_CUT_WORDS;         // the same for the 64 lanes of a wave, and so is the loop below
    const int b = (int)(t & 63);
    unsigned long long cleared = 0;
    for (int64_t word = first; word < first + ZONE_CUT_WORDS && word < nwords; word++) {
        const int64_t row = word / wx;
        const int w = (int)(word - row * wx);
        const int x = 64 * w + b;
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const u64 mid = geo_word(bits + row * wx, nx, wx, w);
        bool clear = false;
        if ((mid >> b) & 1) {
            const int zp = zone[row * nx + x];
            if (zp > 1) {                                    // no zone and zone 1 have nothing below them
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            const int steps = (dz != 0) + (dy != 0) + (dx != 0);
                            if (steps == 0 || (CONN == 6 && steps != 1)) continue;
                            const int zz = z + dz, yy = y + dy, xx = x + dx;
                            if (zz < 0 || zz >= nz || yy < 0 || yy >= ny || xx < 0 || xx >= nx) continue;
                            const int64_t r = (int64_t)zz * ny + yy;
                            if (!((bits[r * wx + (xx >> 6)] >> (xx & 63)) & 1)) continue;      // xx < nx: no tail bit is read
                            const int zq = zone[r * nx + xx];
                            clear |= zq > 0 && zq < zp;
                        }
            }
        }
        const u64 gone = __ballot(clear);
        if (b == 0) out[word] = mid & ~gone;
        cleared += (unsigned long long)__popcll(gone);
    }
    if (b == 0 && cleared) atomicAdd(counter, cleared);      // one integer atomic per wave
}

// ---------------------------------------------------------------------------------------------- entry points
TOMO_API int tomo_geo_seed_bits(const uint64_t *bits, const uint64_t *seeds, int nz, int ny, int nx, float *dist, uint32_t *dirty,
                                void *stream)
{
    GeoGrid g;
    if (!bits || !seeds || !dist || !dirty) return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(geo_seed_bits_kernel, dim3((unsigned)ceil_div64(g.words * 64, GEO_THREADS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, (const u64 *)seeds, g.words, nz, ny, nx, (int)g.wx, (int)g.ty, dist, dirty);
    return tomo_status();
}

TOMO_API int tomo_geo_seed_index(const uint64_t *bits, int nz, int ny, int nx, const uint64_t *index, const uint8_t *sel, int64_t n,
                                 float *dist, uint32_t *dirty, unsigned long long *counters, void *stream)
{
    GeoGrid g;
    if (!bits || !index || !dist || !dirty || !counters || n <= 0) return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    if (ceil_div64(n, GEO_THREADS) >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(geo_seed_index_kernel, dim3((unsigned)ceil_div64(n, GEO_THREADS)), dim3(GEO_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, (int64_t)nz * ny * nx, nz, ny, nx, (int)g.wx, (int)g.ty, (const u64 *)index, sel, n, dist, dirty,
                       counters);
    return tomo_status();
}

TOMO_API int tomo_geo_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *wxy, const float *wz,
                            float *dist, uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters, void *stream)
{
    GeoGrid g;
    if (!bits || !wxy || !wz || !dist || !dirty_cur || !dirty_next || !counters || dirty_cur == dirty_next ||
        (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    geo_launch<geo_sweep_kernel<6>, geo_sweep_kernel<26>>(connectivity, dim3((unsigned)g.tiles), stream, (const u64 *)bits, nz, ny, nx,
                                                          (int)g.wx, (int)g.ty, wxy, wz, dist, dirty_cur, dirty_next, counters);
    return tomo_status();
}

TOMO_API int tomo_geo_reach(const uint64_t *bits, const float *dist, int nz, int ny, int nx, double max_mm, uint64_t *out, void *stream)
{
    GeoGrid g;
    if (!bits || !dist || !out || out == bits || (const void *)out == (const void *)dist || !(max_mm >= 0.0)) return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(geo_reach_kernel, dim3((unsigned)ceil_div64(g.words * 64, GEO_THREADS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, dist, g.words, nx, (int)g.wx, max_mm, isinf(max_mm) ? 1 : 0, (u64 *)out);
    return tomo_status();
}

TOMO_API int tomo_zone_seed_labels(const uint64_t *bits, const int32_t *markers, int nz, int ny, int nx, float *dist, int32_t *zone,
                                   uint32_t *dirty, void *stream)
{
    GeoGrid g;
    if (!bits || !markers || !dist || !zone || !dirty || (const void *)markers == (const void *)zone) return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(zone_seed_kernel, dim3((unsigned)ceil_div64(g.words * 64, GEO_THREADS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, (const int *)markers, g.words, nz, ny, nx, (int)g.wx, (int)g.ty, dist,
                       (int *)zone, dirty);
    return tomo_status();
}

TOMO_API int tomo_zone_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *wxy, const float *wz,
                             const float *dist, int32_t *zone, uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters,
                             void *stream)
{
    GeoGrid g;
    if (!bits || !wxy || !wz || !dist || !zone || !dirty_cur || !dirty_next || !counters || dirty_cur == dirty_next ||
        (const void *)dist == (const void *)zone || (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    geo_launch<zone_sweep_kernel<6>, zone_sweep_kernel<26>>(connectivity, dim3((unsigned)g.tiles), stream, (const u64 *)bits, nz, ny, nx,
                                                            (int)g.wx, (int)g.ty, wxy, wz, dist, (int *)zone, dirty_cur, dirty_next,
                                                            counters);
    return tomo_status();
}

TOMO_API int tomo_zone_cut(const uint64_t *bits, const int32_t *zone, int nz, int ny, int nx, int connectivity, uint64_t *out,
                           unsigned long long *counter, void *stream)
{
    GeoGrid g;
    if (!bits || !zone || !out || !counter || out == bits || (const void *)out == (const void *)zone ||
        (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    const dim3 grid((unsigned)ceil_div64(ceil_div64(g.words, ZONE_CUT_WORDS) * 64, GEO_THREADS));
    geo_launch<zone_cut_kernel<6>, zone_cut_kernel<26>>(connectivity, grid, stream, (const u64 *)bits, (const int *)zone, g.words, nz, ny, nx,
                                                        (int)g.wx, (u64 *)out, counter);
    return tomo_status();
}
