// thin.hip -- homotopic thinning of the resident bit volume: the curve skeleton (no counterpart in the reference).  Contract,
// order and the determinism argument: include/tomo_hip.h.
//
// Pure bit work: the 3 x 3 x 3 neighbourhood of a voxel is a 27-bit PICTURE, bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1), cut out
// of nine row words and the side bits of their neighbouring words.  Nothing is kept per voxel: the bit volume, and one u32 per
// geo_tiles.h tile.
//
// One sub-pass (tomo_thin_pass).  A workgroup of 256 is one 8 x 8 x 64 tile and leaves at once when the tile is not due.  Only
// the rows of the sub-pass's (z & 1, y & 1) do anything: 16 of the tile's 64, four per wave.  For a row the wave's lanes
// 0 .. 26 load the 27 words around it -- masked through geo_word, zero outside the stack -- and the wave reads them back as
// wave-uniform values.  The candidates of the word come from word-wide operations, a lane is a bit: it cuts its picture out of
// the uniform words and runs the two component counts as bit floods (thin_step26 / thin_step6: shifts inside the 3 x 3 x 3
// cube against constant masks).  The wave ballots the deleted lanes and ONE lane stores word & ~ballot.  The simple test is
// COMPUTED; no table is read.
//
// In place, without a second buffer.  The rows y +- 1 and z +- 1 have another parity and are not written in this sub-pass.  In
// its own row every bit a candidate reads lies at x +- 1: the other x-parity, the same before and after any concurrent aligned
// 64-bit store of that word.  Every word has one writer per launch.  So every read sees the volume as it stood when the
// sub-pass began, on every run and under every tiling.
//
// Idle tiles.  stamp[tile] is the tick (the 1-based count of sub-passes of the call) of the latest sub-pass in which the tile,
// or a neighbouring tile next to a cleared face, edge or corner voxel, lost a voxel; the writer raises it with atomicMax.  A
// tile is due at tick t while stamp + 48 >= t: a voxel's verdict in a kind of sub-pass can only change when its picture changed
// since that kind last ran, 48 ticks ago.  A stamp raised during the very launch that reads it makes a tile due that need not
// be -- it then clears nothing, by the same argument -- so the rule changes the work and never the bytes.
#include "cc_runs.h"
#include "geo_tiles.h"
#include "thin_picture.h"

#define THIN_SLOTS 64                              // the cleared voxels are added up in that many counters, 128 bytes apart:
#define THIN_SLOT_WORDS 16                         // atomics of many waves on ONE address queue up behind each other
#define THIN_KINDS 48u                             // sub-passes of one iteration: a tile rests after that many idle ticks
#define THIN_ALL 0x07ffffffu                       // the 27 bits of the cube
#define THIN_X0 0x01249249u                        // the cells with dx = -1: bits 0, 3, 6, ...
#define THIN_X2 (THIN_X0 << 2)                     // dx = +1
#define THIN_Y0 0x001c0e07u                        // dy = -1: bits 0 .. 2 of every slice of nine
#define THIN_Y2 (THIN_Y0 << 6)                     // dy = +1
#define THIN_N6 ((1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22))       // the six face neighbours
#define THIN_N18 (THIN_ALL & ~THIN_CENTRE & ~0x05140145u)  // the cube without its centre and its eight corners

// the cells of m that the cells of f reach in one step of the 26-adjacency (f itself included): a box dilation, axis by axis
__device__ static inline u32 thin_step26(u32 f, u32 m)
{
    f |= ((f & ~THIN_X2) << 1) | ((f & ~THIN_X0) >> 1);
    f |= ((f & ~THIN_Y2) << 3) | ((f & ~THIN_Y0) >> 3);
    f |= (f << 9) | (f >> 9);
    return f & m;
}

// ... and of the 6-adjacency: the three axes side by side
__device__ static inline u32 thin_step6(u32 f, u32 m)
{
    const u32 g = f | ((f & ~THIN_X2) << 1) | ((f & ~THIN_X0) >> 1) | ((f & ~THIN_Y2) << 3) | ((f & ~THIN_Y0) >> 3) | (f << 9) | (f >> 9);
    return g & m;
}

// T26(m) == 1: m is not empty and the flood from its lowest cell covers it.  The flood grows by a cell a turn at least: 26 turns
__device__ static inline bool thin_one26(u32 m)
{
    if (!m) return false;
    u32 f = m & (0u - m);
    for (int i = 0; i < 27; i++) {
        const u32 g = thin_step26(f, m);
        if (g == f) break;
        f = g;
    }
    return f == m;
}

// T6(m) == 1: exactly one 6-connected component of m inside N18 holds a face neighbour of the centre
__device__ static inline bool thin_one6(u32 m)
{
    m &= THIN_N18;
    const u32 faces = m & THIN_N6;
    if (!faces) return false;
    u32 f = faces & (0u - faces);
    for (int i = 0; i < 27; i++) {
        const u32 g = thin_step6(f, m);
        if (g == f) break;
        f = g;
    }
    return (faces & ~f) == 0;
}

// pic: the 27-bit picture of a voxel, its centre bit as it is.  Outside the stack is background, so the complement is taken
// inside the cube only.
template <int CONN>
__device__ static inline bool thin_simple(u32 pic)
{
    const u32 x = pic & ~THIN_CENTRE, c = ~pic & THIN_ALL & ~THIN_CENTRE;
    return CONN == 26 ? (thin_one26(x) && thin_one6(c)) : (thin_one6(x) && thin_one26(c));
}

// (thin_load, the 27 words around a word, and thin_picture, a lane's picture out of them: thin_picture.h)

// ---------------------------------------------------------------------------------------------- one sub-pass
template <int CONN>
__global__ __launch_bounds__(GEO_THREADS) void thin_pass_kernel(u64 *bits, const u64 *__restrict__ anchors, int nz, int ny, int nx,
                                                                int wx, int ty, int tzn, int curve, int direction, int subfield,
                                                                u32 *stamp, u32 tick, unsigned long long *counters)
{
    const int64_t tile = blockIdx.x;
    const u32 seen = __hip_atomic_load(stamp + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen + THIN_KINDS < tick) return;                    // uniform: idle for a whole iteration
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GeoTile t = geo_tile(tile, wx, ty);
    const int sx = subfield & 1, sy = (subfield >> 1) & 1, sz = (subfield >> 2) & 1;
    const int z = t.bz * GEO_TZ + sz + 2 * wave;             // a wave: one slice of the tile, its four rows of the y-parity
    if (z >= nz) return;
    const u64 parity = sx ? 0xaaaaaaaaaaaaaaaaull : 0x5555555555555555ull;
    u32 cleared = 0, nb = 0;                                 // nb: the neighbouring tiles to stamp, one bit per (dz, dy, dx)
    for (int j = 0; j < GEO_TY / 2; j++) {
        const int y = t.by * GEO_TY + sy + 2 * j;
        if (y >= ny) break;                                  // wave-uniform
        const u64 mine = thin_load(bits, nz, ny, nx, wx, z, y, t.bx, lane);
        const u64 w = __shfl(mine, 13, 64);
        if (!w) continue;
        u64 towards;                                         // the neighbours in the direction of the sub-pass: -z +z -y +y -x +x
        switch (direction) {
        case 0: towards = __shfl(mine, 4, 64); break;
        case 1: towards = __shfl(mine, 22, 64); break;
        case 2: towards = __shfl(mine, 10, 64); break;
        case 3: towards = __shfl(mine, 16, 64); break;
        case 4: towards = (w << 1) | (__shfl(mine, 12, 64) >> 63); break;
        default: towards = (w >> 1) | (__shfl(mine, 14, 64) << 63); break;
        }
        u64 cand = w & ~towards & parity;
        if (anchors) cand &= ~anchors[((int64_t)z * ny + y) * wx + t.bx];
        if (!cand) continue;                                 // wave-uniform
        const u32 pic = thin_picture(mine, lane);
        bool del = false;
        if ((cand >> lane) & 1) {
            const bool end = __popc(pic & ~THIN_CENTRE) == 1;
            del = !(curve && end) && thin_simple<CONN>(pic);
        }
        const u64 gone = __ballot(del);
        if (!gone) continue;
        if (lane == 0) bits[((int64_t)z * ny + y) * wx + t.bx] = w & ~gone;  // the one writer of this word; tail bits zero
        cleared += (u32)__popcll(gone);
        const u32 xs = 2u | ((gone & 1ull) ? 1u : 0u) | ((gone >> 63) ? 4u : 0u);      // a cleared voxel at either end of the word
        nb |= geo_marks(geo_steps(z - t.bz * GEO_TZ, GEO_TZ), geo_steps(y - t.by * GEO_TY, GEO_TY), xs);
    }
    if (!cleared) return;                                    // wave-uniform
    if (lane == 0) atomicAdd(counters + THIN_SLOT_WORDS * (int)((4 * tile + wave) % THIN_SLOTS), (unsigned long long)cleared);
    if (lane < 27 && ((nb >> lane) & 1)) {                   // bit 13, this tile, is always among them
        const int nbz = t.bz + lane / 9 - 1, nby = t.by + (lane / 3) % 3 - 1, nbx = t.bx + lane % 3 - 1;
        if (nbz >= 0 && nbz < tzn && nby >= 0 && nby < ty && nbx >= 0 && nbx < wx)
            atomicMax(stamp + ((int64_t)nbz * ty + nby) * wx + nbx, tick);
    }
}

// ---------------------------------------------------------------------------------------------- ends and junctions
// a wave is THIN_NODE_WORDS consecutive words, one after the other, a lane one voxel: the set voxels with exactly one set
// 26-neighbour, and with three or more.  The four counts of a workgroup meet in LDS and go out with one atomic each.
#define THIN_NODE_WORDS 8
__global__ __launch_bounds__(GEO_THREADS) void thin_nodes_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx,
                                                                 int64_t nwords, u64 *__restrict__ ends, u64 *__restrict__ junctions,
                                                                 unsigned long long *counters)
{
    __shared__ u32 sums[4];
    if (threadIdx.x < 4) sums[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t first = ((int64_t)blockIdx.x * (GEO_THREADS / 64) + (threadIdx.x >> 6)) * THIN_NODE_WORDS;   // wave-uniform
    u32 nv = 0, ne = 0, nj = 0, nl = 0;
    for (int64_t word = first; word < first + THIN_NODE_WORDS && word < nwords; word++) {
        const int64_t row = word / wx;
        const int bx = (int)(word - row * wx);
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const u64 mine = thin_load(bits, nz, ny, nx, wx, z, y, bx, lane);
        const u64 w = __shfl(mine, 13, 64);
        u64 e = 0, j = 0, lone = 0;
        if (w) {                                             // wave-uniform
            const u32 pic = thin_picture(mine, lane);
            const bool set = (w >> lane) & 1;
            const int n = __popc(pic & ~THIN_CENTRE);
            e = __ballot(set && n == 1);
            j = __ballot(set && n >= 3);
            lone = __ballot(set && n == 0);
        }
        if (lane == 0) {
            ends[word] = e;
            junctions[word] = j;
        }
        nv += (u32)__popcll(w);
        ne += (u32)__popcll(e);
        nj += (u32)__popcll(j);
        nl += (u32)__popcll(lone);
    }
    if (lane == 0 && nv) {                                   // at most 8 x 64 a wave, 2 048 a workgroup
        atomicAdd(&sums[0], nv);
        if (ne) atomicAdd(&sums[1], ne);
        if (nj) atomicAdd(&sums[2], nj);
        if (nl) atomicAdd(&sums[3], nl);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(counters + threadIdx.x, (unsigned long long)sums[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------- a second volume under the runs
// out[columns * slot[c] + column] += the set bits of `other` under the x-runs of the selected component c + 1: one thread per
// word, the popcount of other & run mask, one atomic per run with a count
__global__ __launch_bounds__(CC_THREADS) void thin_count_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                                const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                int64_t cap_runs, const u32 *__restrict__ parent,
                                                                const u32 *__restrict__ rank, const u64 *__restrict__ other,
                                                                const uint8_t *__restrict__ sel, const u32 *__restrict__ slot,
                                                                unsigned long long *out, int column, int columns, int64_t cap,
                                                                int64_t cap_sel, u64 *flags)
{
    const int64_t word = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (!cc_sel_fits(tot, cap, cap_sel, word == 0, flags) || word >= nwords) return;
    const int64_t row = word / wx;
    const int wj = (int)(word - row * wx);
    const u64 *r = bits + row * wx;
    const u64 cur = cc_word(r, nx, wx, wj);
    const u64 o = other[word] & cur;
    if (!o) return;
    const u32 nruns = (u32)cc_count(tot, cap_runs), ncomp = (u32)cc_ncomp(tot, cap);
    CcWordRuns it = cc_word_runs(r, nx, wx, wj, cur, row_off[row]);
    while (cc_word_runs_next(it)) {
        const int k = __popcll(o & it.mask);
        if (!k) continue;
        if (it.run >= nruns) {
            cc_flag(flags, CC_F_RANGE);
            continue;
        }
        const u32 c = cc_component(parent, rank, it.run);
        u32 s;
        if (c >= ncomp || !cc_sel_row(sel, slot, cap_sel, c, true, flags, s)) continue;
        atomicAdd(out + (int64_t)columns * s + column, (unsigned long long)k);
    }
}

// ---------------------------------------------------------------------------------------------- entry points
TOMO_API int tomo_thin_pass(uint64_t *bits, const uint64_t *anchors, int nz, int ny, int nx, int connectivity, int curve, int direction,
                            int subfield, uint32_t *stamp, uint32_t tick, unsigned long long *counters, void *stream)
{
    GeoGrid grid;
    if (!bits || !stamp || !counters || anchors == bits || (connectivity != 6 && connectivity != 26) || direction < 0 || direction > 5 ||
        subfield < 0 || subfield > 7 || (curve && connectivity == 6) || tick == 0u || tick > 0xffffffffu - THIN_KINDS)
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    geo_launch<thin_pass_kernel<6>, thin_pass_kernel<26>>(connectivity, dim3((unsigned)grid.tiles), stream, (u64 *)bits, (const u64 *)anchors,
                                                          nz, ny, nx, (int)grid.wx, (int)grid.ty, (int)grid.tz, curve ? 1 : 0, direction,
                                                          subfield, (u32 *)stamp, (u32)tick, counters);
    return tomo_status();
}

TOMO_API int tomo_thin_nodes(const uint64_t *bits, int nz, int ny, int nx, uint64_t *ends_out, uint64_t *junctions_out,
                             unsigned long long *counters, void *stream)
{
    GeoGrid grid;
    if (!bits || !ends_out || !junctions_out || !counters || ends_out == bits || junctions_out == bits || ends_out == junctions_out)
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(thin_nodes_kernel, dim3((unsigned)ceil_div64(grid.words, (GEO_THREADS / 64) * THIN_NODE_WORDS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, nz, ny, nx, (int)grid.wx, grid.words, (u64 *)ends_out, (u64 *)junctions_out,
                       counters);
    return tomo_status();
}

TOMO_API int tomo_thin_count(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                             const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint64_t *other,
                             const uint8_t *sel, const uint32_t *slot, int64_t *out, int column, int columns, int64_t cap,
                             int64_t cap_sel, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !other || !sel || !slot || !out || cap_runs <= 0 || cap <= 0 || cap_sel <= 0 ||
        columns <= 0 || column < 0 || column >= columns || (const void *)out == (const void *)bits || (const void *)out == (const void *)other)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;                      // < 2^31 (cc_geometry)
    hipLaunchKernelGGL(thin_count_kernel, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, (const u64 *)other, sel, (const u32 *)slot, (unsigned long long *)out, column, columns, cap,
                       cap_sel, (u64 *)tot + 2);
    return tomo_status();
}
