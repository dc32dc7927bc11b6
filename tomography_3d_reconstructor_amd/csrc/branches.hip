// branches.hip -- the branch table of a skeleton (no counterpart in the reference): regular and node voxels, the steps of every
// branch per slice and direction, the node voxels a branch is attached to, which component a voxel lies in, and the removal of
// flagged components.  Definition and contract: include/tomo_hip.h.
//
// S is any bit volume.  A set voxel with exactly two set 26-neighbours is REGULAR (R), every other set voxel a NODE voxel
// (N = S \ R).  Branches are the 26-components of R, nodes those of N; both are labelled by components.hip as any volume is,
// and everything here works under those run tables.
//
// tomo_branch_split is tomo_thin_nodes' pass with another question: a wave is a word, a lane a bit, the lane's 27-bit picture
// (thin_picture.h) gives its neighbour count, the wave ballots and one lane stores both words.
// tomo_branch_hist is tomo_cc_surface_hist's pass with another counting rule: one thread per row of R slides windows of the row
// and of the neighbour rows along x and popcounts under the masks of the row's runs.  A step to a later voxel may end in R or
// in N, that is anywhere in S; a step to an earlier one counts only when it ends in N.  So the rows in front of p are read from
// S alone, the rows behind it from S and from R: 9 + 5 windows.
// tomo_branch_attach is a word pass over R: a lane whose voxel has a node voxel beside it -- picture of S without picture of R --
// knows the flat index of the lowest and of the highest one; the lanes of a run meet in wave reductions and one lane sends.
// Integer atomics only, nobody waits on anybody: the same bytes on every run.
#include "cc_runs.h"
#include "geo_tiles.h"
#include "thin_picture.h"

#define BRANCH_WAVE_WORDS 8                        // consecutive words a wave of the word passes works through (THIN_NODE_WORDS)

// ---------------------------------------------------------------------------------------------- regular and node voxels
__global__ __launch_bounds__(GEO_THREADS) void branch_split_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx,
                                                                   int64_t nwords, u64 *__restrict__ regular, u64 *__restrict__ nodes,
                                                                   unsigned long long *counters)
{
    __shared__ u32 sums[4];
    if (threadIdx.x < 4) sums[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t first = ((int64_t)blockIdx.x * (GEO_THREADS / 64) + (threadIdx.x >> 6)) * BRANCH_WAVE_WORDS;  // wave-uniform
    u32 nv = 0, nr = 0, nl = 0;
    for (int64_t word = first; word < first + BRANCH_WAVE_WORDS && word < nwords; word++) {
        const int64_t row = word / wx;
        const int bx = (int)(word - row * wx);
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const u64 mine = thin_load(bits, nz, ny, nx, wx, z, y, bx, lane);
        const u64 w = __shfl(mine, 13, 64);
        u64 r = 0, lone = 0;
        if (w) {                                             // wave-uniform
            const u32 pic = thin_picture(mine, lane);
            const bool set = (w >> lane) & 1;
            const int n = __popc(pic & ~THIN_CENTRE);
            r = __ballot(set && n == 2);
            lone = __ballot(set && n == 0);
        }
        if (lane == 0) {                                     // every word is written; w has no tail bits
            regular[word] = r;
            nodes[word] = w & ~r;
        }
        nv += (u32)__popcll(w);
        nr += (u32)__popcll(r);
        nl += (u32)__popcll(lone);
    }
    if (lane == 0 && nv) {                                   // at most 8 x 64 a wave, 2 048 a workgroup
        atomicAdd(&sums[0], nv);
        if (nr) atomicAdd(&sums[1], nr);
        if (nv - nr) atomicAdd(&sums[2], nv - nr);
        if (nl) atomicAdd(&sums[3], nl);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(counters + threadIdx.x, (unsigned long long)sums[threadIdx.x]);
}

TOMO_API int tomo_branch_split(const uint64_t *bits, int nz, int ny, int nx, uint64_t *regular_out, uint64_t *nodes_out,
                               unsigned long long *counters, void *stream)
{
    GeoGrid grid;
    if (!bits || !regular_out || !nodes_out || !counters || regular_out == bits || nodes_out == bits || regular_out == nodes_out)
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(branch_split_kernel, dim3((unsigned)ceil_div64(grid.words, (GEO_THREADS / 64) * BRANCH_WAVE_WORDS)),
                       dim3(GEO_THREADS), 0, (hipStream_t)stream, (const u64 *)bits, nz, ny, nx, (int)grid.wx, grid.words,
                       (u64 *)regular_out, (u64 *)nodes_out, counters);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- the steps of a branch
// The windows of row (z, y) of R: 0 the row, 1 (z, y - 1), 2 .. 4 (z - 1, y - 1 .. y + 1) of R; 5 the row, 6 (z, y - 1),
// 7 (z, y + 1), 8 .. 10 (z + 1, y - 1 .. y + 1), 11 .. 13 (z - 1, y - 1 .. y + 1) of S.
#define BRANCH_WINDOWS 14

// the bits of mask whose neighbour in row s is set: at the same x -> centre, at x + 1 and at x - 1 -> side
__device__ static inline void branch_set_beside(const CcWin &s, u64 mask, u64 &centre, u64 &side)
{
    centre += (u64)__popcll(mask & s.cur);
    side += (u64)(__popcll(mask & cc_xp(s)) + __popcll(mask & cc_xm(s)));
}

// ... is a node voxel: set in s, the row of S, and clear in r, the same row of R
__device__ static inline void branch_node_beside(const CcWin &s, const CcWin &r, u64 mask, u64 &centre, u64 &side)
{
    centre += (u64)__popcll(mask & s.cur & ~r.cur);
    side += (u64)(__popcll(mask & cc_xp(s) & ~cc_xp(r)) + __popcll(mask & cc_xm(s) & ~cc_xm(r)));
}

struct BranchExtra {
    const u64 *other;                                       // S, the volume the regular voxels were split from
};

// The accumulator of row (z, y) of the histogram pass (cc_runs.h).  ANY_ALL: a regular voxel whose two neighbours are earlier
// regular voxels counts nothing, so any() asks every counter, not the first one.
struct BranchAcc : CcCounts<CC_SURF, true> {
    using CcCounts::CcCounts;
    using Extra = BranchExtra;
    static constexpr bool UNLABELLED = false;
    static constexpr int NR = BRANCH_WINDOWS;
    static constexpr CcRowAt ROWS[NR] = {{0, 0, 0}, {0, -1, 0}, {-1, -1, 0}, {-1, 0, 0}, {-1, 1, 0},                 // of R
                                         {0, 0, 1}, {0, -1, 1}, {0, 1, 1}, {1, -1, 1}, {1, 0, 1}, {1, 1, 1},         // of S
                                         {-1, -1, 1}, {-1, 0, 1}, {-1, 1, 1}};
    __device__ void add(const CcWin *win, u64 mask)
    {
        n[0] += (u64)(__popcll(mask & cc_xp(win[5])) + __popcll(mask & cc_xm(win[5]) & ~cc_xm(win[0])));
        branch_node_beside(win[6], win[1], mask, n[1], n[2]);
        branch_set_beside(win[7], mask, n[1], n[2]);
        branch_set_beside(win[8], mask, n[5], n[6]);
        branch_set_beside(win[9], mask, n[3], n[4]);
        branch_set_beside(win[10], mask, n[5], n[6]);
        branch_node_beside(win[11], win[2], mask, n[9], n[10]);
        branch_node_beside(win[12], win[3], mask, n[7], n[8]);
        branch_node_beside(win[13], win[4], mask, n[9], n[10]);
    }
};

TOMO_API int tomo_branch_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                              const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                              const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, const uint64_t *other,
                              void *stream)
{
    const bool ok = other && (const void *)hist != (const void *)bits && (const void *)hist != (const void *)other;
    return cc_hist_launch<BranchAcc>(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, hist, hist_cap, ok,
                                     {(const u64 *)other}, stream);
}

// ---------------------------------------------------------------------------------------------- the attachments of a branch
__global__ __launch_bounds__(CC_THREADS) void branch_attach_init_kernel(unsigned long long *__restrict__ attach,
                                                                        unsigned long long *__restrict__ count, int64_t cap_sel)
{
    const int64_t s = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (s >= cap_sel) return;
    attach[2 * s] = ~0ull;
    attach[2 * s + 1] = 0ull;
    count[s] = 0ull;
}

// A wave is BRANCH_WAVE_WORDS consecutive words of R, one after the other, a lane one voxel.  The cells of the picture ascend in
// raster order, so the lowest and the highest node voxel beside a voxel are the lowest and the highest bit of its cells.
__global__ __launch_bounds__(GEO_THREADS) void branch_attach_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx,
                                                                    int64_t nwords, const u32 *__restrict__ row_off,
                                                                    const u64 *__restrict__ tot, int64_t cap_runs,
                                                                    const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                                    const u64 *__restrict__ other, const uint8_t *__restrict__ sel,
                                                                    const u32 *__restrict__ slot, unsigned long long *attach,
                                                                    unsigned long long *count, int64_t cap, int64_t cap_sel, u64 *flags)
{
    if (!cc_sel_fits(tot, cap, cap_sel, blockIdx.x == 0 && threadIdx.x == 0, flags)) return;
    const u32 nruns = (u32)cc_count(tot, cap_runs), ncomp = (u32)cc_ncomp(tot, cap);
    const int lane = threadIdx.x & 63;
    const int64_t first = ((int64_t)blockIdx.x * (GEO_THREADS / 64) + (threadIdx.x >> 6)) * BRANCH_WAVE_WORDS;  // wave-uniform
    for (int64_t word = first; word < first + BRANCH_WAVE_WORDS && word < nwords; word++) {
        const int64_t row = word / wx;
        const int bx = (int)(word - row * wx);
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const u64 w = geo_word(bits + row * wx, nx, wx, bx); // one word, the same for the wave: most words of R are empty
        if (!w) continue;                                    // wave-uniform
        const u64 mine = thin_load(bits, nz, ny, nx, wx, z, y, bx, lane);
        const u64 around = thin_load(other, nz, ny, nx, wx, z, y, bx, lane);
        const u32 beside = thin_picture(around, lane) & ~thin_picture(mine, lane) & ~THIN_CENTRE;    // every lane takes part in the shuffles
        const u32 cells = ((w >> lane) & 1) ? beside : 0u;
        if (!__ballot(cells != 0u)) continue;                // no voxel of the word has a node voxel beside it
        u64 lo = ~0ull, hi = 0ull;
        if (cells) {                                         // a cell of a set picture lies inside the stack and below nx
            const int a = __ffs((int)cells) - 1, b = 31 - __clz((int)cells);
            const int x = 64 * bx + lane;
            lo = (u64)(((int64_t)(z + a / 9 - 1) * ny + (y + (a / 3) % 3 - 1)) * nx + (x + a % 3 - 1));
            hi = (u64)(((int64_t)(z + b / 9 - 1) * ny + (y + (b / 3) % 3 - 1)) * nx + (x + b % 3 - 1));
        }
        const u64 *r = bits + row * wx;
        CcWordRuns it = cc_word_runs(r, nx, wx, bx, w, row_off[row]);
        while (cc_word_runs_next(it)) {                      // wave-uniform
            const bool has = ((it.mask >> lane) & 1) && cells != 0u;
            if (!__ballot(has)) continue;
            if (it.run >= nruns) {
                if (lane == 0) cc_flag(flags, CC_F_RANGE);
                continue;
            }
            const u32 c = cc_component(parent, rank, it.run);
            u32 s;
            if (c >= ncomp || !cc_sel_row(sel, slot, cap_sel, c, lane == 0, flags, s)) continue;
            const u64 least = wave_min64(has ? lo : ~0ull), most = wave_max64(has ? hi : 0ull);
            const u32 k = wave_sum(has ? (u32)__popc(cells) : 0u);
            if (lane == 0) {
                atomicMin(attach + 2 * (int64_t)s, least);
                atomicMax(attach + 2 * (int64_t)s + 1, most);
                atomicAdd(count + s, (unsigned long long)k);
            }
        }
    }
}

TOMO_API int tomo_branch_attach(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint64_t *other,
                                const uint8_t *sel, const uint32_t *slot, uint64_t *attach, uint64_t *attach_count, int64_t cap,
                                int64_t cap_sel, void *stream)
{
    GeoGrid grid;
    if (!bits || !row_off || !parent || !rank || !tot || !other || !sel || !slot || !attach || !attach_count || cap_runs <= 0 || cap <= 0 ||
        cap_sel <= 0 || attach == attach_count || attach == bits || attach == other || attach_count == bits || attach_count == other)
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(branch_attach_init_kernel, dim3((unsigned)ceil_div64(cap_sel, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (unsigned long long *)attach, (unsigned long long *)attach_count, cap_sel);
    hipLaunchKernelGGL(branch_attach_kernel, dim3((unsigned)ceil_div64(grid.words, (GEO_THREADS / 64) * BRANCH_WAVE_WORDS)),
                       dim3(GEO_THREADS), 0, st, (const u64 *)bits, nz, ny, nx, (int)grid.wx, grid.words, (const u32 *)row_off,
                       (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank, (const u64 *)other, sel, (const u32 *)slot,
                       (unsigned long long *)attach, (unsigned long long *)attach_count, cap, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- the component of a voxel
// The tables hold no run starts -- a run is where the bits say it is -- so the run of a voxel is the row's first run plus the
// starts in the words in front of it and in its own word up to its bit (cc_run_of_bit), not a search.
__global__ __launch_bounds__(CC_THREADS) void branch_lookup_kernel(const u64 *__restrict__ bits, int64_t nvoxels, int nx, int wx,
                                                                   const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                   int64_t cap_runs, const u32 *__restrict__ parent,
                                                                   const u32 *__restrict__ rank, int64_t cap,
                                                                   const int64_t *__restrict__ queries, int64_t n,
                                                                   int64_t *__restrict__ labels, u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    if (i >= n) return;
    const int64_t q = queries[i];
    int64_t label = 0;
    if (q >= 0 && q < nvoxels) {
        const int64_t row = q / nx;
        const int x = (int)(q - row * nx), wj = x >> 6, bit = x & 63;
        const u64 *r = bits + row * wx;
        if ((cc_word(r, nx, wx, wj) >> bit) & 1) {
            const u32 run = cc_run_of_bit(r, nx, wx, wj, bit, row_off[row]);
            if (run < (u32)cc_count(tot, cap_runs)) {
                const u32 c = cc_component(parent, rank, run);
                if (c < (u32)cc_ncomp(tot, cap)) label = (int64_t)c + 1;
            } else {
                cc_flag(flags, CC_F_RANGE);
            }
        }
    }
    labels[i] = label;
}

TOMO_API int tomo_branch_lookup(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap,
                                const int64_t *queries, int64_t n, int64_t *labels_out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !queries || !labels_out || cap_runs <= 0 || cap <= 0 || n <= 0 ||
        (const void *)labels_out == (const void *)queries || (const void *)labels_out == (const void *)bits)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(branch_lookup_kernel, dim3((unsigned)ceil_div64(n, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nrows * nx, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, cap, queries, n, labels_out, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- flagged components removed
// one thread per word of the run tables' volume, as cc_filter_kernel: the runs of the word whose component is flagged leave `in`
__global__ __launch_bounds__(CC_THREADS) void branch_clear_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                                  const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                  int64_t cap_runs, const u32 *__restrict__ parent,
                                                                  const u32 *__restrict__ rank, const uint8_t *__restrict__ flagged,
                                                                  u32 nflagged, const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                  u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= nwords) return;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const int64_t row = i / wx;
    const int wj = (int)(i - row * wx);
    const u64 *r = bits + row * wx;
    const u64 m = cc_word(r, nx, wx, wj);
    u64 res = in[i] & cc_tail_mask(nx, wx, wj);
    if (m) {
        CcWordRuns it = cc_word_runs(r, nx, wx, wj, m, row_off[row]);
        while (cc_word_runs_next(it)) {
            if (it.run < nruns) {
                const u32 c = cc_component(parent, rank, it.run);
                if (c >= nflagged) cc_flag(flags, CC_F_RANGE);
                else if (flagged[c]) res &= ~it.mask;
            } else {
                cc_flag(flags, CC_F_RANGE);
            }
        }
    }
    out[i] = res;
}

TOMO_API int tomo_branch_clear(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                               const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *flagged,
                               int64_t n_flagged, const uint64_t *in, uint64_t *out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !flagged || !in || !out || out == in || out == bits || cap_runs <= 0 || n_flagged <= 0 ||
        n_flagged > cap_runs)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;
    hipLaunchKernelGGL(branch_clear_kernel, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, flagged, (u32)n_flagged, (const u64 *)in, (u64 *)out, (u64 *)tot + 2);
    return tomo_status();
}
