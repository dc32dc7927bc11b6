// cc_runs.h -- the device-side vocabulary of the run tables (components.hip labels them, component_measures.hip measures
// what they hold, branches.hip measures the branches of a skeleton): rows and their runs, the union-find over run ids, which
// run a bit lies in, and the ROW PASS -- one thread per row adds up what its runs give per component, a wave combines -- that
// every per-component quantity goes through; then the WINDOW WALK, the row pass for what a voxel's neighbours decide, with the
// table of its neighbour rows; at the end the HISTOGRAM PASS, WORDS uint64 per slice of every selected component's box: one
// kernel (cc_hist_kernel), one launcher (cc_hist_launch) and one set of counters (CcCounts) for the five such passes of
// component_measures.hip and branches.hip.  A new measurement per slice writes an accumulator's add(), its row list, its word
// count and a finishing loop over its entries; the section says what else an accumulator declares.  In between, the WORD PASS --
// one wave per word, one lane per bit, for what a per-voxel map gives per component: one kernel (cc_word_kernel), one launcher
// (cc_word_launch), a reduction is a pass struct -- and the SELECTED ROW: cc_selected answers whether the selection fits, whether
// a component is selected and which row of a compacted result is its own, for every kernel that writes one; the results that
// only copy columns are writers of cc_rows_kernel.
//
// tot (device uint64[8]): [0] runs  [1] components  [2] flags (1: 2^31 runs or more, 2: more runs than the caller's buffers
// hold, 4: a run id outside the tables -- the bits changed between the calls, 8: tomo_profile_stats met a value it does not
// admit)  [3] label tomo_cc_filter(largest) kept (0: none)  [4] counters of the slice histogram  [5] components tomo_cc_select
// (tomo_cc_zhist_offsets) selected.
#pragma once
#include <array>
#include <utility>
#include "tomo_common.h"

#define CC_THREADS 256
#define CC_SCAN_TILE 1024            // entries per workgroup of the scan kernels (4 per thread)
#define CC_F_MANY 1ull
#define CC_F_CAP 2ull
#define CC_F_RANGE 4ull
#define CC_COLS 10                   // columns of a row of the measurement table (tomo_cc_measure)

static int cc_geometry(const void *bits, int nz, int ny, int nx, int64_t *nrows, int *wx)
{
    if (!bits || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    *wx = (int)tomo_words_per_row(nx);
    *nrows = (int64_t)nz * ny;
    if (*nrows * *wx >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    return TOMO_OK;
}

// (flags == NULL: a call without tables, which has no guard that could fire)
__device__ static inline void cc_flag(u64 *flags, u64 f) { if (flags) atomicOr((unsigned long long *)flags, f); }

// ---------------------------------------------------------------------------------------------- rows and runs
__device__ static inline u64 cc_tail_mask(int nx, int wx, int w)
{
    const int r = nx - 64 * (wx - 1);                      // bits of the last word, 1 .. 64
    return (w == wx - 1 && r < 64) ? ((1ull << r) - 1) : ~0ull;
}

// word w of a row, bits at x >= nx cleared whatever the buffer holds there
__device__ static inline u64 cc_word(const u64 *__restrict__ row, int nx, int wx, int w)
{
    return row[w] & cc_tail_mask(nx, wx, w);
}

// bits of word w at which a run starts
__device__ static inline u64 cc_starts(const u64 *__restrict__ row, int nx, int wx, int w, u64 cur)
{
    const u64 carry = w > 0 ? row[w - 1] >> 63 : 0ull;    // bit 63 of a word before the last is never a tail bit
    return cur & ~((cur << 1) | carry);
}

// the runs of one row, in ascending x: [s, e)
struct CcRuns {
    const u64 *row;
    int nx, wx, pos;
    int s, e;
    bool valid;
};

__device__ static inline void cc_runs_next(CcRuns &it)
{
    const int end = 64 * it.wx;
    it.valid = false;
    if (it.pos >= end) return;
    int w = it.pos >> 6;
    u64 m = cc_word(it.row, it.nx, it.wx, w) & (~0ull << (it.pos & 63));
    while (m == 0) {                                        // w only grows: at most wx turns
        if (++w >= it.wx) { it.pos = end; return; }
        m = cc_word(it.row, it.nx, it.wx, w);
    }
    it.s = 64 * w + __ffsll((long long)m) - 1;
    w = it.s >> 6;
    m = ~cc_word(it.row, it.nx, it.wx, w) & (~0ull << (it.s & 63));
    int e = end;
    while (true) {
        if (m != 0) { e = 64 * w + __ffsll((long long)m) - 1; break; }
        if (++w >= it.wx) break;
        m = ~cc_word(it.row, it.nx, it.wx, w);
    }
    it.e = e;
    it.pos = e;
    it.valid = true;
}

__device__ static inline CcRuns cc_runs_begin(const u64 *__restrict__ bits, int64_t row, int nx, int wx)
{
    CcRuns it;
    it.row = bits + row * wx;
    it.nx = nx;
    it.wx = wx;
    it.pos = 0;
    it.s = it.e = 0;
    cc_runs_next(it);
    return it;
}

// ---------------------------------------------------------------------------------------------- the counts of the tables
// n comes from the host (n_dev == NULL) or from device memory, clipped to the capacity the grid was sized for
__device__ static inline int64_t cc_count(const u64 *n_dev, int64_t cap)
{
    if (!n_dev) return cap;
    const u64 n = *n_dev;
    return n > (u64)cap ? 0 : (int64_t)n;                  // too many for the buffers: nothing is touched (flag CC_F_CAP)
}

// the count of components comes from tot[1]; more than a table's rows: nothing is touched (CC_F_CAP)
__device__ static inline int64_t cc_ncomp(const u64 *tot, int64_t cap)
{
    const u64 n = tot[1];
    return n > (u64)cap ? 0 : (int64_t)n;
}

// one workgroup: blk[i] = sum of blk[0 .. i) for i < nblk, *total = the sum of all; 1024 entries per step with a running carry
static __global__ __launch_bounds__(1024) void cc_scan1_kernel(u64 *__restrict__ blk, int64_t nblk, u64 *__restrict__ total, u64 *flags)
{
    __shared__ u64 wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (int64_t i0 = 0; i0 < nblk; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const u64 v = i < nblk ? blk[i] : 0;
        const u64 inc = wave_inclusive_scan64(v);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u64 before = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const u64 x = wsum[w];
            before += w < wave ? x : 0;
            sum += x;
        }
        if (i < nblk) blk[i] = carry + before + inc - v;
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (flags && carry >= (1ull << 31)) *flags |= CC_F_MANY;
    }
}

// ---------------------------------------------------------------------------------------------- union-find over runs
__device__ static inline u32 cc_load(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this thread can see it (ids strictly decrease along the way: at most x steps)
__device__ static inline u32 cc_find(const u32 *parent, u32 x)
{
    u32 p = cc_load(parent + x);
    while (p < x) {
        x = p;
        p = cc_load(parent + x);
    }
    return x;
}

// ... and every run on the way is pointed at it (atomicMin: a parent never rises)
__device__ static inline u32 cc_find_compress(u32 *parent, u32 x)
{
    const u32 r = cc_find(parent, x);
    while (x > r) {
        const u32 old = atomicMin(parent + x, r);
        if (old >= x) break;
        x = old;
    }
    return r;
}

// Only a ROOT is ever hooked (compare-and-swap): the parent of a run that has one is changed by cc_find_compress alone, to an
// ancestor further up, so a root a thread has found stays an ancestor of every run it found it from.  Hooking with atomicMin
// would also re-parent a run that somebody else hooked in the meantime, into ANOTHER tree; a cc_find_compress still on its way
// to the root it found before that then walks on in that other tree and points its runs at the old root, which cuts them off
// from their own, smaller root for good (seen past 900 000 runs: one to three components split per labelling).
__device__ static inline void cc_union(u32 *parent, u32 a, u32 b)
{
    while (true) {
        a = cc_find_compress(parent, a);
        b = cc_find_compress(parent, b);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }       // a > b: hook a under b
        if (atomicCAS(parent + a, a, b) == a) return;       // a was still a root: hooked
    }                                                       // somebody hooked a first: look again from where it points now
}

// 0-based component of a run once the trees are flat and the roots are numbered (a parent above its run cannot be: the run
// stands for itself then, and nothing is read outside the tables)
__device__ static inline u32 cc_component(const u32 *__restrict__ parent, const u32 *__restrict__ rank, u32 run)
{
    const u32 p = parent[run];
    return rank[p < run ? p : run];
}

// ---------------------------------------------------------------------------------------------- the keep rule
// one workgroup: tot[3] = label of the largest component with at least min_voxels voxels, the lowest label among equals; 0: none
// (the size of component c is sizes[STRIDE * c]: 1 for the sizes table, CC_COLS for column 0 of the measurement table)
template <int STRIDE>
__global__ __launch_bounds__(1024) void cc_largest_kernel(const unsigned long long *__restrict__ sizes, u64 *tot, int64_t cap,
                                                          int64_t cap_runs, u64 min_voxels)
{
    __shared__ u64 bs[16];
    __shared__ u64 bl[16];
    u64 n = tot[1];
    if (n > (u64)cap || tot[0] > (u64)cap_runs) n = 0;
    u64 best = 0, lab = 0;                                  // lab 0: nothing yet
    for (u64 c = threadIdx.x; c < n; c += 1024) {           // ascending labels: a later equal size never replaces
        const u64 s = sizes[STRIDE * c];
        if (s >= min_voxels && s > 0 && (lab == 0 || s > best)) { best = s; lab = c + 1; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 os = __shfl_xor(best, d, 64), ol = __shfl_xor(lab, d, 64);
        if (ol != 0 && (lab == 0 || os > best || (os == best && ol < lab))) { best = os; lab = ol; }
    }
    if ((threadIdx.x & 63) == 0) { bs[threadIdx.x >> 6] = best; bl[threadIdx.x >> 6] = lab; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++)
            if (bl[w] != 0 && (lab == 0 || bs[w] > best || (bs[w] == best && bl[w] < lab))) { best = bs[w]; lab = bl[w]; }
        tot[3] = lab;
    }
}

// ---------------------------------------------------------------------------------------------- per word: which run is a bit in?
// runs that start in the words of the row in front of word wj, + the row's first run id
__device__ static inline u32 cc_before(const u64 *__restrict__ row, int nx, int wx, int wj, u32 first)
{
    for (int w = 0; w < wj; w++) first += (u32)__popcll(cc_starts(row, nx, wx, w, cc_word(row, nx, wx, w)));
    return first;
}

// bit b of a word belongs to run before + popcount(starts & bits 0 .. b) - 1, before = cc_before and starts = cc_starts of the
// word (a run that came in from the word before has no start bit here)
__device__ static inline u32 cc_run_at(u32 before, u64 starts, int bit)
{
    return before + (u32)__popcll(starts & (~0ull >> (63 - bit))) - 1;
}

// the run of the SET bit `bit` of word wj of a row whose first run has the id `first`
__device__ static inline u32 cc_run_of_bit(const u64 *__restrict__ row, int nx, int wx, int wj, int bit, u32 first)
{
    return cc_run_at(cc_before(row, nx, wx, wj, first), cc_starts(row, nx, wx, wj, cc_word(row, nx, wx, wj)), bit);
}

// The runs that touch ONE word, in ascending x.  Set m = the word, carry = the word before ended inside a run, next = the id of
// the next run that STARTS (cc_before for a word on its own; it carries on from word to word of a row); every
// cc_word_runs_next that returns true leaves the run's bits of this word in mask and its id in run.
struct CcWordRuns {
    u64 m;
    u32 next;
    bool carry;
    u64 mask;
    u32 run;
};

__device__ static inline bool cc_word_runs_next(CcWordRuns &it)
{
    if (!it.m) return false;                                // every turn clears at least one bit of m
    const int s = __ffsll((long long)it.m) - 1;
    const u64 z = ~(it.m >> s);                             // bit k: position s + k is clear (the shift brings zeros in from the top)
    const int len = z ? __ffsll((long long)z) - 1 : 64;
    it.mask = len >= 64 ? ~0ull : ((1ull << len) - 1) << s;
    it.run = (s == 0 && it.carry) ? it.next - 1 : it.next++;
    it.m &= ~it.mask;
    return true;
}

// the runs of word wj of the row r whose first run has the id `first`; m: the word, tail bits clear
__device__ static inline CcWordRuns cc_word_runs(const u64 *__restrict__ r, int nx, int wx, int wj, u64 m, u32 first)
{
    return {m, cc_before(r, nx, wx, wj, first), wj > 0 && (r[wj - 1] >> 63) != 0, 0, 0};
}

// ---------------------------------------------------------------------------------------------- the selected row
// A selected component c writes row slot[c] of a compacted result of cap_sel rows (sel, slot, tot[5]: tomo_cc_select).  Does the
// selection fit -- tot[5] rows in cap_sel, tot[1] components in cap, and `room` for what else the kernel needs (a histogram)?  If
// not, nothing is written at all and the ONE thread of the grid that `speaks` raises CC_F_CAP.
__device__ static inline bool cc_sel_fits(const u64 *__restrict__ tot, int64_t cap, int64_t cap_sel, bool speaks, u64 *flags,
                                          bool room = true)
{
    const bool fits = room && tot[5] <= (u64)cap_sel && tot[1] <= (u64)cap;
    if (speaks && !fits) cc_flag(flags, CC_F_CAP);
    return fits;
}

// Is component c (below the count of components) selected, and which row k is its own?  A row outside the result is CC_F_RANGE
// (speaks: every thread that finds one, or one lane for a wave that asks together).
__device__ static inline bool cc_sel_row(const uint8_t *__restrict__ sel, const u32 *__restrict__ slot, int64_t cap_sel, int64_t c,
                                         bool speaks, u64 *flags, u32 &k)
{
    if (!sel[c]) return false;
    k = slot[c];
    if ((int64_t)k < cap_sel) return true;
    if (speaks) cc_flag(flags, CC_F_RANGE);
    return false;
}

// One thread per component c: both questions, thread 0 speaks for the grid.  The per-word kernels ask cc_sel_fits once per thread
// and cc_sel_row per run.
__device__ static inline bool cc_selected(const u64 *__restrict__ tot, int64_t cap, const uint8_t *__restrict__ sel,
                                          const u32 *__restrict__ slot, int64_t cap_sel, int64_t c, u64 *flags, u32 &k,
                                          bool room = true)
{
    if (!cc_sel_fits(tot, cap, cap_sel, c == 0, flags, room) || c >= cc_ncomp(tot, cap)) return false;
    return cc_sel_row(sel, slot, cap_sel, c, true, flags, k);
}

// The ROW WRITER: one thread per component, a selected one writes the Writer::COLS columns of its row -- tomo_cc_value_rows,
// tomo_cc_topology_rows, tomo_profile_rows.  A new compacted result is a writer: COLS, the arrays it reads, and
//   void write(u64 *o, int64_t c) const     the columns of component c (0-based) into its row o
struct CcRowsArgs {
    const u64 *tot;
    int64_t cap;
    const uint8_t *sel;
    const u32 *slot;
    u64 *out;
    int64_t cap_sel;
    u64 *flags;
};

template <class Writer>
__global__ __launch_bounds__(CC_THREADS) void cc_rows_kernel(Writer w, CcRowsArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    u32 k;
    if (!cc_selected(a.tot, a.cap, a.sel, a.slot, a.cap_sel, c, a.flags, k)) return;
    w.write(a.out + Writer::COLS * (int64_t)k, c);
}

// ok: what the entry point asks of the writer's arrays (TOMO_E_ARG); the sizes come after every argument
template <class Writer>
static int cc_rows_launch(const Writer &w, bool ok, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                          int64_t *out, int64_t cap_sel, void *stream)
{
    if (!ok || !tot || !sel || !slot || !out || cap <= 0 || cap_sel <= 0) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const CcRowsArgs a = {(const u64 *)tot, cap, sel, (const u32 *)slot, (u64 *)out, cap_sel, (u64 *)tot + 2};
    hipLaunchKernelGGL(cc_rows_kernel<Writer>, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream, w, a);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- the word pass
// One wave per 64-bit word of a row, one lane per bit, for what a per-voxel array gives per component (component_measures.hip:
// the value passes and the level histogram; profile.hip): the array is read in whole rows, the runs that touch the word are
// walked by all lanes together.  One kernel (cc_word_kernel), one launcher (cc_word_launch); a reduction is its PASS, below.
struct CcWordAt {
    int64_t row;                                            // z * ny + y
    int wj, bit;                                            // the word of the row, the lane's bit: x = 64 * wj + bit
    u64 cur;                                                // the word, tail bits clear
    CcWordRuns it;                                          // its runs
};

__device__ static inline u64 cc_load64(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct CcWordArgs {                                         // (the counter block is an argument of its own: see cc_word_kernel)
    const u64 *bits;
    int64_t nwords;
    int ny, nx, wx;
    const u32 *row_off;
    int64_t cap_runs;
    const u32 *parent, *rank;
    int64_t cap;
    u64 *flags;
};

// -> false: the wave has no word, or a word without a set bit (wave-uniform)
__device__ static inline bool cc_word_at(const CcWordArgs &a, CcWordAt &w)
{
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int64_t word = t >> 6;                            // the same for the 64 lanes of a wave
    if (word >= a.nwords) return false;
    w.row = word / a.wx;
    w.wj = (int)(word - w.row * a.wx);
    w.bit = (int)(t & 63);
    const u64 *r = a.bits + w.row * a.wx;
    w.cur = cc_word(r, a.nx, a.wx, w.wj);
    if (!w.cur) return false;
    w.it = cc_word_runs(r, a.nx, a.wx, w.wj, w.cur, a.row_off[w.row]);
    return true;
}

struct CcClear {                                            // `bytes` bytes at `array` are set to `byte` before the launch
    void *array;
    int byte;
    size_t bytes;
};

// The kernel owns the front: CC_F_CAP from thread 0 of workgroup 0 (raised even where the first wave has no word), the word and
// its runs (a wave without a word, or with an empty one, leaves before the map is read), the counts, CC_F_RANGE for a run id
// outside the tables, the component of a run, the components beyond the tables skipped.  A PASS says the rest:
//   Lane                     what a lane holds while the runs are walked
//   SELECTED, sel            only the components with sel[c] count
//   bool fits(tot) const     room the pass needs besides the tables: false -> CC_F_CAP and nothing is touched
//   Lane load(a, tot, w, set, at) const     before the run loop, every lane of the wave: the voxel `at` of the map, read if `set`
//   void run(a, w, c, mine, lane, at) const   one run of the word, wave-uniform component c (0-based); mine: the lane's bit is the run's
//   bool ok(bits) const      host: what the entry point asks of the pass's own arguments, aliasing included
//   std::array<CcClear, N> clears(cap) const   host: the arrays cleared before the launch, and to what
// A pass sends at most one atomic per run and array, and only what beats a plain load of the cell (cc_load, cc_load64).
// tot is a const __restrict__ ARGUMENT, not a member of the struct: only so does the compiler take the counts for invariant
// behind the atomicOr of cc_flag and read them with scalar loads BEHIND the word, next to the loads of the map.  As a member they
// are vector loads (counts in VGPRs, vector compares per run); read in front of the word every wave waits for them first.  Both
// cost the value passes 8 to 13 % where nearly every word is set (profiles/r42_word_front.md).
template <class Pass>
__global__ __launch_bounds__(CC_THREADS) void cc_word_kernel(CcWordArgs a, const u64 *__restrict__ tot, Pass p)
{
    const bool fits = p.fits(tot);
    if (blockIdx.x == 0 && threadIdx.x == 0 && (!fits || tot[1] > (u64)a.cap)) cc_flag(a.flags, CC_F_CAP);
    if (!fits) return;
    CcWordAt w;
    if (!cc_word_at(a, w)) return;
    const u32 nruns = (u32)cc_count(tot, a.cap_runs), ncomp = (u32)cc_ncomp(tot, a.cap);
    const bool set = (w.cur >> w.bit) & 1;
    const int64_t at = w.row * a.nx + 64 * w.wj + w.bit;    // a set bit lies below nx: inside the map
    const typename Pass::Lane lane = p.load(a, tot, w, set, at);
    while (cc_word_runs_next(w.it)) {                       // wave-uniform
        if (w.it.run >= nruns) {
            if (w.bit == 0) cc_flag(a.flags, CC_F_RANGE);
            continue;
        }
        const u32 c = cc_component(a.parent, a.rank, w.it.run);
        if (c >= ncomp) continue;                           // more components than the tables hold: CC_F_CAP, above
        if constexpr (Pass::SELECTED) {
            if (!p.sel[c]) continue;
        }
        p.run(a, w, c, (w.it.mask >> w.bit) & 1, lane, at);
    }
}

// the clears, the grid of one wave per word, the launch: for an entry point that has made its checks (nwords < 2^31: cc_geometry)
template <class Pass>
static int cc_word_go(const uint64_t *bits, int64_t nrows, int ny, int nx, int wx, const uint32_t *row_off, int64_t cap_runs,
                      const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap, const Pass &p, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    for (const CcClear &c : p.clears(cap))
        if (hipMemsetAsync(c.array, c.byte, c.bytes, st) != hipSuccess) return TOMO_E_LAUNCH;
    const int64_t nwords = nrows * wx;                      // the grid has fewer than 2^29 workgroups
    const CcWordArgs a = {(const u64 *)bits, nwords, ny, nx, wx, (const u32 *)row_off, cap_runs, (const u32 *)parent, (const u32 *)rank,
                          cap, (u64 *)tot + 2};
    hipLaunchKernelGGL(cc_word_kernel<Pass>, dim3((unsigned)ceil_div64(nwords * 64, CC_THREADS)), dim3(CC_THREADS), 0, st, a,
                       (const u64 *)tot, p);
    return tomo_status();
}

// The checks of a word pass over the run tables: the geometry, then the arguments (TOMO_E_ARG; p.ok: what the pass asks of its
// own), then the sizes (TOMO_E_SIZE).  tomo_cc_level_hist makes cc_hist_check's instead and calls cc_word_go.
template <class Pass>
static int cc_word_launch(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                          const uint32_t *rank, unsigned long long *tot, int64_t cap, const Pass &p, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!p.ok(bits) || !row_off || !parent || !rank || !tot || cap_runs <= 0 || cap <= 0) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    return cc_word_go(bits, nrows, ny, nx, wx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

// ---------------------------------------------------------------------------------------------- the row pass
// One thread per row adds up what the row gives per component: neighbouring runs of one component first, flushed to the
// tables when the component changes; then a wave whose lanes all hold the same component combines and flushes once (one solid
// body: one set of atomics per 64 rows).  What is added up, how it combines and which atomics flush it, checked against which
// bound, is the kernel's ACCUMULATOR:
//   bool any() const              something has been added up since begin
//   u32 begin(u32 c, ...)         start afresh for component c (1-based) -> c, or 0 to refuse it
//   void add(...)                 (the arguments are the CcRuns at the run, in cc_row_walk)
//   void flush(u32 c) const       one lane's own, into component c (0-based)
//   W combine(bool mine, u32 zz) const    the sum over the lanes with `mine`, for slice zz: again has any() and flush(c)
//   u32 filter(u32 c) const       FILTER only: c if the component is counted at all, else 0

// the component changed: flush what was added up, then start afresh
template <class Acc, class... At>
__device__ static inline u32 cc_change(u32 &comp, u32 c, Acc &acc, const At &...at)
{
    if (c != comp) {
        if (acc.any()) acc.flush(comp - 1);
        comp = c = acc.begin(c, at...);
    }
    return c;
}

// the runs of one row -> the component + 1 the thread is left adding up.  A run id outside the tables stops the walk.
template <bool FILTER, class Acc>
__device__ static inline u32 cc_row_walk(const u64 *__restrict__ bits, int64_t row, int nx, int wx, const u32 *__restrict__ row_off,
                                         u32 nruns, const u32 *__restrict__ parent, const u32 *__restrict__ rank, u64 *flags, Acc &acc)
{
    u32 comp = 0;
    CcRuns a = cc_runs_begin(bits, row, nx, wx);
    u32 ia = row_off[row];
    while (a.valid) {
        if (ia >= nruns) {
            cc_flag(flags, CC_F_RANGE);
            break;
        }
        u32 c = cc_component(parent, rank, ia) + 1;
        if constexpr (FILTER) c = acc.filter(c);
        c = cc_change(comp, c, acc, a);
        if (!FILTER || c) acc.add(a);
        cc_runs_next(a);
        ia++;
    }
    return comp;
}

// The wave tail.  comp: the component + 1 the lane holds, z: the slice of its row.  SLICED: the lanes combine once per slice
// the wave's rows lie in -- mostly one, more where the wave straddles slices (ny < 64) -- otherwise once, whatever the slices.
template <bool SLICED, class Acc>
__device__ static inline void cc_wave_tail(u32 comp, u32 z, const Acc &acc)
{
    if (!acc.any()) comp = 0;
    const u32 top = wave_max32(comp);
    if (top == 0) return;                                   // wave-uniform
    if (__all(comp == 0 || comp == top)) {
        const u32 zlo = SLICED ? wave_min32(comp ? z : ~0u) : 0u, zhi = SLICED ? wave_max32(comp ? z : 0u) : 0u;
        for (u32 zz = zlo; zz <= zhi; zz++) {               // wave-uniform bounds: at most 64 slices hold the wave's 64 rows
            const auto w = acc.combine(comp != 0 && (!SLICED || z == zz), zz);
            if ((threadIdx.x & 63) == 0 && w.any()) w.flush(top - 1);
        }
    } else if (comp != 0) {
        acc.flush(comp - 1);
    }
}

// the simplest accumulator: one u64 per component, out[c] += sum while c < bound (a two's complement sum may cancel to 0)
struct CcSumAcc {
    unsigned long long *out;
    u32 bound;
    u64 sum;
    __device__ bool any() const { return sum != 0; }
    template <class... At>
    __device__ u32 begin(u32 c, const At &...) { sum = 0; return c; }
    __device__ void add(const CcRuns &a) { sum += (u64)(a.e - a.s); }
    __device__ void flush(u32 c) const { if (c < bound) atomicAdd(out + c, (unsigned long long)sum); }
    __device__ CcSumAcc combine(bool mine, u32) const { return {out, bound, wave_sum64(mine ? sum : 0)}; }
};

// ---------------------------------------------------------------------------------------------- the per-slice histograms
#define CC_SURF 11                   // counters per component and slice of tomo_cc_surface_hist and tomo_branch_hist
#define CC_SURF_CLASSES 7            // x, y, xy, z, xz, yz, xyz: the counters with up and down folded
#define CC_BREADTH 18                // words per component and slice of tomo_cc_breadth_hist: CC_BREADTH_IN raw counts of the cells
#define CC_BREADTH_IN 6              //   inside the slice, then the signed cross parts of the families but (1, 0, 0)
#define CC_BREADTH_FAMILIES 13       // families of lattice planes: the columns of section_euler

struct CcHist {
    const u64 *table, *off;                                 // both NULL: the whole volume is component 0, one entry per slice
    u64 *hist;
    u64 total;                                              // entries of the histogram
    u64 *flags;
};

// hist[SUMS * (off[c] + z - zmin[c]) + k] += v[k]: checked against the component's box and the histogram's length before the adds
template <int SUMS>
__device__ static inline void cc_hist_add(const CcHist &h, u32 c, u32 z, const u64 (&v)[SUMS])
{
    const u64 z0 = h.table ? h.table[(int64_t)c * CC_COLS + 1] : 0ull, z1 = h.table ? h.table[(int64_t)c * CC_COLS + 2] : h.total - 1;
    const u64 pos = (h.off ? h.off[c] : 0ull) + ((u64)z - z0);
    if (z < z0 || z > z1 || pos >= h.total) {
        cc_flag(h.flags, CC_F_RANGE);
        return;
    }
#pragma unroll
    for (int k = 0; k < SUMS; k++)
        if (SUMS == 1 || v[k]) atomicAdd(h.hist + SUMS * pos + k, v[k]);
}

// has anything been counted?  Word 0 answers where every voxel seen counts there; ANY_ALL asks every word
template <bool ANY_ALL, int WORDS>
__device__ static inline bool cc_counted(const u64 (&v)[WORDS])
{
    u64 a = v[0];
    if constexpr (ANY_ALL) {
#pragma unroll
        for (int k = 1; k < WORDS; k++) a |= v[k];
    }
    return a != 0;
}

// what the lanes of a wave hold of one component in slice z, added up
template <int WORDS, bool ANY_ALL = false>
struct CcSliceSum {
    const CcHist &h;
    u32 z;
    u64 v[WORDS];
    __device__ bool any() const { return cc_counted<ANY_ALL>(v); }
    __device__ void flush(u32 c) const { cc_hist_add<WORDS>(h, c, z, v); }
};

// ---------------------------------------------------------------------------------------------- the window walk
struct CcWin {                                               // three neighbouring words of one row, slid along x
    u64 prv, cur, nxt;
};

__device__ static inline u64 cc_word_or0(const u64 *__restrict__ row, int nx, int wx, int w)
{
    return (row && w < wx) ? cc_word(row, nx, wx, w) : 0ull;
}

__device__ static inline u64 cc_xp(const CcWin &r) { return (r.cur >> 1) | (r.nxt << 63); }      // bit x = voxel x + 1
__device__ static inline u64 cc_xm(const CcWin &r) { return (r.cur << 1) | (r.prv >> 63); }      // bit x = voxel x - 1

// The WINDOW WALK: the row pass for what a voxel's neighbours decide.  One thread per row (z, y) slides CcWin windows of the row
// r[0] and of NR - 1 neighbour rows along x (r[i] == NULL: a row outside the stack, it reads as 0) and, LABELLED, walks the runs
// in every word (as cc_filter_kernel walks them): neighbouring runs of one component are added up, flushed when the component
// changes -> the component + 1 the thread is left adding up.  Not LABELLED: no table is read, everything is component 1.  The
// accumulator is the row pass's with, in place of add(run):
//   void word(const CcWin *win)              a word of the row that holds a set bit: what every run of it shares
//   void add(const CcWin *win, u64 mask)     the bits `mask` of that word belong to the component begun
template <int NR, bool LABELLED, bool FILTER, class Acc>
__device__ static inline u32 cc_window_walk(const u64 *const *r, int nx, int wx, u32 first, u32 nruns,
                                            const u32 *__restrict__ parent, const u32 *__restrict__ rank, u64 *flags, Acc &acc)
{
    u32 comp = 0;
    CcWin win[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) {
        win[i].prv = 0;
        win[i].cur = cc_word_or0(r[i], nx, wx, 0);
        win[i].nxt = cc_word_or0(r[i], nx, wx, 1);
    }
    CcWordRuns it = {0, first, false};
    for (int w = 0; w < wx; w++) {
        const u64 m = win[0].cur;
        if (m) {
            acc.word(win);
            if (!LABELLED) {
                cc_change(comp, 1u, acc);
                acc.add(win, m);
            }
            it.m = LABELLED ? m : 0;
            while (cc_word_runs_next(it)) {
                if (it.run < nruns) {
                    u32 c = cc_component(parent, rank, it.run) + 1;
                    if constexpr (FILTER) c = acc.filter(c);
                    c = cc_change(comp, c, acc);
                    if (!FILTER || c) acc.add(win, it.mask);
                } else {
                    cc_flag(flags, CC_F_RANGE);
                }
            }
        }
        it.carry = (m >> 63) != 0;                          // the word ended inside a run
#pragma unroll
        for (int i = 0; i < NR; i++) {
            win[i].prv = win[i].cur;
            win[i].cur = win[i].nxt;
            win[i].nxt = cc_word_or0(r[i], nx, wx, w + 2);
        }
    }
    return comp;
}

// The rows a window walk reads are a constant list next to the accumulator that indexes win[i]: ROWS[i] = row (z + dz, y + dy) of
// the volume itself (src 0) or of a second volume of the same shape (src 1), NR of them, ROWS[0] the row itself.
struct CcRowAt {
    int dz, dy, src;
};

// self: where row (z, y) starts in the volume named; the step from there to a neighbour row is the same for every thread
template <int DZ, int DY>
__device__ static inline const u64 *cc_row_or_null(const u64 *self, int64_t row, int64_t nrows, int ny, int wx, int y)
{
    const bool inside = (DY < 0 ? y > 0 : DY > 0 ? y + 1 < ny : true) && (DZ < 0 ? row >= ny : DZ > 0 ? row + ny < nrows : true);
    return inside ? self + ((int64_t)DZ * ny + DY) * wx : nullptr;
}

template <class List, int... I>
__device__ static inline void cc_rows_fill(const u64 **r, const u64 *self, const u64 *all, int64_t row, int64_t nrows, int ny, int wx,
                                           int y, std::integer_sequence<int, I...>)
{
    ((r[I] = cc_row_or_null<List::ROWS[I].dz, List::ROWS[I].dy>(List::ROWS[I].src ? all : self, row, nrows, ny, wx, y)), ...);
}

template <class List>
constexpr bool cc_two_volumes()
{
    for (const CcRowAt &at : List::ROWS)
        if (at.src) return true;
    return false;
}

// r[i] = where row List::ROWS[i] of row (z, y) starts, NULL for a row outside the stack (the list is resolved when compiled: r[]
// and the windows stay in registers).  other: the second volume, not read where the list names none.
template <class List>
__device__ static inline void cc_rows(const u64 *(&r)[List::NR], const u64 *bits, const u64 *other, int64_t row, int64_t nrows, int ny,
                                      int wx, int y)
{
    const u64 *all = nullptr;
    if constexpr (cc_two_volumes<List>()) all = other + row * wx;
    cc_rows_fill<List>(r, bits + row * wx, all, row, nrows, ny, wx, y, std::make_integer_sequence<int, List::NR>{});
}

// ---------------------------------------------------------------------------------------------- the histogram pass
// WORDS uint64 per slice of every selected component's box, filed by one thread per row: what tomo_cc_zhist, tomo_cc_moment_hist,
// tomo_cc_surface_hist, tomo_cc_breadth_hist and tomo_branch_hist are.  One kernel, one launcher; a measurement is its accumulator:
//   WORDS                uint64 per entry of the histogram
//   NR, ROWS[NR]         the rows of its window walk (above); NR == 0: it walks the runs (cc_row_walk, add(run))
//   add(...)             what a run, or the bits of a word under a run's mask, count
//   Extra                what its kernel takes besides CcHistArgs (CcOneVolume: nothing)
//   UNLABELLED, WALKS_EMPTY, SQUARES     where the passes differ: the list above cc_hist_launch
// and a finishing kernel that sums a component's slices (component_measures.hip: cc_slices and its callers).  A window walk gets
// everything but add and ROWS from CcCounts.
struct CcHistArgs {
    const u64 *bits;
    int64_t nrows;
    int ny, nx, wx;
    const u32 *row_off;
    const u64 *tot;
    int64_t cap_runs;
    const u32 *parent, *rank;
    const u64 *table;
    int64_t cap;
    const uint8_t *sel;
    const u64 *off;
    u64 *hist;
    int64_t hist_cap;
    u64 *flags;
};

struct CcOneVolume {
    static constexpr const u64 *other = nullptr;
};

// The counters of row (z, y) for a window walk: n[WORDS], zero when a component is begun, popcounts added by the add() of the
// struct that derives from this.  sel == NULL: no labelling, everything counts.  ANY_ALL = false: any() asks n[0], the word that
// counts every voxel seen (surface: every run ends at a clear bit or at the edge of the stack; breadth: the voxels themselves).
// ANY_ALL = true: any() ORs every word -- the branch pass must, a regular voxel whose two neighbours are earlier regular voxels
// counts in none of them.
template <int N, bool ANY_ALL>
struct CcCounts {
    static constexpr int WORDS = N;
    static constexpr bool WALKS_EMPTY = false, SQUARES = false;
    CcHist h;
    const uint8_t *sel;
    u32 ncomp, z;
    u64 n[N];
    __device__ CcCounts(const CcHistArgs &a, u64 total, u32 ncomp, u32 z, u32)
        : h{a.table, a.off, a.hist, total, a.flags}, sel(a.sel), ncomp(ncomp), z(z), n{}
    {
    }
    __device__ u32 filter(u32 c) const { return (c - 1 >= ncomp || !sel[c - 1]) ? 0u : c; }
    __device__ bool any() const { return cc_counted<ANY_ALL>(n); }
    __device__ u32 begin(u32 c)
    {
#pragma unroll
        for (int k = 0; k < N; k++) n[k] = 0;
        return c;
    }
    __device__ void word(const CcWin *) {}
    __device__ CcSliceSum<N, ANY_ALL> combine(bool mine, u32 zz) const
    {
        CcSliceSum<N, ANY_ALL> w = {h, zz, {}};
#pragma unroll
        for (int k = 0; k < N; k++) w.v[k] = wave_sum64(mine ? n[k] : 0);
        return w;
    }
    __device__ void flush(u32 c) const { cc_hist_add<N>(h, c, z, n); }
};

// One thread per row (z, y).  A histogram shorter than the selection's entries, or a table shorter than the components: CC_F_CAP
// and nothing is touched.  Not LABELLED: no table is read, the whole volume is component 1 with one entry per slice.
template <class Acc, bool LABELLED>
__global__ __launch_bounds__(CC_THREADS) void cc_hist_kernel(CcHistArgs a, typename Acc::Extra x)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = LABELLED ? (u32)cc_count(a.tot, a.cap_runs) : 0u;
    const u64 total = LABELLED ? a.tot[4] : (u64)(a.nrows / a.ny);      // no labelling: the host checked hist_cap
    const bool fits = total <= (u64)a.hist_cap;
    const u32 ncomp = !fits ? 0u : LABELLED ? (u32)cc_ncomp(a.tot, a.cap) : 1u;
    if (LABELLED && row == 0 && (!fits || a.tot[1] > (u64)a.cap)) cc_flag(a.flags, CC_F_CAP);
    const bool live = row < a.nrows && (Acc::WALKS_EMPTY || ncomp != 0);
    const u32 z = live ? (u32)(row / a.ny) : 0u, y = live ? (u32)(row % a.ny) : 0u;
    Acc acc(a, total, ncomp, z, y);
    u32 comp = 0;                                           // SELECTED component + 1 the thread is left with, 0: none
    if (live) {
        if constexpr (Acc::NR == 0) {
            comp = cc_row_walk<true>(a.bits, row, a.nx, a.wx, a.row_off, nruns, a.parent, a.rank, a.flags, acc);
        } else {
            const u64 *r[Acc::NR];
            cc_rows<Acc>(r, a.bits, x.other, row, a.nrows, a.ny, a.wx, (int)y);
            comp = cc_window_walk<Acc::NR, LABELLED, LABELLED>(r, a.nx, a.wx, LABELLED ? a.row_off[row] : 0u, nruns, a.parent, a.rank,
                                                               a.flags, acc);
        }
    }
    cc_wave_tail<true>(comp, acc.z, acc);
}

// The checks every histogram entry point makes, tomo_cc_level_hist's word pass included: the geometry, then the arguments
// (TOMO_E_ARG), then the sizes (TOMO_E_SIZE).  ok: what the entry point asks of arguments of its own; words: uint64 per entry, read
// only once ok holds.  unlabelled: the entry point has the form without tables -- parent == NULL, one entry per slice.
static int cc_hist_check(bool unlabelled, const void *bits, int nz, int ny, int nx, const void *row_off, int64_t cap_runs,
                         const void *parent, const void *rank, const void *tot, const void *table, int64_t cap, const void *sel,
                         const void *off, const void *hist, int64_t hist_cap, int64_t words, bool ok, int64_t *nrows, int *wx)
{
    const int g = cc_geometry(bits, nz, ny, nx, nrows, wx);
    if (g != TOMO_OK) return g;
    const bool labelled = parent || !unlabelled;
    if (!ok || !hist || hist_cap <= 0) return TOMO_E_ARG;
    if (labelled && (!row_off || !parent || !rank || !tot || !table || !sel || !off || cap_runs <= 0 || cap <= 0)) return TOMO_E_ARG;
    if (!labelled && hist_cap < nz) return TOMO_E_ARG;
    if (hist_cap >= ((int64_t)1 << 60) / words || (labelled && (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31))))
        return TOMO_E_SIZE;
    return TOMO_OK;
}

// Checks, the histogram zeroed, the launch.  Where the five passes differ, and it is behaviour that stays:
//   Acc::WALKS_EMPTY   the passes over the runs walk a row even with no component to count (a table or a histogram that is too
//                      short), so they can raise CC_F_RANGE where the window walks, which then stop, raise only CC_F_CAP
//   Acc::UNLABELLED    surface and breadth have a form without tables: parent == NULL, one entry per slice, hist_cap >= nz, no
//                      flags; the passes over the runs and the branch pass refuse a null table (TOMO_E_ARG)
//   Acc::SQUARES       the moment sums alone refuse a stack in which a slice's sum of j'^2, i'^2 or j' i' could leave 63 bits
//   ok, x              the branch pass alone takes a second volume, and refuses a histogram that is either volume
//   Acc::WORDS         the bound on hist_cap is 2^60 / WORDS: 2^60 itself for one word
template <class Acc>
static int cc_hist_launch(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                          const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap, const uint8_t *sel,
                          const uint64_t *off, uint64_t *hist, int64_t hist_cap, bool ok, typename Acc::Extra x, void *stream)
{
    int64_t nrows;
    int wx;
    const int r = cc_hist_check(Acc::UNLABELLED, bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, hist,
                                hist_cap, Acc::WORDS, ok, &nrows, &wx);
    if (r != TOMO_OK) return r;
    if constexpr (Acc::SQUARES) {
        const unsigned __int128 side = (unsigned __int128)(ny > nx ? ny : nx);
        if ((unsigned __int128)ny * (unsigned __int128)nx * side * side >= ((unsigned __int128)1 << 63)) return TOMO_E_SIZE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)hist_cap * Acc::WORDS * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    const dim3 grid((unsigned)ceil_div64(nrows, CC_THREADS)), block(CC_THREADS);
    if (parent || !Acc::UNLABELLED) {
        const CcHistArgs a = {(const u64 *)bits, nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs,
                              (const u32 *)parent, (const u32 *)rank, (const u64 *)table, cap, sel, (const u64 *)off, (u64 *)hist,
                              hist_cap, (u64 *)tot + 2};
        hipLaunchKernelGGL((cc_hist_kernel<Acc, true>), grid, block, 0, st, a, x);
    } else if constexpr (Acc::UNLABELLED) {
        const CcHistArgs a = {(const u64 *)bits, nrows, ny, nx, wx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr,
                              (u64 *)hist, hist_cap, nullptr};
        hipLaunchKernelGGL((cc_hist_kernel<Acc, false>), grid, block, 0, st, a, x);
    }
    return tomo_status();
}
