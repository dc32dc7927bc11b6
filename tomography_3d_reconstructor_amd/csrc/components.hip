// components.hip -- connected-component labelling, component sizes and island removal on the resident bit volume
// (scipy.ndimage.label with generate_binary_structure(3, 1) or (3, 3); no counterpart in the reference, whose only defence
// against debris is the opening of voxel_processor.py:88).
//
// The unit of work is the X-RUN, a maximal run of set bits in a row, never the voxel.  Run ids are handed out in raster order
// (exclusive scan of the runs per row), every run starts as its own tree (linked to its first neighbour in the row above, which
// needs no atomic), overlapping runs of neighbouring rows are united by hooking the larger root under the smaller one with
// atomicMin, and the trees are flattened in a launch of their own.  A root is the smallest run id of its component = the
// component's first run in raster order, so numbering the roots with a scan IS scipy's numbering, whatever the schedule did.
// Sizes are integer atomics per component.  Nothing here holds a per-voxel array except tomo_cc_expand's output.
//
// Termination: parent[r] <= r always and a parent only ever decreases (atomicMin, or a store of a smaller ancestor); cc_find
// follows strictly decreasing ids; every turn of cc_union's loop that does not end it lowers a + b.  No kernel waits for
// another workgroup: the phases are separate launches.
//
// tot (device uint64[8]): [0] runs  [1] components  [2] flags (1: 2^31 runs or more, 2: more runs than the caller's buffers
// hold, 4: a run id outside the tables -- the bits changed between the calls)  [3] label tomo_cc_filter(largest) kept (0: none)
// [4] counters of the slice histogram  [5] components tomo_cc_zhist_offsets selected.
#include "tomo_common.h"

#define CC_THREADS 256
#define CC_SCAN_TILE 1024            // entries per workgroup of the scan kernels (4 per thread)
#define CC_F_MANY 1ull
#define CC_F_CAP 2ull
#define CC_F_RANGE 4ull
#define CC_COLS 10                   // columns of a row of the measurement table (tomo_cc_measure)

TOMO_API int64_t tomo_cc_scan_blocks(int64_t n)
{
    if (n <= 0) return TOMO_E_ARG;
    return ceil_div64(n, CC_SCAN_TILE) + 1;
}

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

// row_off[row] = runs of the row (row_off[nrows] = 0): the input of the scan
__global__ __launch_bounds__(CC_THREADS) void cc_row_count_kernel(const u64 *__restrict__ bits, int64_t nrows, int nx, int wx,
                                                                  u32 *__restrict__ row_off)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (row > nrows) return;
    u32 c = 0;
    if (row < nrows) {
        const u64 *r = bits + row * wx;
        for (int w = 0; w < wx; w++) c += (u32)__popcll(cc_starts(r, nx, wx, w, cc_word(r, nx, wx, w)));
    }
    row_off[row] = c;
}

// ---------------------------------------------------------------------------------------------- exclusive scan of u32, in place
// n comes from the host (n_dev == NULL) or from device memory, clipped to the capacity the grid was sized for
__device__ static inline int64_t cc_count(const u64 *n_dev, int64_t cap)
{
    if (!n_dev) return cap;
    const u64 n = *n_dev;
    return n > (u64)cap ? 0 : (int64_t)n;                  // too many for the buffers: nothing is touched (flag CC_F_CAP)
}

__global__ __launch_bounds__(CC_THREADS) void cc_blocksum_kernel(const u32 *__restrict__ v, const u64 *n_dev, int64_t cap,
                                                                 u64 *__restrict__ blk)
{
    __shared__ u32 wsum[CC_THREADS / 64];
    const int64_t n = cc_count(n_dev, cap);
    const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + 4 * threadIdx.x;
    u32 acc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) acc += i0 + j < n ? v[i0 + j] : 0u;
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = (u64)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: blk[i] = sum of blk[0 .. i) for i < nblk, *total = the sum of all; 1024 entries per step with a running carry
__global__ __launch_bounds__(1024) void cc_scan1_kernel(u64 *__restrict__ blk, int64_t nblk, u64 *__restrict__ total, u64 *flags)
{
    __shared__ u64 wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (int64_t i0 = 0; i0 < nblk; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const u64 v = i < nblk ? blk[i] : 0;
        u64 inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
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

__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(u32 *__restrict__ v, const u64 *n_dev, int64_t cap,
                                                              const u64 *__restrict__ blk)
{
    __shared__ u32 wsum[CC_THREADS / 64];
    const int64_t n = cc_count(n_dev, cap);
    const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + 4 * threadIdx.x;
    u32 x[4];
    u32 acc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        x[j] = i0 + j < n ? v[i0 + j] : 0u;
        acc += x[j];
    }
    const u32 inc = wave_inclusive_scan(acc);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    u32 before = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) before += wsum[w];
    u32 run = (u32)blk[blockIdx.x] + before + inc - acc;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n) v[i0 + j] = run;
        run += x[j];
    }
}

static void cc_scan(u32 *v, const u64 *n_dev, int64_t cap, u64 *blk, u64 *total, u64 *flags, hipStream_t st)
{
    const int64_t nblk = ceil_div64(cap, CC_SCAN_TILE);
    hipLaunchKernelGGL(cc_blocksum_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, (const u32 *)v, n_dev, cap, blk);
    hipLaunchKernelGGL(cc_scan1_kernel, dim3(1), dim3(1024), 0, st, blk, nblk, total, flags);
    hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, v, n_dev, cap, (const u64 *)blk);
}

static int cc_geometry(const void *bits, int nz, int ny, int nx, int64_t *nrows, int *wx)
{
    if (!bits || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    *wx = (int)tomo_words_per_row(nx);
    *nrows = (int64_t)nz * ny;
    if (*nrows * *wx >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    return TOMO_OK;
}

TOMO_API int tomo_cc_count_runs(const uint64_t *bits, int nz, int ny, int nx, uint32_t *row_off, uint64_t *blk,
                                unsigned long long *tot, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !blk || !tot) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(tot, 0, 8 * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_row_count_kernel, dim3((unsigned)ceil_div64(nrows + 1, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u64 *)bits, nrows, nx, wx, (u32 *)row_off);
    cc_scan((u32 *)row_off, NULL, nrows + 1, (u64 *)blk, (u64 *)tot, (u64 *)tot + 2, st);
    return tomo_status();
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

__device__ static inline void cc_union(u32 *parent, u32 a, u32 b)
{
    while (true) {
        a = cc_find_compress(parent, a);
        b = cc_find_compress(parent, b);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }       // a > b: hook a under b
        const u32 old = atomicMin(parent + a, b);
        if (old >= a) return;                               // a was a root: hooked (old == a; > a cannot be)
        a = old;                                            // somebody hooked a first, under old < a: unite old and b
    }
}

// 0-based component of a run once the trees are flat and the roots are numbered (a parent above its run cannot be: the run
// stands for itself then, and nothing is read outside the tables)
__device__ static inline u32 cc_component(const u32 *__restrict__ parent, const u32 *__restrict__ rank, u32 run)
{
    const u32 p = parent[run];
    return rank[p < run ? p : run];
}

// The runs of `row` against the runs of the neighbour row `nb` (widen = 1: diagonal neighbours count, connectivity 26).
// mode 0: parent[a] = the FIRST run of nb that touches a (or a itself) -- plain stores, every run is written exactly once, by
//         this thread; only for the row above in the same slice;  mode 1: unite with every touching run but the first (what
//         mode 0 left to do);  mode 2: unite with every touching run.
template <int MODE>
__device__ static inline void cc_pair_rows(const u64 *__restrict__ bits, int nx, int wx, int64_t row, int64_t nb,
                                           const u32 *__restrict__ row_off, u32 nruns, int widen, u32 *parent, u64 *flags)
{
    CcRuns a = cc_runs_begin(bits, row, nx, wx);
    u32 ia = row_off[row], ib = 0;
    CcRuns b;
    b.valid = false;
    if (nb >= 0) {
        b = cc_runs_begin(bits, nb, nx, wx);
        ib = row_off[nb];
    }
    bool linked = false;
    while (a.valid) {                                       // every turn moves a or b on: at most runs(a) + runs(b) turns
        if (ia >= nruns || (b.valid && ib >= nruns)) {
            atomicOr((unsigned long long *)flags, CC_F_RANGE);
            return;
        }
        bool next_a = true;
        if (b.valid) {
            if (a.s < b.e + widen && b.s < a.e + widen) {
                if (MODE == 0) {
                    if (!linked) parent[ia] = ib;
                } else if (MODE == 2 || linked) {
                    cc_union(parent, ia, ib);
                }
                linked = true;
            }
            next_a = a.e <= b.e;
        }
        if (next_a) {
            if (MODE == 0 && !linked) parent[ia] = ia;
            cc_runs_next(a);
            ia++;
            linked = false;
        } else {
            cc_runs_next(b);
            ib++;
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                             const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                             int widen, u32 *__restrict__ parent, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (row >= nrows) return;
    const u32 nruns = (u32)cc_count(tot, cap);
    if (row == 0 && tot[0] > (u64)cap) atomicOr((unsigned long long *)flags, CC_F_CAP);
    const int y = (int)(row % ny);
    cc_pair_rows<0>(bits, nx, wx, row, y > 0 ? row - 1 : -1, row_off, nruns, widen, parent, flags);
}

__global__ __launch_bounds__(CC_THREADS) void cc_union_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                              const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                              int widen, u32 *parent, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (row >= nrows) return;
    const u32 nruns = (u32)cc_count(tot, cap);
    const int y = (int)(row % ny);
    const bool below = row >= ny;                           // there is a slice z - 1
    if (y > 0) cc_pair_rows<1>(bits, nx, wx, row, row - 1, row_off, nruns, widen, parent, flags);
    if (below) {
        cc_pair_rows<2>(bits, nx, wx, row, row - ny, row_off, nruns, widen, parent, flags);
        if (widen) {
            if (y > 0) cc_pair_rows<2>(bits, nx, wx, row, row - ny - 1, row_off, nruns, widen, parent, flags);
            if (y + 1 < ny) cc_pair_rows<2>(bits, nx, wx, row, row - ny + 1, row_off, nruns, widen, parent, flags);
        }
    }
}

// parent[r] = its root.  mark: rank[r] = 1 for a root, 0 otherwise (the input of the numbering scan)
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(u32 *parent, const u64 *__restrict__ tot, int64_t cap, u32 *__restrict__ rank)
{
    const int64_t r = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (r >= cc_count(tot, cap)) return;
    const u32 root = cc_find(parent, (u32)r);
    if (root != (u32)r) __hip_atomic_store(parent + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // smaller than what was there
    if (rank) rank[r] = root == (u32)r ? 1u : 0u;
}

// sizes[c] += voxels of the runs of component c = rank[parent[run]]; a thread adds up neighbouring runs of one component
// first, a wave whose lanes all hold the same component adds once (one solid body: one atomic per 64 rows)
__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const u64 *__restrict__ bits, int64_t nrows, int nx, int wx,
                                                              const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                              const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                              unsigned long long *__restrict__ sizes, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap);
    u32 comp = 0;                                           // component + 1 the thread is adding up, 0: none
    u64 acc = 0;
    if (row < nrows) {
        CcRuns a = cc_runs_begin(bits, row, nx, wx);
        u32 ia = row_off[row];
        while (a.valid) {
            if (ia >= nruns) {
                atomicOr((unsigned long long *)flags, CC_F_RANGE);
                break;
            }
            const u32 c = cc_component(parent, rank, ia) + 1;
            if (c != comp) {
                if (acc && comp - 1 < nruns) atomicAdd(sizes + (comp - 1), (unsigned long long)acc);
                comp = c;
                acc = 0;
            }
            acc += (u64)(a.e - a.s);
            cc_runs_next(a);
            ia++;
        }
    }
    if (!acc) comp = 0;
    u32 top = comp;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = __shfl_xor(top, d, 64);
        top = o > top ? o : top;
    }
    if (top == 0) return;                                   // wave-uniform
    if (__all(comp == 0 || comp == top)) {
        const u64 sum = wave_sum64(acc);
        if ((threadIdx.x & 63) == 0 && top - 1 < nruns) atomicAdd(sizes + (top - 1), (unsigned long long)sum);
    } else if (acc && comp - 1 < nruns) {
        atomicAdd(sizes + (comp - 1), (unsigned long long)acc);
    }
}

TOMO_API int tomo_cc_label_runs(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const uint32_t *row_off,
                                int64_t cap_runs, uint32_t *parent, uint32_t *rank, int64_t *sizes, uint64_t *blk,
                                unsigned long long *tot, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !sizes || !blk || !tot || cap_runs <= 0 || (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const int widen = connectivity == 26 ? 1 : 0;
    const unsigned row_blocks = (unsigned)ceil_div64(nrows, CC_THREADS), run_blocks = (unsigned)ceil_div64(cap_runs, CC_THREADS);
    const u64 *t = (const u64 *)tot;
    u64 *flags = (u64 *)tot + 2;
    if (hipMemsetAsync(sizes, 0, (size_t)cap_runs * sizeof(int64_t), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_init_kernel, dim3(row_blocks), dim3(CC_THREADS), 0, st, (const u64 *)bits, nrows, ny, nx, wx,
                       (const u32 *)row_off, t, cap_runs, widen, (u32 *)parent, flags);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(run_blocks), dim3(CC_THREADS), 0, st, (u32 *)parent, t, cap_runs, (u32 *)nullptr);
    hipLaunchKernelGGL(cc_union_kernel, dim3(row_blocks), dim3(CC_THREADS), 0, st, (const u64 *)bits, nrows, ny, nx, wx,
                       (const u32 *)row_off, t, cap_runs, widen, (u32 *)parent, flags);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(run_blocks), dim3(CC_THREADS), 0, st, (u32 *)parent, t, cap_runs, (u32 *)rank);
    cc_scan((u32 *)rank, t, cap_runs, (u64 *)blk, (u64 *)tot + 1, nullptr, st);
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(row_blocks), dim3(CC_THREADS), 0, st, (const u64 *)bits, nrows, nx, wx,
                       (const u32 *)row_off, t, cap_runs, (const u32 *)parent, (const u32 *)rank, (unsigned long long *)sizes, flags);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- per word: which run is bit b in?
// runs that start in the words of the row in front of word wj, + the row's first run id: bit b of the word belongs to run
// cc_before + popcount(starts & bits 0 .. b) - 1 (a run that came in from the word before has no start bit here)
__device__ static inline u32 cc_before(const u64 *__restrict__ row, int nx, int wx, int wj, u32 first)
{
    for (int w = 0; w < wj; w++) first += (u32)__popcll(cc_starts(row, nx, wx, w, cc_word(row, nx, wx, w)));
    return first;
}

// MAP: the label of 0-based component c is map[c] (c < nmap), not c + 1 -- the global labels of one Z-slab
template <bool MAP>
__global__ __launch_bounds__(CC_THREADS) void cc_expand_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                               const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                               const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                               const int32_t *__restrict__ map, u32 nmap,
                                                               int32_t *__restrict__ labels, u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;       // the word of this lane
    const int lane = threadIdx.x & 63;
    const u32 nruns = (u32)cc_count(tot, cap);
    u64 cur = 0, starts = 0;
    u32 before = 0;
    int64_t row = 0;
    int wj = 0;
    if (i < nwords) {
        row = i / wx;
        wj = (int)(i - row * wx);
        const u64 *r = bits + row * wx;
        cur = cc_word(r, nx, wx, wj);
        starts = cc_starts(r, nx, wx, wj, cur);
        before = cc_before(r, nx, wx, wj, row_off[row]);
    }
    // the 64 words of the wave one after the other: lane b writes voxel b of the word (256 contiguous bytes per store)
    const int64_t wave0 = i - lane;
    for (int j = 0; j < 64; j++) {
        if (wave0 + j >= nwords) break;                     // wave-uniform
        const u64 c = __shfl(cur, j, 64), s = __shfl(starts, j, 64);
        const u32 bf = __shfl(before, j, 64);
        const int64_t rj = __shfl(row, j, 64);
        const int x = 64 * __shfl(wj, j, 64) + lane;
        if (x < nx) {                                       // no lane leaves the loop early: the shuffles need all 64
            int32_t lab = 0;
            if ((c >> lane) & 1) {
                const u32 run = bf + (u32)__popcll(s & (~0ull >> (63 - lane))) - 1;
                const u32 c = run < nruns ? cc_component(parent, rank, run) : ~0u;
                if (run < nruns && (!MAP || c < nmap)) lab = MAP ? map[c] : (int32_t)(c + 1);
                else atomicOr((unsigned long long *)flags, CC_F_RANGE);
            }
            labels[rj * nx + x] = lab;
        }
    }
}

TOMO_API int tomo_cc_expand(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                            const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int32_t *labels, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !labels || cap_runs <= 0) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;
    hipLaunchKernelGGL(cc_expand_kernel<false>, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, (const int32_t *)nullptr, 0u, labels, (u64 *)tot + 2);
    return tomo_status();
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

// out word = the bits of the word's runs whose component is kept (MAP: kept = map[c] != 0 for c < nmap, whatever the sizes say)
template <bool MAP>
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                               const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                               const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                               const unsigned long long *__restrict__ sizes, u64 min_voxels, int largest,
                                                               const uint8_t *__restrict__ map, u32 nmap, u64 *__restrict__ out, u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= nwords) return;
    const u32 nruns = (u32)cc_count(tot, cap);
    const u64 only = !MAP && largest ? tot[3] : 0;
    const int64_t row = i / wx;
    const int wj = (int)(i - row * wx);
    const u64 *r = bits + row * wx;
    u64 m = cc_word(r, nx, wx, wj);
    u64 res = 0;
    if (m) {
        const bool carry = wj > 0 && (r[wj - 1] >> 63);
        u32 next = cc_before(r, nx, wx, wj, row_off[row]);   // id of the next run that STARTS in this word
        while (m) {                                         // every turn clears at least one bit of m
            const int s = __ffsll((long long)m) - 1;
            const u64 z = ~(m >> s);                        // bit k: position s + k is clear (the shift brings zeros in from the top)
            const int len = z ? __ffsll((long long)z) - 1 : 64;
            const u64 mask = len >= 64 ? ~0ull : ((1ull << len) - 1) << s;
            const u32 run = (s == 0 && carry) ? next - 1 : next++;
            if (run < nruns) {
                const u32 c = cc_component(parent, rank, run);
                bool keep;
                if (MAP) {
                    keep = c < nmap && map[c] != 0;
                    if (c >= nmap) atomicOr((unsigned long long *)flags, CC_F_RANGE);
                } else {
                    keep = largest ? (u64)c + 1 == only : (c < nruns && sizes[c] >= min_voxels);
                }
                if (keep) res |= mask;
            } else {
                atomicOr((unsigned long long *)flags, CC_F_RANGE);
            }
            m &= ~mask;
        }
    }
    out[i] = res;
}

TOMO_API int tomo_cc_filter(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                            const uint32_t *parent, const uint32_t *rank, const int64_t *sizes, unsigned long long *tot,
                            int64_t min_voxels, int largest, uint64_t *out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !sizes || !tot || !out || out == bits || cap_runs <= 0 || min_voxels < 0) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nwords = nrows * wx;
    if (largest)
        hipLaunchKernelGGL(cc_largest_kernel<1>, dim3(1), dim3(1024), 0, st, (const unsigned long long *)sizes, (u64 *)tot, cap_runs,
                           cap_runs, (u64)min_voxels);
    hipLaunchKernelGGL(cc_filter_kernel<false>, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, st, (const u64 *)bits,
                       nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank,
                       (const unsigned long long *)sizes, (u64)min_voxels, largest ? 1 : 0, (const uint8_t *)nullptr, 0u, (u64 *)out,
                       (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- measurements per component
// table (device int64[cap][CC_COLS]), row c = component c + 1: [0] voxels  [1, 2] zmin, zmax  [3, 4] ymin, ymax  [5, 6] xmin,
// xmax (inclusive indices)  [7] sum of z over the voxels  [8] sum of y  [9] sum of x.  Every entry is a non-negative integer
// below 2^63, so the kernels work on it as u64 and the 64-bit unsigned min / max / add atomics keep it exact and the same on
// every run.  The count of components comes from tot[1]; more than the table's rows: nothing is touched (CC_F_CAP).
__device__ static inline int64_t cc_ncomp(const u64 *tot, int64_t cap)
{
    const u64 n = tot[1];
    return n > (u64)cap ? 0 : (int64_t)n;
}

// the minima start at the largest int64 (a memset cannot give that), everything else at 0
__global__ __launch_bounds__(CC_THREADS) void cc_table_init_kernel(u64 *__restrict__ table, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= cap * CC_COLS) return;
    const int col = (int)(i % CC_COLS);
    table[i] = (col == 1 || col == 3 || col == 5) ? 0x7fffffffffffffffull : 0ull;
}

// what a thread, or a wave, has added up for ONE component
struct CcMeasure {
    u64 vox, sz, sy, sx;
    u32 z0, z1, y0, y1, x0, x1;
};

__device__ static inline void cc_measure_flush(u64 *__restrict__ table, u32 c, const CcMeasure &m)
{
    u64 *t = table + (int64_t)c * CC_COLS;
    atomicAdd(t + 0, m.vox);
    atomicMin(t + 1, (u64)m.z0);
    atomicMax(t + 2, (u64)m.z1);
    atomicMin(t + 3, (u64)m.y0);
    atomicMax(t + 4, (u64)m.y1);
    atomicMin(t + 5, (u64)m.x0);
    atomicMax(t + 6, (u64)m.x1);
    atomicAdd(t + 7, m.sz);
    atomicAdd(t + 8, m.sy);
    atomicAdd(t + 9, m.sx);
}

__device__ static inline u32 wave_min32(u32 v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ static inline u32 wave_max32(u32 v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One thread per row (z, y) over its runs, as cc_sizes_kernel: a run [s, e) adds len = e - s voxels, len * z, len * y and
// len * (s + e - 1) / 2 = s + (s + 1) + .. + (e - 1) (len or s + e - 1 is even: exact) and widens the box.  A thread adds up
// neighbouring runs of one component first; a wave whose lanes all hold the same component adds once (one solid body: ten
// atomics per 64 rows, whatever slices the rows lie in -- every lane brings its own z and y).
__global__ __launch_bounds__(CC_THREADS) void cc_measure_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                int64_t cap_runs, const u32 *__restrict__ parent,
                                                                const u32 *__restrict__ rank, u64 *__restrict__ table, int64_t cap,
                                                                u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const u32 ncomp = (u32)cc_ncomp(tot, cap);
    if (row == 0 && tot[1] > (u64)cap) atomicOr((unsigned long long *)flags, CC_F_CAP);
    u32 comp = 0;                                           // component + 1 the thread is adding up, 0: none
    CcMeasure m = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (row < nrows) {
        const u32 z = (u32)(row / ny), y = (u32)(row % ny);
        m.z0 = m.z1 = z;
        m.y0 = m.y1 = y;
        CcRuns a = cc_runs_begin(bits, row, nx, wx);
        u32 ia = row_off[row];
        while (a.valid) {
            if (ia >= nruns) {
                atomicOr((unsigned long long *)flags, CC_F_RANGE);
                break;
            }
            const u32 c = cc_component(parent, rank, ia) + 1;
            if (c != comp) {
                if (m.vox && comp - 1 < ncomp) {
                    m.sz = m.vox * z;
                    m.sy = m.vox * y;
                    cc_measure_flush(table, comp - 1, m);
                }
                comp = c;
                m.vox = m.sx = 0;
                m.x0 = (u32)a.s;
            }
            const u64 len = (u64)(a.e - a.s);
            m.vox += len;
            m.sx += len * (u64)(a.s + a.e - 1) / 2;
            m.x1 = (u32)(a.e - 1);                          // the runs ascend
            cc_runs_next(a);
            ia++;
        }
        m.sz = m.vox * z;
        m.sy = m.vox * y;
    }
    if (!m.vox) comp = 0;
    const u32 top = wave_max32(comp);
    if (top == 0) return;                                   // wave-uniform
    if (__all(comp == 0 || comp == top)) {
        const bool has = comp != 0;
        CcMeasure w;
        w.vox = wave_sum64(m.vox);
        w.sz = wave_sum64(has ? m.sz : 0);
        w.sy = wave_sum64(has ? m.sy : 0);
        w.sx = wave_sum64(m.sx);
        w.z0 = wave_min32(has ? m.z0 : ~0u);
        w.z1 = wave_max32(has ? m.z1 : 0u);
        w.y0 = wave_min32(has ? m.y0 : ~0u);
        w.y1 = wave_max32(has ? m.y1 : 0u);
        w.x0 = wave_min32(has ? m.x0 : ~0u);
        w.x1 = wave_max32(has ? m.x1 : 0u);
        if ((threadIdx.x & 63) == 0 && top - 1 < ncomp) cc_measure_flush(table, top - 1, w);
    } else if (comp != 0 && comp - 1 < ncomp) {
        cc_measure_flush(table, comp - 1, m);
    }
}

TOMO_API int tomo_cc_measure(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                             const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t *table, int64_t cap,
                             void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !table || cap_runs <= 0 || cap <= 0) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_table_init_kernel, dim3((unsigned)ceil_div64(cap * CC_COLS, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (u64 *)table, cap);
    hipLaunchKernelGGL(cc_measure_kernel, dim3((unsigned)ceil_div64(nrows, CC_THREADS)), dim3(CC_THREADS), 0, st, (const u64 *)bits,
                       nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank,
                       (u64 *)table, cap, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- voxels per component and slice
// The volume of a component under per-slice depths needs its voxels PER SLICE.  The selected components (the keep rule of
// tomo_cc_filter on column 0 of the table) get a segment of zmax - zmin + 1 counters each in one histogram: off = the
// exclusive scan of the segment lengths, 0-length for the others, in 64 bits (2^31 components of up to 2^31 slices), and
// slot = the exclusive scan of the selection = the row of a selected component in the compacted results.
// tot[4] = all counters, tot[5] = selected components.
__device__ static inline bool cc_selected(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t c, u64 min_voxels,
                                          int largest)
{
    return largest ? (u64)c + 1 == tot[3] : table[c * CC_COLS] >= min_voxels;
}

// length of the segment of component c (0: not selected, or a box that is none)
__device__ static inline u64 cc_zspan(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t c, u64 min_voxels,
                                      int largest, bool *sel)
{
    const u64 z0 = table[c * CC_COLS + 1], z1 = table[c * CC_COLS + 2];
    *sel = cc_selected(table, tot, c, min_voxels, largest);
    return *sel && z1 >= z0 ? z1 - z0 + 1 : 0;
}

__device__ static inline u64 wave_inclusive_scan64(u64 v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// per tile of CC_SCAN_TILE components: blk[b] = its counters, blk[nblk + b] = its selected components; sel[c] on the way
__global__ __launch_bounds__(CC_THREADS) void cc_zspan_blocksum_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                       int64_t cap, u64 min_voxels, int largest,
                                                                       uint8_t *__restrict__ sel, u64 *__restrict__ blk, int64_t nblk,
                                                                       u64 *flags)
{
    __shared__ u64 wsum[2][CC_THREADS / 64];
    const int64_t n = cc_ncomp(tot, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0 && tot[1] > (u64)cap) atomicOr((unsigned long long *)flags, CC_F_CAP);
    const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + 4 * threadIdx.x;
    u64 span = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n) {
            bool s;
            span += cc_zspan(table, tot, i0 + j, min_voxels, largest, &s);
            cnt += s ? 1 : 0;
            sel[i0 + j] = s ? 1 : 0;
        }
    }
    span = wave_sum64(span);
    cnt = wave_sum64(cnt);
    if ((threadIdx.x & 63) == 0) {
        wsum[0][threadIdx.x >> 6] = span;
        wsum[1][threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        blk[nblk + blockIdx.x] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    }
}

// off[c], slot[c] for every c < n and off[n] = all counters (written by the thread that holds component n - 1)
__global__ __launch_bounds__(CC_THREADS) void cc_zspan_apply_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                    int64_t cap, u64 min_voxels, int largest,
                                                                    const u64 *__restrict__ blk, int64_t nblk, u64 *__restrict__ off,
                                                                    u32 *__restrict__ slot)
{
    __shared__ u64 wsum[2][CC_THREADS / 64];
    const int64_t n = cc_ncomp(tot, cap);
    const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + 4 * threadIdx.x;
    u64 x[4], k[4];
    u64 span = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        bool s = false;
        x[j] = i0 + j < n ? cc_zspan(table, tot, i0 + j, min_voxels, largest, &s) : 0;
        k[j] = s ? 1 : 0;
        span += x[j];
        cnt += k[j];
    }
    const u64 ispan = wave_inclusive_scan64(span), icnt = wave_inclusive_scan64(cnt);
    if ((threadIdx.x & 63) == 63) {
        wsum[0][threadIdx.x >> 6] = ispan;
        wsum[1][threadIdx.x >> 6] = icnt;
    }
    __syncthreads();
    u64 bspan = 0, bcnt = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) {
        bspan += wsum[0][w];
        bcnt += wsum[1][w];
    }
    u64 run = blk[blockIdx.x] + bspan + ispan - span, num = blk[nblk + blockIdx.x] + bcnt + icnt - cnt;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n) {
            off[i0 + j] = run;
            slot[i0 + j] = (u32)num;
            if (i0 + j == n - 1) off[n] = run + x[j];
        }
        run += x[j];
        num += k[j];
    }
}

TOMO_API int tomo_cc_zhist_offsets(const int64_t *table, int64_t cap, unsigned long long *tot, int64_t min_voxels, int largest,
                                   uint8_t *sel, uint64_t *off, uint32_t *slot, uint64_t *blk, void *stream)
{
    if (!table || !tot || !sel || !off || !slot || !blk || cap <= 0 || min_voxels < 0) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const u64 *t = (const u64 *)table;
    u64 *tt = (u64 *)tot;
    const int64_t nblk = ceil_div64(cap, CC_SCAN_TILE);
    if (largest)                                            // no run table is read here: only the count of components is capped
        hipLaunchKernelGGL(cc_largest_kernel<CC_COLS>, dim3(1), dim3(1024), 0, st, (const unsigned long long *)t, tt, cap,
                           (int64_t)0x7fffffffffffffffll, (u64)min_voxels);
    hipLaunchKernelGGL(cc_zspan_blocksum_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, t, (const u64 *)tt, cap,
                       (u64)min_voxels, largest ? 1 : 0, sel, (u64 *)blk, nblk, tt + 2);
    hipLaunchKernelGGL(cc_scan1_kernel, dim3(1), dim3(1024), 0, st, (u64 *)blk, nblk, tt + 4, (u64 *)nullptr);
    hipLaunchKernelGGL(cc_scan1_kernel, dim3(1), dim3(1024), 0, st, (u64 *)blk + nblk, nblk, tt + 5, (u64 *)nullptr);
    hipLaunchKernelGGL(cc_zspan_apply_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, t, (const u64 *)tt, cap, (u64)min_voxels,
                       largest ? 1 : 0, (const u64 *)blk, nblk, (u64 *)off, (u32 *)slot);
    return tomo_status();
}

// hist[off[c] + z - zmin[c]] += voxels: checked against the component's box and the histogram's length before the add
__device__ static inline void cc_zhist_add(const u64 *__restrict__ table, const u64 *__restrict__ off, u64 *__restrict__ hist,
                                           u64 total, u32 c, u32 z, u64 count, u64 *flags)
{
    const u64 z0 = table[(int64_t)c * CC_COLS + 1], z1 = table[(int64_t)c * CC_COLS + 2];
    const u64 pos = off[c] + ((u64)z - z0);
    if (z < z0 || z > z1 || pos >= total) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    atomicAdd(hist + pos, count);
}

// One thread per row, as cc_measure_kernel; only the runs of selected components count.  A wave whose lanes all hold the
// same component adds once PER SLICE the wave's rows lie in: mostly one, more where the wave straddles slices (ny < 64).
__global__ __launch_bounds__(CC_THREADS) void cc_zhist_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                              const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                              int64_t cap_runs, const u32 *__restrict__ parent,
                                                              const u32 *__restrict__ rank, const u64 *__restrict__ table, int64_t cap,
                                                              const uint8_t *__restrict__ sel, const u64 *__restrict__ off,
                                                              u64 *__restrict__ hist, int64_t hist_cap, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const u64 total = tot[4];
    const bool fits = total <= (u64)hist_cap;
    const u32 ncomp = fits ? (u32)cc_ncomp(tot, cap) : 0u;  // a histogram that is too short: nothing is touched
    if (row == 0 && (!fits || tot[1] > (u64)cap)) atomicOr((unsigned long long *)flags, CC_F_CAP);
    const u32 z = row < nrows ? (u32)(row / ny) : 0u;
    u32 comp = 0;                                           // SELECTED component + 1 the thread is adding up, 0: none
    u64 acc = 0;
    if (row < nrows) {
        CcRuns a = cc_runs_begin(bits, row, nx, wx);
        u32 ia = row_off[row];
        while (a.valid) {
            if (ia >= nruns) {
                atomicOr((unsigned long long *)flags, CC_F_RANGE);
                break;
            }
            u32 c = cc_component(parent, rank, ia) + 1;
            if (c - 1 >= ncomp || !sel[c - 1]) c = 0;
            if (c != comp) {
                if (acc) cc_zhist_add(table, off, hist, total, comp - 1, z, acc, flags);
                comp = c;
                acc = 0;
            }
            if (c) acc += (u64)(a.e - a.s);
            cc_runs_next(a);
            ia++;
        }
    }
    if (!acc) comp = 0;
    const u32 top = wave_max32(comp);
    if (top == 0) return;                                   // wave-uniform
    if (__all(comp == 0 || comp == top)) {
        const u32 zlo = wave_min32(comp ? z : ~0u), zhi = wave_max32(comp ? z : 0u);
        for (u32 zz = zlo; zz <= zhi; zz++) {               // wave-uniform bounds: at most 64 slices hold the wave's 64 rows
            const u64 sum = wave_sum64(comp && z == zz ? acc : 0);
            if ((threadIdx.x & 63) == 0 && sum) cc_zhist_add(table, off, hist, total, top - 1, zz, sum, flags);
        }
    } else if (comp != 0) {
        cc_zhist_add(table, off, hist, total, comp - 1, z, acc, flags);
    }
}

TOMO_API int tomo_cc_zhist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                           const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                           const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !table || !sel || !off || !hist || cap_runs <= 0 || cap <= 0 || hist_cap <= 0)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || hist_cap >= ((int64_t)1 << 60)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)hist_cap * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_zhist_kernel, dim3((unsigned)ceil_div64(nrows, CC_THREADS)), dim3(CC_THREADS), 0, st, (const u64 *)bits,
                       nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank,
                       (const u64 *)table, cap, sel, (const u64 *)off, (u64 *)hist, hist_cap, (u64 *)tot + 2);
    return tomo_status();
}

// One thread per component; a selected one walks its slices in ascending z: vol += (double)count * w[z] and
// mz += ((double)count * w[z]) * zc[z], plain sequential float64 (nothing is contracted in this file: -ffp-contract=off), so
// vol is the float a host loop over the slices of the mask `labels == c` gives -- the slices outside the box add 0.0 there.
// out[slot[c]] = (vol, mz), labels[slot[c]] = c + 1.
__global__ __launch_bounds__(CC_THREADS) void cc_zsums_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                                              const uint8_t *__restrict__ sel, const u64 *__restrict__ off,
                                                              const u32 *__restrict__ slot, const u64 *__restrict__ hist,
                                                              int64_t hist_cap, const double *__restrict__ w,
                                                              const double *__restrict__ zc, int nz, double *__restrict__ out,
                                                              int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u64 total = tot[4];
    const bool fits = total <= (u64)hist_cap && tot[5] <= (u64)cap_sel && tot[1] <= (u64)cap;
    if (c == 0 && !fits) atomicOr((unsigned long long *)flags, CC_F_CAP);
    if (!fits || c >= cc_ncomp(tot, cap) || !sel[c]) return;
    const u64 z0 = table[c * CC_COLS + 1], z1 = table[c * CC_COLS + 2], o = off[c];
    const u32 k = slot[c];
    if (z1 < z0 || z1 >= (u64)nz || o + (z1 - z0) >= total || (int64_t)k >= cap_sel) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    double vol = 0.0, mz = 0.0;
    for (u64 z = z0; z <= z1; z++) {
        const double v = (double)hist[o + (z - z0)] * w[z];
        vol += v;
        mz += v * zc[z];
    }
    out[2 * (int64_t)k] = vol;
    out[2 * (int64_t)k + 1] = mz;
    labels[k] = c + 1;
}

TOMO_API int tomo_cc_zsums(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                           const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *w, const double *zc, int nz,
                           double *out, int64_t *labels, int64_t cap_sel, void *stream)
{
    if (!table || !tot || !sel || !off || !slot || !hist || !w || !zc || !out || !labels || cap <= 0 || hist_cap <= 0 || nz <= 0 ||
        cap_sel <= 0)
        return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31) || hist_cap >= ((int64_t)1 << 60)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_zsums_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot, (const u64 *)hist, hist_cap,
                       w, zc, nz, out, labels, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- second moments per component
// A set voxel (k, j, i) of component c is a point mass at (zc[k], j * mm_y, i * mm_x) of weight w[k] = (mm_x * mm_y) * depth[k].
// Its second moments need, per slice of the component's box, six integer sums over the slice's voxels of the component, taken
// about the box corner (j' = j - ymin, i' = i - xmin) to keep them small: N, sum j', sum i', sum j'^2, sum i'^2, sum j' i'.
// They live in the segments of tomo_cc_zhist_offsets, six words per entry: mom[6 * (off[c] + z - zmin) + k].
#define CC_MOMS 6                    // sums per component and slice
#define CC_MOMENT_COLS 22            // doubles per row of tomo_cc_moments' output
#define CC_JACOBI_SWEEPS 32          // limit of the cyclic Jacobi iteration (a 3 x 3 matrix is done in 5 or 6)

// 0^2 + 1^2 + .. + (n - 1)^2 = (n - 1) n (2 n - 1) / 6; n <= nx, and tomo_cc_moment_hist refuses max(ny, nx)^3 >= 2^63
__device__ static inline u64 cc_squares_below(u64 n)
{
    return (n - 1) * n * (2 * n - 1) / 6;                   // n = 0: the wrapped factor meets a 0
}

// the six sums of one row from what its runs gave (voxels, sum i', sum i'^2) and the row's j'
__device__ static inline void cc_moment_row(u64 n, u64 si, u64 sii, u64 jp, u64 (&v)[CC_MOMS])
{
    v[0] = n;
    v[1] = jp * n;
    v[2] = si;
    v[3] = jp * jp * n;
    v[4] = sii;
    v[5] = jp * si;
}

// mom[6 * (off[c] + z - zmin[c]) + k] += v[k]: checked against the component's box and the histogram's length before the adds
__device__ static inline void cc_moment_add(const u64 *__restrict__ table, const u64 *__restrict__ off, u64 *__restrict__ mom,
                                            u64 total, u32 c, u32 z, const u64 (&v)[CC_MOMS], u64 *flags)
{
    const u64 z0 = table[(int64_t)c * CC_COLS + 1], z1 = table[(int64_t)c * CC_COLS + 2];
    const u64 pos = off[c] + ((u64)z - z0);
    if (z < z0 || z > z1 || pos >= total) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
#pragma unroll
    for (int k = 0; k < CC_MOMS; k++)
        if (v[k]) atomicAdd(mom + CC_MOMS * pos + k, v[k]);
}

// One thread per row, as cc_zhist_kernel: a run [s, e) of a selected component adds its length and, in closed form, the sums
// of i' and i'^2 over it; the row supplies the factors j'.  A thread adds up neighbouring runs of one component first; a wave
// whose lanes all hold the same component adds once PER SLICE the wave's rows lie in.  A voxel in front of the box corner
// (the bits changed since tomo_cc_measure) is CC_F_RANGE and adds nothing.
__global__ __launch_bounds__(CC_THREADS) void cc_moment_hist_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                    const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                    int64_t cap_runs, const u32 *__restrict__ parent,
                                                                    const u32 *__restrict__ rank, const u64 *__restrict__ table,
                                                                    int64_t cap, const uint8_t *__restrict__ sel,
                                                                    const u64 *__restrict__ off, u64 *__restrict__ mom,
                                                                    int64_t hist_cap, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const u64 total = tot[4];
    const bool fits = total <= (u64)hist_cap;
    const u32 ncomp = fits ? (u32)cc_ncomp(tot, cap) : 0u;  // a histogram that is too short: nothing is touched
    if (row == 0 && (!fits || tot[1] > (u64)cap)) atomicOr((unsigned long long *)flags, CC_F_CAP);
    const u32 z = row < nrows ? (u32)(row / ny) : 0u, y = row < nrows ? (u32)(row % ny) : 0u;
    u32 comp = 0;                                           // SELECTED component + 1 the thread is adding up, 0: none
    u64 x0 = 0, jp = 0;                                     // its box corner in x, the row's j' in its box
    u64 n = 0, si = 0, sii = 0;
    u64 v[CC_MOMS];
    if (row < nrows) {
        CcRuns a = cc_runs_begin(bits, row, nx, wx);
        u32 ia = row_off[row];
        while (a.valid) {
            if (ia >= nruns) {
                atomicOr((unsigned long long *)flags, CC_F_RANGE);
                break;
            }
            u32 c = cc_component(parent, rank, ia) + 1;
            if (c - 1 >= ncomp || !sel[c - 1]) c = 0;
            if (c != comp) {
                if (n) {
                    cc_moment_row(n, si, sii, jp, v);
                    cc_moment_add(table, off, mom, total, comp - 1, z, v, flags);
                }
                comp = c;
                n = si = sii = 0;
                if (c) {
                    const u64 y0 = table[(int64_t)(c - 1) * CC_COLS + 3];
                    x0 = table[(int64_t)(c - 1) * CC_COLS + 5];
                    jp = (u64)y - y0;
                    if ((u64)y < y0) {
                        atomicOr((unsigned long long *)flags, CC_F_RANGE);
                        comp = c = 0;
                    }
                }
            }
            if (c) {
                if ((u64)a.s < x0) {
                    atomicOr((unsigned long long *)flags, CC_F_RANGE);
                } else {
                    const u64 s = (u64)a.s - x0, e = (u64)a.e - x0, len = e - s;
                    n += len;
                    si += len * (s + e - 1) / 2;            // len or s + e - 1 is even: exact
                    sii += cc_squares_below(e) - cc_squares_below(s);
                }
            }
            cc_runs_next(a);
            ia++;
        }
    }
    if (!n) comp = 0;
    const u32 top = wave_max32(comp);
    if (top == 0) return;                                   // wave-uniform
    cc_moment_row(n, si, sii, jp, v);
    if (__all(comp == 0 || comp == top)) {
        const u32 zlo = wave_min32(comp ? z : ~0u), zhi = wave_max32(comp ? z : 0u);
        for (u32 zz = zlo; zz <= zhi; zz++) {               // wave-uniform bounds: at most 64 slices hold the wave's 64 rows
            const bool mine = comp && z == zz;
            u64 sum[CC_MOMS];
#pragma unroll
            for (int k = 0; k < CC_MOMS; k++) sum[k] = wave_sum64(mine ? v[k] : 0);
            if ((threadIdx.x & 63) == 0 && sum[0]) cc_moment_add(table, off, mom, total, top - 1, zz, sum, flags);
        }
    } else if (comp != 0) {
        cc_moment_add(table, off, mom, total, comp - 1, z, v, flags);
    }
}

TOMO_API int tomo_cc_moment_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                 const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table,
                                 int64_t cap, const uint8_t *sel, const uint64_t *off, uint64_t *mom, int64_t hist_cap, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !table || !sel || !off || !mom || cap_runs <= 0 || cap <= 0 || hist_cap <= 0)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || hist_cap >= ((int64_t)1 << 60) / CC_MOMS) return TOMO_E_SIZE;
    const unsigned __int128 side = (unsigned __int128)(ny > nx ? ny : nx);
    if ((unsigned __int128)ny * (unsigned __int128)nx * side * side >= ((unsigned __int128)1 << 63))
        return TOMO_E_SIZE;                                 // a slice's sum of j'^2, i'^2 or j' i' could leave 63 bits
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(mom, 0, (size_t)hist_cap * CC_MOMS * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_moment_hist_kernel, dim3((unsigned)ceil_div64(nrows, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u64 *)bits, nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, (const u64 *)table, cap, sel, (const u64 *)off, (u64 *)mom, hist_cap, (u64 *)tot + 2);
    return tomo_status();
}

// One Jacobi rotation of a symmetric 3 x 3 matrix that annihilates a_pq (r = the third index): A <- J^T A J, the eigenvector
// estimates ep, eq (columns p, q of the accumulated rotations) turn with it.  t is the smaller root, |t| <= 1.
__device__ static inline void cc_jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (&ep)[3],
                                               double (&eq)[3])
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq), at = fabs(theta);
    double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = ep[k], vq = eq[k];
        ep[k] = c * vp - s * vq;
        eq[k] = s * vp + c * vq;
    }
}

// swap so that the larger eigenvalue comes first; equal ones keep their order
__device__ static inline void cc_order_pair(double &la, double &lb, double (&ea)[3], double (&eb)[3])
{
    if (la < lb) {
        const double l = la;
        la = lb;
        lb = l;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double e = ea[k];
            ea[k] = eb[k];
            eb[k] = e;
        }
    }
}

// the component of largest magnitude positive, the first such on a tie
__device__ static inline void cc_axis_sign(double (&e)[3])
{
    int k = 0;
    if (fabs(e[1]) > fabs(e[k])) k = 1;
    if (fabs(e[2]) > fabs(e[k])) k = 2;
    if (e[k] < 0.0) {
#pragma unroll
        for (int j = 0; j < 3; j++) e[j] = 0.0 - e[j];
    }
}

// One thread per component, as cc_zsums_kernel; a selected one walks its slices in ascending z twice, plain sequential
// float64 (nothing is contracted in this file).  First walk: W by cc_zsums_kernel's very additions, the z moment likewise, and
// the first moments about the box corner (zc[zmin], ymin, xmin).  Second walk: the six central sums about the centre those
// give.  Then cyclic Jacobi on the 3 x 3 covariance, the eigenvalues sorted descending (clamped at 0), the sign rule.
// out[slot[c]] = W, centre (z, y, x) in mm, covariance zz zy zx yy yx xx, variances, axes (rows); labels[slot[c]] = c + 1.
__global__ __launch_bounds__(CC_THREADS) void cc_moments_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                int64_t cap, const uint8_t *__restrict__ sel,
                                                                const u64 *__restrict__ off, const u32 *__restrict__ slot,
                                                                const u64 *__restrict__ mom, int64_t hist_cap,
                                                                const double *__restrict__ w, const double *__restrict__ zc, int nz,
                                                                double mm_y, double mm_x, double *__restrict__ out,
                                                                int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u64 total = tot[4];
    const bool fits = total <= (u64)hist_cap && tot[5] <= (u64)cap_sel && tot[1] <= (u64)cap;
    if (c == 0 && !fits) atomicOr((unsigned long long *)flags, CC_F_CAP);
    if (!fits || c >= cc_ncomp(tot, cap) || !sel[c]) return;
    const u64 z0 = table[c * CC_COLS + 1], z1 = table[c * CC_COLS + 2], o = off[c];
    const u32 k = slot[c];
    if (z1 < z0 || z1 >= (u64)nz || o + (z1 - z0) >= total || (int64_t)k >= cap_sel) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    const u64 *m = mom + CC_MOMS * o;
    const double zo = zc[z0];
    double vol = 0.0, mz = 0.0, sz = 0.0, sy = 0.0, sx = 0.0;
    for (u64 z = z0; z <= z1; z++) {
        const u64 *s = m + CC_MOMS * (z - z0);
        const double v = (double)s[0] * w[z];
        vol += v;
        mz += v * zc[z];
        sz += v * (zc[z] - zo);
        sy += w[z] * (double)s[1];
        sx += w[z] * (double)s[2];
    }
    if (!(vol > 0.0)) {                                     // no voxel arrived in the segment: the bits changed
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    const double cz = sz / vol, cy = sy / vol, cx = sx / vol;    // about the box corner: mm along z, indices in the plane
    double qzz = 0.0, qzy = 0.0, qzx = 0.0, qyy = 0.0, qyx = 0.0, qxx = 0.0;
    for (u64 z = z0; z <= z1; z++) {
        const u64 *s = m + CC_MOMS * (z - z0);
        const double n = (double)s[0], sj = (double)s[1], si = (double)s[2], sjj = (double)s[3], sii = (double)s[4],
                     sji = (double)s[5];
        const double dz = (zc[z] - zo) - cz;
        const double a = sj - n * cy, b = si - n * cx;      // sums of j' - cy and of i' - cx over the slice
        qzz += w[z] * (n * dz * dz);
        qzy += w[z] * (dz * a);
        qzx += w[z] * (dz * b);
        qyy += w[z] * ((sjj - cy * sj) - cy * a);
        qyx += w[z] * ((sji - cy * si) - cx * a);
        qxx += w[z] * ((sii - cx * si) - cx * b);
    }
    double a00 = qzz / vol, a01 = qzy * mm_y / vol, a02 = qzx * mm_x / vol, a11 = qyy * (mm_y * mm_y) / vol,
           a12 = qyx * (mm_y * mm_x) / vol, a22 = qxx * (mm_x * mm_x) / vol;
    double *r = out + CC_MOMENT_COLS * (int64_t)k;
    r[0] = vol;
    r[1] = mz / vol;
    r[2] = ((double)table[c * CC_COLS + 3] + cy) * mm_y;
    r[3] = ((double)table[c * CC_COLS + 5] + cx) * mm_x;
    r[4] = a00;
    r[5] = a01;
    r[6] = a02;
    r[7] = a11;
    r[8] = a12;
    r[9] = a22;
    double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < CC_JACOBI_SWEEPS; sweep++) {
        const double offd = fabs(a01) + fabs(a02) + fabs(a12);
        if (offd <= 0x1p-60 * (fabs(a00) + fabs(a11) + fabs(a22))) break;      // also a zero matrix
        cc_jacobi_rotate(a00, a11, a01, a02, a12, e0, e1);
        cc_jacobi_rotate(a00, a22, a02, a01, a12, e0, e2);
        cc_jacobi_rotate(a11, a22, a12, a01, a02, e1, e2);
    }
    cc_order_pair(a00, a11, e0, e1);
    cc_order_pair(a11, a22, e1, e2);
    cc_order_pair(a00, a11, e0, e1);
    cc_axis_sign(e0);
    cc_axis_sign(e1);
    cc_axis_sign(e2);
    r[10] = a00 > 0.0 ? a00 : 0.0;
    r[11] = a11 > 0.0 ? a11 : 0.0;
    r[12] = a22 > 0.0 ? a22 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        r[13 + j] = e0[j];
        r[16 + j] = e1[j];
        r[19 + j] = e2[j];
    }
    labels[k] = c + 1;
}

TOMO_API int tomo_cc_moments(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                             const uint32_t *slot, const uint64_t *mom, int64_t hist_cap, const double *w, const double *zc, int nz,
                             double mm_y, double mm_x, double *out, int64_t *labels, int64_t cap_sel, void *stream)
{
    if (!table || !tot || !sel || !off || !slot || !mom || !w || !zc || !out || !labels || cap <= 0 || hist_cap <= 0 || nz <= 0 ||
        cap_sel <= 0 || !(mm_y > 0.0 && mm_y < __builtin_inf()) || !(mm_x > 0.0 && mm_x < __builtin_inf()))
        return TOMO_E_ARG;                                  // a NaN fails both comparisons
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31) || hist_cap >= ((int64_t)1 << 60) / CC_MOMS) return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_moments_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot, (const u64 *)mom, hist_cap,
                       w, zc, nz, mm_y, mm_x, out, labels, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- Euler number, cavities, handles
// chi of the set voxels as a sum over the voxels, every cell of the complex counted by exactly ONE of them, so that nothing is
// divided and the voxels of a component add up to the component's chi (every cell touches voxels of one component only):
//   connectivity 6:  the dual complex (a cell = 1, 2, 4 or 8 voxels that are ALL set) -- a cell belongs to its low-corner
//                    voxel.  Voxel v adds 1 - [x] - [y] - [z] + [x y xy] + [x z xz] + [y z yz] - [all seven], the names
//                    being the voxels of the 2 x 2 x 2 block above v that must be set.
//   connectivity 26: the cubical complex (a lattice vertex / edge / face / cube is present if ANY voxel incident to it is
//                    set) -- a cell belongs to the raster-first set voxel incident to it, i.e. v owns a cell iff every
//                    raster-EARLIER voxel incident to the cell is clear.  Of the 27 cells of v's cube the ones no earlier voxel
//                    touches cancel (1 vertex - 3 edges + 3 faces - 1 cube = 0), and so do all that hang on the voxel at
//                    x - 1 or at y - 1 alone.  With Q, P, R the rows (z-1, y), (z-1, y-1), (z-1, y+1), S the row (z, y-1), T
//                    the row itself, a suffix m / p for the voxel at x - 1 / x + 1 and [..] = 1 iff all the voxels named are
//                    CLEAR, what is left is
//                      [Q] - [Q R] - [S Q P] - [Q Qp] - [Tm Q Qm]
//                      + [Q Qp R Rp] + [Q Qm R Rm Tm] + [Q Qp P Pp S Sp] + [Q Qm P Pm Tm S Sm]
//                    (the face below; the two edges below along x and the two along y; the four vertices below).
// Per word these are ANDs / ORs of the row's word with up to four neighbour rows and their shifts by one bit, carried across
// the word boundaries; a run's share is the popcount of every term under the run's mask.  Rows outside the stack and bits at
// x >= nx read as 0.
struct CcWin {                                               // three neighbouring words of one row, slid along x
    u64 prv, cur, nxt;
};

__device__ static inline u64 cc_word_or0(const u64 *__restrict__ row, int nx, int wx, int w)
{
    return (row && w < wx) ? cc_word(row, nx, wx, w) : 0ull;
}

__device__ static inline u64 cc_xp(const CcWin &r) { return (r.cur >> 1) | (r.nxt << 63); }      // bit x = voxel x + 1
__device__ static inline u64 cc_xm(const CcWin &r) { return (r.cur << 1) | (r.prv >> 63); }      // bit x = voxel x - 1

#define CC_EULER_POS 5
#define CC_EULER_NEG 4

// the terms of chi for the word win[0].cur of the row: pos[] count + 1 per bit, neg[] count - 1
template <int K>
__device__ static inline void cc_euler_terms(const CcWin *win, u64 *pos, u64 *neg)
{
    const u64 t = win[0].cur;
    if constexpr (K == 6) {                                 // win: the row, (z, y+1), (z+1, y), (z+1, y+1)
        const u64 b = win[1].cur, c = win[2].cur, d = win[3].cur;
        const u64 ex = t & cc_xp(win[0]), ey = t & b, ez = t & c;
        const u64 fxy = ex & b & cc_xp(win[1]), fxz = ex & c & cc_xp(win[2]), fyz = ey & c & d;
        pos[0] = t;
        pos[1] = fxy;
        pos[2] = fxz;
        pos[3] = fyz;
        pos[4] = 0;
        neg[0] = ex;
        neg[1] = ey;
        neg[2] = ez;
        neg[3] = fxy & c & cc_xp(win[2]) & d & cc_xp(win[3]);
    } else {                                                // win: the row T, S = (z, y-1), Q = (z-1, y), P = (z-1, y-1), R = (z-1, y+1)
        const u64 tm = cc_xm(win[0]);
        const u64 s = win[1].cur, q = win[2].cur, p = win[3].cur, r = win[4].cur;
        const u64 qlo = q | cc_xm(win[2]) | tm, qhi = q | cc_xp(win[2]);       // below and behind / below and ahead
        const u64 slo = s | cc_xm(win[1]), shi = s | cc_xp(win[1]);
        const u64 plo = p | cc_xm(win[3]), phi = p | cc_xp(win[3]);
        const u64 rlo = r | cc_xm(win[4]), rhi = r | cc_xp(win[4]);
        pos[0] = t & ~q;
        pos[1] = t & ~(qhi | rhi);
        pos[2] = t & ~(qlo | rlo);
        pos[3] = t & ~(qhi | phi | shi);
        pos[4] = t & ~(qlo | plo | slo);
        neg[0] = t & ~(q | r);
        neg[1] = t & ~(s | q | p);
        neg[2] = t & ~qhi;
        neg[3] = t & ~qlo;
    }
}

// chi of the bits under mask, as a two's complement u64
__device__ static inline u64 cc_euler_under(const u64 *pos, const u64 *neg, u64 mask)
{
    int v = 0;
#pragma unroll
    for (int i = 0; i < CC_EULER_POS; i++) v += __popcll(pos[i] & mask);
#pragma unroll
    for (int i = 0; i < CC_EULER_NEG; i++) v -= __popcll(neg[i] & mask);
    return (u64)(int64_t)v;
}

// One thread per row (z, y) over its words and, LABELLED, over the runs in every word (as cc_filter_kernel walks them): a
// thread adds up neighbouring runs of one component, a wave whose lanes all hold the same component adds once, then one signed
// 64-bit atomic add (two's complement on u64) into euler[rank[parent[run]]].  Not LABELLED: no table is read and everything
// goes to euler[0] -- the Euler number of the whole volume.
template <int K, bool LABELLED>
__global__ __launch_bounds__(CC_THREADS) void cc_euler_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                              const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                              int64_t cap_runs, const u32 *__restrict__ parent,
                                                              const u32 *__restrict__ rank, unsigned long long *__restrict__ euler,
                                                              int64_t cap, u64 *flags)
{
    constexpr int NR = K == 6 ? 4 : 5;
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = LABELLED ? (u32)cc_count(tot, cap_runs) : 0u;
    const u32 ncomp = LABELLED ? (u32)cc_ncomp(tot, cap) : 1u;
    if (LABELLED && row == 0 && tot[1] > (u64)cap) atomicOr((unsigned long long *)flags, CC_F_CAP);
    u32 comp = 0;                                           // component + 1 the thread is adding up, 0: none
    u64 acc = 0;
    if (row < nrows) {
        const int y = (int)(row % ny);
        const bool up = y + 1 < ny, down = y > 0, front = row + ny < nrows, back = row >= ny;
        const u64 *self = bits + row * wx;
        const u64 *r[NR];
        r[0] = self;
        if constexpr (K == 6) {
            r[1] = up ? self + wx : nullptr;
            r[2] = front ? self + (int64_t)ny * wx : nullptr;
            r[3] = up && front ? self + (int64_t)(ny + 1) * wx : nullptr;
        } else {
            r[1] = down ? self - wx : nullptr;
            r[2] = back ? self - (int64_t)ny * wx : nullptr;
            r[3] = back && down ? self - (int64_t)(ny + 1) * wx : nullptr;
            r[4] = back && up ? self - (int64_t)(ny - 1) * wx : nullptr;
        }
        CcWin win[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) {
            win[i].prv = 0;
            win[i].cur = cc_word_or0(r[i], nx, wx, 0);
            win[i].nxt = cc_word_or0(r[i], nx, wx, 1);
        }
        u32 next = LABELLED ? row_off[row] : 0u;            // id of the next run that STARTS
        bool carry = false;                                 // the word before ended inside a run
        for (int w = 0; w < wx; w++) {
            u64 m = win[0].cur;
            if (m) {
                u64 pos[CC_EULER_POS], neg[CC_EULER_NEG];
                cc_euler_terms<K>(win, pos, neg);
                if (!LABELLED) {
                    comp = 1;
                    acc += cc_euler_under(pos, neg, m);
                }
                while (LABELLED && m) {                     // every turn clears at least one bit of m
                    const int s = __ffsll((long long)m) - 1;
                    const u64 z = ~(m >> s);
                    const int len = z ? __ffsll((long long)z) - 1 : 64;
                    const u64 mask = len >= 64 ? ~0ull : ((1ull << len) - 1) << s;
                    const u32 run = (s == 0 && carry) ? next - 1 : next++;
                    if (run < nruns) {
                        const u32 c = cc_component(parent, rank, run) + 1;
                        if (c != comp) {
                            if (acc && comp - 1 < ncomp) atomicAdd(euler + (comp - 1), (unsigned long long)acc);
                            comp = c;
                            acc = 0;
                        }
                        acc += cc_euler_under(pos, neg, mask);
                    } else {
                        atomicOr((unsigned long long *)flags, CC_F_RANGE);
                    }
                    m &= ~mask;
                }
            }
            carry = (win[0].cur >> 63) != 0;
#pragma unroll
            for (int i = 0; i < NR; i++) {
                win[i].prv = win[i].cur;
                win[i].cur = win[i].nxt;
                win[i].nxt = cc_word_or0(r[i], nx, wx, w + 2);
            }
        }
    }
    if (!acc) comp = 0;
    const u32 top = wave_max32(comp);
    if (top == 0) return;                                   // wave-uniform
    if (__all(comp == 0 || comp == top)) {
        const u64 sum = wave_sum64(acc);
        if ((threadIdx.x & 63) == 0 && sum && top - 1 < ncomp) atomicAdd(euler + (top - 1), (unsigned long long)sum);
    } else if (comp != 0 && comp - 1 < ncomp) {
        atomicAdd(euler + (comp - 1), (unsigned long long)acc);
    }
}

TOMO_API int tomo_cc_euler(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const uint32_t *row_off, int64_t cap_runs,
                           const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t *euler, int64_t cap,
                           void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!euler || cap <= 0 || (connectivity != 6 && connectivity != 26)) return TOMO_E_ARG;
    if (parent && (!row_off || !rank || !tot || cap_runs <= 0)) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || (parent && cap_runs >= ((int64_t)1 << 31))) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(euler, 0, (size_t)cap * sizeof(int64_t), st) != hipSuccess) return TOMO_E_LAUNCH;
    const dim3 grid((unsigned)ceil_div64(nrows, CC_THREADS)), block(CC_THREADS);
    const u64 *b = (const u64 *)bits, *t = (const u64 *)tot;
    const u32 *ro = (const u32 *)row_off, *pa = (const u32 *)parent, *ra = (const u32 *)rank;
    unsigned long long *e = (unsigned long long *)euler;
    u64 *flags = tot ? (u64 *)tot + 2 : nullptr;
    if (parent) {
        if (connectivity == 6)
            hipLaunchKernelGGL((cc_euler_kernel<6, true>), grid, block, 0, st, b, nrows, ny, nx, wx, ro, t, cap_runs, pa, ra, e, cap, flags);
        else
            hipLaunchKernelGGL((cc_euler_kernel<26, true>), grid, block, 0, st, b, nrows, ny, nx, wx, ro, t, cap_runs, pa, ra, e, cap, flags);
    } else {
        if (connectivity == 6)
            hipLaunchKernelGGL((cc_euler_kernel<6, false>), grid, block, 0, st, b, nrows, ny, nx, wx, ro, t, cap_runs, pa, ra, e, cap, flags);
        else
            hipLaunchKernelGGL((cc_euler_kernel<26, false>), grid, block, 0, st, b, nrows, ny, nx, wx, ro, t, cap_runs, pa, ra, e, cap, flags);
    }
    return tomo_status();
}

// out = the complement inside the stack: ~word, the bits at x >= nx clear
__global__ __launch_bounds__(CC_THREADS) void cc_complement_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                                   u64 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= nwords) return;
    out[i] = ~bits[i] & cc_tail_mask(nx, wx, (int)(i % wx));
}

TOMO_API int tomo_cc_complement(const uint64_t *bits, int nz, int ny, int nx, uint64_t *out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!out || out == bits) return TOMO_E_ARG;
    const int64_t nwords = nrows * wx;
    hipLaunchKernelGGL(cc_complement_kernel, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (u64 *)out);
    return tomo_status();
}

// x of the k-th (0-based) run of a row, -1 if the row has no such run (at most wx + 64 turns)
__device__ static inline int cc_run_start(const u64 *__restrict__ row, int nx, int wx, u32 k)
{
    for (int w = 0; w < wx; w++) {
        u64 s = cc_starts(row, nx, wx, w, cc_word(row, nx, wx, w));
        const u32 c = (u32)__popcll(s);
        if (k < c) {
            while (k--) s &= s - 1;
            return 64 * w + __ffsll((long long)s) - 1;
        }
        k -= c;
    }
    return -1;
}

// topo (device int64[cap][3]): row c = (euler[c], 0, 0) for c < n, zeros behind
__global__ __launch_bounds__(CC_THREADS) void cc_topology_init_kernel(const u64 *__restrict__ euler, const u64 *__restrict__ tot,
                                                                      int64_t cap, u64 *__restrict__ topo)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= cap) return;
    topo[3 * c] = c < cc_ncomp(tot, cap) ? euler[c] : 0ull;
    topo[3 * c + 1] = 0;
    topo[3 * c + 2] = 0;
}

// One thread per run of the BACKGROUND (the complement, labelled under the complementary connectivity; bg_table = its
// measurement table).  A run that is its own root is the first run of its component in raster order; if the component's box
// touches no face of the stack it is a cavity, the voxel left of the run's start is set and belongs to the foreground
// component that encloses it: its run is found as cc_expand_kernel maps a bit to a run, and that component counts one more.
__global__ __launch_bounds__(CC_THREADS) void cc_cavities_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                 const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                 int64_t cap_runs, const u32 *__restrict__ parent,
                                                                 const u32 *__restrict__ rank, int64_t cap,
                                                                 const u64 *__restrict__ bg_bits, const u32 *__restrict__ bg_row_off,
                                                                 const u64 *__restrict__ bg_tot, int64_t bg_cap_runs,
                                                                 const u32 *__restrict__ bg_parent, const u32 *__restrict__ bg_rank,
                                                                 const u64 *__restrict__ bg_table, int64_t bg_cap,
                                                                 unsigned long long *__restrict__ topo, u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i == 0 && (tot[0] > (u64)cap_runs || tot[1] > (u64)cap || bg_tot[0] > (u64)bg_cap_runs || bg_tot[1] > (u64)bg_cap))
        atomicOr((unsigned long long *)flags, CC_F_CAP);
    const u32 nruns = (u32)cc_count(tot, cap_runs), ncomp = (u32)cc_ncomp(tot, cap);
    const u32 nbg_comp = (u32)cc_ncomp(bg_tot, bg_cap);
    if (i >= cc_count(bg_tot, bg_cap_runs) || nruns == 0 || ncomp == 0 || nbg_comp == 0) return;
    const u32 run = (u32)i;
    if (bg_parent[run] != run) return;
    const u32 c = bg_rank[run];
    if (c >= nbg_comp) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    const u64 *box = bg_table + (int64_t)c * CC_COLS;
    const u64 nz = (u64)(nrows / ny);
    if (box[1] == 0 || box[2] + 1 >= nz || box[3] == 0 || box[4] + 1 >= (u64)ny || box[5] == 0 || box[6] + 1 >= (u64)nx) return;
    int64_t lo = 0, hi = nrows - 1;                         // the row of the run: the last one with bg_row_off[row] <= run
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (bg_row_off[mid] <= run) lo = mid;
        else hi = mid - 1;
    }
    const u32 first = bg_row_off[lo];
    const int s = first <= run ? cc_run_start(bg_bits + lo * wx, nx, wx, run - first) : -1;
    bool ok = s > 0;
    if (ok) {
        const int x = s - 1, wj = x >> 6, b = x & 63;
        const u64 *r = bits + lo * wx;
        const u64 cur = cc_word(r, nx, wx, wj);
        ok = ((cur >> b) & 1) != 0;
        if (ok) {
            const u64 starts = cc_starts(r, nx, wx, wj, cur);
            const u32 fr = cc_before(r, nx, wx, wj, row_off[lo]) + (u32)__popcll(starts & (~0ull >> (63 - b))) - 1;
            ok = fr < nruns;
            if (ok) {
                const u32 fc = cc_component(parent, rank, fr);
                ok = fc < ncomp;
                if (ok) atomicAdd(topo + 3 * (int64_t)fc + 1, 1ull);
            }
        }
    }
    if (!ok) atomicOr((unsigned long long *)flags, CC_F_RANGE);
}

// handles = 1 - euler + cavities
__global__ __launch_bounds__(CC_THREADS) void cc_handles_kernel(const u64 *__restrict__ tot, int64_t cap, u64 *__restrict__ topo)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= cc_ncomp(tot, cap)) return;
    topo[3 * c + 2] = 1ull - topo[3 * c] + topo[3 * c + 1];
}

TOMO_API int tomo_cc_cavities(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                              const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap,
                              const uint64_t *bg_bits, const uint32_t *bg_row_off, int64_t bg_cap_runs, const uint32_t *bg_parent,
                              const uint32_t *bg_rank, const unsigned long long *bg_tot, const int64_t *bg_table, int64_t bg_cap,
                              const int64_t *euler, int64_t *topo, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !euler || !topo || cap_runs <= 0 || cap <= 0 || bg_cap_runs < 0) return TOMO_E_ARG;
    if (bg_cap_runs > 0 && (!bg_bits || !bg_row_off || !bg_parent || !bg_rank || !bg_tot || !bg_table || bg_cap <= 0)) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || bg_cap_runs >= ((int64_t)1 << 31) || bg_cap >= ((int64_t)1 << 31))
        return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned comp_blocks = (unsigned)ceil_div64(cap, CC_THREADS);
    hipLaunchKernelGGL(cc_topology_init_kernel, dim3(comp_blocks), dim3(CC_THREADS), 0, st, (const u64 *)euler, (const u64 *)tot, cap,
                       (u64 *)topo);
    if (bg_cap_runs > 0)                                    // a full volume has no background run: nothing to attribute
        hipLaunchKernelGGL(cc_cavities_kernel, dim3((unsigned)ceil_div64(bg_cap_runs, CC_THREADS)), dim3(CC_THREADS), 0, st,
                           (const u64 *)bits, nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                           (const u32 *)rank, cap, (const u64 *)bg_bits, (const u32 *)bg_row_off, (const u64 *)bg_tot, bg_cap_runs,
                           (const u32 *)bg_parent, (const u32 *)bg_rank, (const u64 *)bg_table, bg_cap, (unsigned long long *)topo,
                           (u64 *)tot + 2);
    hipLaunchKernelGGL(cc_handles_kernel, dim3(comp_blocks), dim3(CC_THREADS), 0, st, (const u64 *)tot, cap, (u64 *)topo);
    return tomo_status();
}

// out[slot[c]] = (c + 1, voxels, euler, cavities, handles) for every selected component c (sel, slot, tot[5]: tomo_cc_zhist_offsets)
__global__ __launch_bounds__(CC_THREADS) void cc_topology_rows_kernel(const u64 *__restrict__ table, const u64 *__restrict__ topo,
                                                                      const u64 *__restrict__ tot, int64_t cap,
                                                                      const uint8_t *__restrict__ sel, const u32 *__restrict__ slot,
                                                                      u64 *__restrict__ out, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const bool fits = tot[5] <= (u64)cap_sel && tot[1] <= (u64)cap;
    if (c == 0 && !fits) atomicOr((unsigned long long *)flags, CC_F_CAP);
    if (!fits || c >= cc_ncomp(tot, cap) || !sel[c]) return;
    const u32 k = slot[c];
    if ((int64_t)k >= cap_sel) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    u64 *o = out + 5 * (int64_t)k;
    o[0] = (u64)c + 1;
    o[1] = table[c * CC_COLS];
    o[2] = topo[3 * c];
    o[3] = topo[3 * c + 1];
    o[4] = topo[3 * c + 2];
}

TOMO_API int tomo_cc_topology_rows(const int64_t *table, const int64_t *topo, int64_t cap, unsigned long long *tot, const uint8_t *sel,
                                   const uint32_t *slot, int64_t *out, int64_t cap_sel, void *stream)
{
    if (!table || !topo || !tot || !sel || !slot || !out || cap <= 0 || cap_sel <= 0) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_topology_rows_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u64 *)topo, (const u64 *)tot, cap, sel, (const u32 *)slot, (u64 *)out, cap_sel,
                       (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- components across Z-slabs
// A stack cut along z: rank r labels its slab with the kernels above (n_r components) and local component c gets the global
// id base_r + c, base_r = n_0 + ... + n_(r-1).  Global ids ascend in (rank, local raster order of the first voxel) = the
// raster order of the pieces' first voxels in the whole stack, so after uniting the pieces that touch across a cut with
// cc_union (larger root under smaller) the root of a component is the piece that holds its first voxel, and numbering the
// roots in ascending id is scipy's numbering of the whole stack.
//
// What travels: the last slice of a slab as bits + one int32 per run of it (the run's local component), and a WINDOW of the
// id table: rank r unites only ids of ranks r - 1 and r, so its table has n_(r-1) + n_r entries, ids relative to base_(r-1).
// Everything read from such a message is range-checked before it is used as an index (CC_F_RANGE).

// out[j] = local component of run j of slice z (j < runs of the slice), 0 behind them up to cap_out
__global__ __launch_bounds__(CC_THREADS) void cc_slice_components_kernel(int ny, int z, const u32 *__restrict__ row_off,
                                                                         const u64 *__restrict__ tot, int64_t cap,
                                                                         const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                                         int32_t *__restrict__ out, int64_t cap_out, u64 *flags)
{
    const int64_t j = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (j >= cap_out) return;
    const u32 nruns = (u32)cc_count(tot, cap);
    const u32 first = row_off[(int64_t)z * ny], last = row_off[(int64_t)(z + 1) * ny];
    int32_t c = 0;
    if (last < first || (int64_t)(last - first) > cap_out) {
        if (j == 0) atomicOr((unsigned long long *)flags, CC_F_CAP);
    } else if (j < (int64_t)(last - first)) {
        const u32 run = first + (u32)j;
        if (run < nruns) c = (int32_t)cc_component(parent, rank, run);
        else atomicOr((unsigned long long *)flags, CC_F_RANGE);
    }
    out[j] = c;
}

TOMO_API int tomo_cc_slice_components(int nz, int ny, int z, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                                      const uint32_t *rank, unsigned long long *tot, int32_t *out, int64_t cap_out, void *stream)
{
    if (nz <= 0 || ny <= 0 || z < 0 || z >= nz || !row_off || !parent || !rank || !tot || !out || cap_runs <= 0 || cap_out <= 0)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap_out >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_slice_components_kernel, dim3((unsigned)ceil_div64(cap_out, CC_THREADS)), dim3(CC_THREADS), 0,
                       (hipStream_t)stream, ny, z, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, out, cap_out, (u64 *)tot + 2);
    return tomo_status();
}

__global__ __launch_bounds__(CC_THREADS) void cc_iota_kernel(u32 *__restrict__ v, int64_t n, u64 *first, u64 value)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n) v[i] = (u32)i;
    if (i == 0 && first) *first = value;
}

// What one side of a seam needs to name the components of its runs: the slice's bits, its row offsets and, for the lower
// side, the received component of every run (comp; parent == NULL) or, for the upper side, the slab's own run tables.
struct CcSeamSide {
    const u64 *bits;
    const u32 *row_off;
    const u32 *parent, *rank;
    const int32_t *comp;
    u32 nruns;                  // run ids the tables hold
    u32 ncomp;                  // components of the side's slab
    u32 base;                   // id of its component 0 in the window
};

// window id of run i of a side, or ~0u (flag CC_F_RANGE) if the run or its component lies outside the side's tables
__device__ static inline u32 cc_seam_id(const CcSeamSide &s, u32 i, u64 *flags)
{
    if (i < s.nruns) {
        const u32 c = s.comp ? (u32)s.comp[i] : cc_component(s.parent, s.rank, i);     // a negative component is >= 2^31 here
        if (c < s.ncomp) return s.base + c;
    }
    atomicOr((unsigned long long *)flags, CC_F_RANGE);
    return ~0u;
}

// cc_pair_rows<2> between row y of the upper side's first slice and row yy of the lower side's last slice
__device__ static inline void cc_pair_seam(const CcSeamSide &up, const CcSeamSide &lo, int nx, int wx, int y, int yy, int widen,
                                           u32 *win, u64 *flags)
{
    CcRuns a = cc_runs_begin(up.bits, y, nx, wx), b = cc_runs_begin(lo.bits, yy, nx, wx);
    u32 ia = up.row_off[y], ib = lo.row_off[yy];
    while (a.valid && b.valid) {                            // every turn moves a or b on: at most runs(a) + runs(b) turns
        if (a.s < b.e + widen && b.s < a.e + widen) {
            const u32 ga = cc_seam_id(up, ia, flags), gb = cc_seam_id(lo, ib, flags);
            if (ga == ~0u || gb == ~0u) return;
            cc_union(win, ga, gb);
        }
        if (a.e <= b.e) {
            cc_runs_next(a);
            ia++;
        } else {
            cc_runs_next(b);
            ib++;
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_seam_union_kernel(CcSeamSide up, CcSeamSide lo, const u64 *__restrict__ tot, int64_t cap,
                                                                u32 nb_runs, int ny, int nx, int wx, int widen, u32 *win, u64 *flags)
{
    const int y = blockIdx.x * CC_THREADS + threadIdx.x;
    if (y >= ny) return;
    up.nruns = (u32)cc_count(tot, cap);
    if (y == 0 && lo.row_off[ny] != nb_runs) atomicOr((unsigned long long *)flags, CC_F_RANGE);   // the message and its bits disagree
    cc_pair_seam(up, lo, nx, wx, y, y, widen, win, flags);
    if (widen) {
        if (y > 0) cc_pair_seam(up, lo, nx, wx, y, y - 1, widen, win, flags);
        if (y + 1 < ny) cc_pair_seam(up, lo, nx, wx, y, y + 1, widen, win, flags);
    }
}

TOMO_API int tomo_cc_seam_union(const uint64_t *bits, int ny, int nx, int connectivity, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, const unsigned long long *tot, const uint64_t *nb_bits,
                                const uint32_t *nb_row_off, const int32_t *nb_comp, int64_t nb_runs, int64_t n_prev, int64_t n_own,
                                uint32_t *win, unsigned long long *seam_tot, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, 1, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !nb_bits || !nb_row_off || !nb_comp || !win || !seam_tot || cap_runs <= 0 ||
        nb_runs <= 0 || n_prev <= 0 || n_own <= 0 || (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || nb_runs >= ((int64_t)1 << 31) || n_prev + n_own >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(seam_tot, 0, 8 * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_iota_kernel, dim3((unsigned)ceil_div64(n_prev + n_own, CC_THREADS)), dim3(CC_THREADS), 0, st, (u32 *)win,
                       n_prev + n_own, (u64 *)nullptr, (u64)0);
    const CcSeamSide up = {(const u64 *)bits, (const u32 *)row_off, (const u32 *)parent, (const u32 *)rank, nullptr, 0u, (u32)n_own,
                           (u32)n_prev};
    const CcSeamSide lo = {(const u64 *)nb_bits, (const u32 *)nb_row_off, nullptr, nullptr, nb_comp, (u32)nb_runs, (u32)n_prev, 0u};
    hipLaunchKernelGGL(cc_seam_union_kernel, dim3((unsigned)ceil_div64(ny, CC_THREADS)), dim3(CC_THREADS), 0, st, up, lo,
                       (const u64 *)tot, cap_runs, (u32)nb_runs, ny, nx, wx, connectivity == 26 ? 1 : 0, (u32 *)win, (u64 *)seam_tot + 2);
    return tomo_status();
}

// The gathered step-3 messages, one row of `stride` int64 per rank: [0] the seam's flags, [1 .. 1 + n_r) the sizes of the
// rank's components, from word off_win on its window as int32.  bases (device int64[world + 1]): base_r, the last = N.
__global__ __launch_bounds__(CC_THREADS) void cc_fold_kernel(const int64_t *__restrict__ msg, int64_t stride, int64_t off_win,
                                                          const int64_t *__restrict__ bases, int64_t n_total, u32 *table, u64 *flags)
{
    const int r = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int64_t *row = msg + (int64_t)r * stride;
    if (i == 0 && row[0] != 0) atomicOr((unsigned long long *)flags, (unsigned long long)row[0]);
    if (r == 0) return;                                     // the lowest slab has no seam below it
    const int64_t lo = bases[r - 1], wlen = bases[r + 1] - lo;
    if (lo < 0 || wlen < 0 || lo + wlen > n_total || 2 * (stride - off_win) < wlen) {
        if (i == 0) atomicOr((unsigned long long *)flags, CC_F_CAP);
        return;
    }
    if (i >= wlen) return;
    const u32 t = (u32)((const int32_t *)(row + off_win))[i];
    if (t >= (u32)wlen) {
        atomicOr((unsigned long long *)flags, CC_F_RANGE);
        return;
    }
    if (t != (u32)i) cc_union(table, (u32)(lo + i), (u32)(lo + t));
}

// sizes[number of the root of base_r + c] += the size rank r found for its component c
__global__ __launch_bounds__(CC_THREADS) void cc_fold_sizes_kernel(const int64_t *__restrict__ msg, int64_t stride, int64_t off_win,
                                                                const int64_t *__restrict__ bases, int64_t n_total,
                                                                const u32 *__restrict__ table, const u32 *__restrict__ num,
                                                                unsigned long long *__restrict__ sizes, u64 *flags)
{
    const int r = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int64_t lo = bases[r], n = bases[r + 1] - lo;
    if (lo < 0 || n < 0 || lo + n > n_total || n > off_win - 1) {
        if (c == 0) atomicOr((unsigned long long *)flags, CC_F_CAP);
        return;
    }
    if (c >= n) return;
    const u32 k = cc_component(table, num, (u32)(lo + c));
    if (k < (u32)n_total) atomicAdd(sizes + k, (unsigned long long)msg[(int64_t)r * stride + 1 + c]);
    else atomicOr((unsigned long long *)flags, CC_F_RANGE);
}

TOMO_API int tomo_cc_merge_tables(const int64_t *msg, int world, int64_t stride, int64_t off_win, const int64_t *bases,
                                  int64_t n_total, int64_t max_n, int64_t max_win, uint32_t *table, uint32_t *num, int64_t *sizes,
                                  uint64_t *blk, unsigned long long *tot, void *stream)
{
    if (!msg || !bases || !table || !num || !sizes || !blk || !tot || world <= 0 || world > 65535 || n_total <= 0 || max_n <= 0 ||
        max_n > n_total || max_win < 0 || max_win > n_total || off_win < 1 + max_n || stride < off_win + (max_win + 1) / 2)
        return TOMO_E_ARG;
    if (n_total >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    u64 *t = (u64 *)tot;
    const unsigned all_blocks = (unsigned)ceil_div64(n_total, CC_THREADS);
    if (hipMemsetAsync(tot, 0, 8 * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    if (hipMemsetAsync(sizes, 0, (size_t)n_total * sizeof(int64_t), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(cc_iota_kernel, dim3(all_blocks), dim3(CC_THREADS), 0, st, (u32 *)table, n_total, t, (u64)n_total);
    hipLaunchKernelGGL(cc_fold_kernel, dim3((unsigned)ceil_div64(max_win > 0 ? max_win : 1, CC_THREADS), (unsigned)world),
                       dim3(CC_THREADS), 0, st, msg, stride, off_win, bases, n_total, (u32 *)table, t + 2);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(all_blocks), dim3(CC_THREADS), 0, st, (u32 *)table, (const u64 *)nullptr, n_total,
                       (u32 *)num);
    cc_scan((u32 *)num, nullptr, n_total, (u64 *)blk, t + 1, nullptr, st);
    hipLaunchKernelGGL(cc_fold_sizes_kernel, dim3((unsigned)ceil_div64(max_n, CC_THREADS), (unsigned)world), dim3(CC_THREADS), 0, st,
                       msg, stride, off_win, bases, n_total, (const u32 *)table, (const u32 *)num, (unsigned long long *)sizes, t + 2);
    return tomo_status();
}

// what filter and expand look up per LOCAL component c of the slab at `base`: keep[c] (the keep rule on the global sizes)
// and / or label[c] (the global label)
__global__ __launch_bounds__(CC_THREADS) void cc_local_maps_kernel(const u32 *__restrict__ table, const u32 *__restrict__ num,
                                                                const unsigned long long *__restrict__ sizes, const u64 *__restrict__ tot,
                                                                int64_t n_total, int64_t base, int64_t n_local, u64 min_voxels,
                                                                int largest, uint8_t *__restrict__ keep, int32_t *__restrict__ label,
                                                                u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= n_local) return;
    const u32 k = cc_component(table, num, (u32)(base + c));
    const bool ok = k < (u32)n_total && (u64)k < tot[1];
    if (!ok) atomicOr((unsigned long long *)flags, CC_F_RANGE);
    if (keep) keep[c] = ok && (largest ? (u64)k + 1 == tot[3] : sizes[k] >= min_voxels) ? 1 : 0;
    if (label) label[c] = ok ? (int32_t)(k + 1) : 0;
}

TOMO_API int tomo_cc_local_maps(const uint32_t *table, const uint32_t *num, const int64_t *sizes, unsigned long long *tot,
                                int64_t n_total, int64_t base, int64_t n_local, int64_t min_voxels, int largest, uint8_t *keep,
                                int32_t *label, void *stream)
{
    if (!table || !num || !sizes || !tot || (!keep && !label) || n_total <= 0 || base < 0 || n_local <= 0 || base + n_local > n_total ||
        min_voxels < 0)
        return TOMO_E_ARG;
    if (n_total >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (keep && largest)
        hipLaunchKernelGGL(cc_largest_kernel<1>, dim3(1), dim3(1024), 0, st, (const unsigned long long *)sizes, (u64 *)tot, n_total,
                           n_total, (u64)min_voxels);
    hipLaunchKernelGGL(cc_local_maps_kernel, dim3((unsigned)ceil_div64(n_local, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u32 *)table, (const u32 *)num, (const unsigned long long *)sizes, (const u64 *)tot, n_total, base, n_local,
                       (u64)min_voxels, largest ? 1 : 0, keep, label, (u64 *)tot + 2);
    return tomo_status();
}

TOMO_API int tomo_cc_filter_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *keep,
                                int64_t n_local, uint64_t *out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !keep || !out || out == bits || cap_runs <= 0 || n_local <= 0 || n_local > cap_runs)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;
    hipLaunchKernelGGL(cc_filter_kernel<true>, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, (const unsigned long long *)nullptr, (u64)0, 0, keep, (u32)n_local, (u64 *)out, (u64 *)tot + 2);
    return tomo_status();
}

TOMO_API int tomo_cc_expand_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int32_t *label,
                                int64_t n_local, int32_t *labels, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !label || !labels || cap_runs <= 0 || n_local <= 0 || n_local > cap_runs)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;
    hipLaunchKernelGGL(cc_expand_kernel<true>, dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, label, (u32)n_local, labels, (u64 *)tot + 2);
    return tomo_status();
}
