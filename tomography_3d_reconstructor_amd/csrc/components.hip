// components.hip -- connected-component labelling, component sizes and island removal on the resident bit volume
// (scipy.ndimage.label with generate_binary_structure(3, 1) or (3, 3); no counterpart in the reference, whose only defence
// against debris is the opening of voxel_processor.py:88).
//
// The unit of work is the X-RUN, a maximal run of set bits in a row, never the voxel.  Run ids are handed out in raster order
// (exclusive scan of the runs per row), every run starts as its own tree (linked to its first neighbour in the row above, which
// needs no atomic), overlapping runs of neighbouring rows are united by hooking the larger root under the smaller one with
// a compare-and-swap, and the trees are flattened in a launch of their own.  A root is the smallest run id of its component = the
// component's first run in raster order, so numbering the roots with a scan IS scipy's numbering, whatever the schedule did.
// Sizes are integer atomics per component.  Nothing here holds a per-voxel array except tomo_cc_expand's output.
//
// Termination: parent[r] <= r always and a parent only ever decreases (the swap of a root, atomicMin or a store of a smaller
// ancestor); cc_find follows strictly decreasing ids; a turn of cc_union's loop that does not end it has seen another thread
// hook a root, which happens fewer times than there are runs.  No kernel waits for
// another workgroup: the phases are separate launches.
//
// The vocabulary of the run tables and the layout of tot are in cc_runs.h; what is measured per component on these tables
// is in component_measures.hip.
#include "cc_runs.h"

TOMO_API int64_t tomo_cc_scan_blocks(int64_t n)
{
    if (n <= 0) return TOMO_E_ARG;
    return ceil_div64(n, CC_SCAN_TILE) + 1;
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
// (cc_count: n from the host or from device memory; cc_scan1_kernel: the one-workgroup scan of the tile sums -- cc_runs.h)
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

// ---------------------------------------------------------------------------------------------- labelling: union-find over runs (cc_runs.h)
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
            cc_flag(flags, CC_F_RANGE);
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
    if (row == 0 && tot[0] > (u64)cap) cc_flag(flags, CC_F_CAP);
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
    CcSumAcc acc = {sizes, nruns, 0};                       // a component's number is below the count of runs
    u32 comp = 0;
    if (row < nrows) comp = cc_row_walk<false>(bits, row, nx, wx, row_off, nruns, parent, rank, flags, acc);
    cc_wave_tail<false>(comp, 0u, acc);
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

// ---------------------------------------------------------------------------------------------- labels per voxel
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
                const u32 run = cc_run_at(bf, s, lane);
                const u32 c = run < nruns ? cc_component(parent, rank, run) : ~0u;
                if (run < nruns && (!MAP || c < nmap)) lab = MAP ? map[c] : (int32_t)(c + 1);
                else cc_flag(flags, CC_F_RANGE);
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

// ---------------------------------------------------------------------------------------------- the keep rule (cc_largest_kernel: cc_runs.h)
// out word = the bits of the word's runs whose component is kept (MAP: kept = map[c] != 0 for c < nmap, whatever the sizes say;
// SOLID: ORed with the word of a second volume, its bits at x >= nx cleared)
template <bool MAP, bool SOLID>
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                               const u32 *__restrict__ row_off, const u64 *__restrict__ tot, int64_t cap,
                                                               const u32 *__restrict__ parent, const u32 *__restrict__ rank,
                                                               const unsigned long long *__restrict__ sizes, u64 min_voxels, int largest,
                                                               const uint8_t *__restrict__ map, u32 nmap,
                                                               const u64 *__restrict__ solid, u64 *__restrict__ out, u64 *flags)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= nwords) return;
    const u32 nruns = (u32)cc_count(tot, cap);
    const u64 only = !MAP && largest ? tot[3] : 0;
    const int64_t row = i / wx;
    const int wj = (int)(i - row * wx);
    const u64 *r = bits + row * wx;
    const u64 m = cc_word(r, nx, wx, wj);
    u64 res = SOLID ? solid[i] & cc_tail_mask(nx, wx, wj) : 0;
    if (m) {
        CcWordRuns it = cc_word_runs(r, nx, wx, wj, m, row_off[row]);
        while (cc_word_runs_next(it)) {
            if (it.run < nruns) {
                const u32 c = cc_component(parent, rank, it.run);
                bool keep;
                if (MAP) {
                    keep = c < nmap && map[c] != 0;
                    if (c >= nmap) cc_flag(flags, CC_F_RANGE);
                } else {
                    keep = largest ? (u64)c + 1 == only : (c < nruns && sizes[c] >= min_voxels);
                }
                if (keep) res |= it.mask;
            } else {
                cc_flag(flags, CC_F_RANGE);
            }
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
    hipLaunchKernelGGL((cc_filter_kernel<false, false>), dim3((unsigned)ceil_div64(nwords, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, (const unsigned long long *)sizes, (u64)min_voxels, largest ? 1 : 0, (const uint8_t *)nullptr, 0u,
                       (const u64 *)nullptr, (u64 *)out, (u64 *)tot + 2);
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
        if (j == 0) cc_flag(flags, CC_F_CAP);
    } else if (j < (int64_t)(last - first)) {
        const u32 run = first + (u32)j;
        if (run < nruns) c = (int32_t)cc_component(parent, rank, run);
        else cc_flag(flags, CC_F_RANGE);
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
    cc_flag(flags, CC_F_RANGE);
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
    if (y == 0 && lo.row_off[ny] != nb_runs) cc_flag(flags, CC_F_RANGE);   // the message and its bits disagree
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
    if (i == 0 && row[0] != 0) cc_flag(flags, (unsigned long long)row[0]);
    if (r == 0) return;                                     // the lowest slab has no seam below it
    const int64_t lo = bases[r - 1], wlen = bases[r + 1] - lo;
    if (lo < 0 || wlen < 0 || lo + wlen > n_total || 2 * (stride - off_win) < wlen) {
        if (i == 0) cc_flag(flags, CC_F_CAP);
        return;
    }
    if (i >= wlen) return;
    const u32 t = (u32)((const int32_t *)(row + off_win))[i];
    if (t >= (u32)wlen) {
        cc_flag(flags, CC_F_RANGE);
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
        if (c == 0) cc_flag(flags, CC_F_CAP);
        return;
    }
    if (c >= n) return;
    const u32 k = cc_component(table, num, (u32)(lo + c));
    if (k < (u32)n_total) atomicAdd(sizes + k, (unsigned long long)msg[(int64_t)r * stride + 1 + c]);
    else cc_flag(flags, CC_F_RANGE);
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
    if (!ok) cc_flag(flags, CC_F_RANGE);
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

// the keep map applied to the runs of `bits`; solid (may be NULL): a second volume of the same geometry every word is ORed with
TOMO_API int tomo_cc_fill_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                              const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *keep,
                              int64_t n_local, const uint64_t *solid, uint64_t *out, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !keep || !out || out == bits || out == solid || cap_runs <= 0 || n_local <= 0 ||
        n_local > cap_runs)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t nwords = nrows * wx;
    const dim3 grid((unsigned)ceil_div64(nwords, CC_THREADS)), block(CC_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (solid)
        hipLaunchKernelGGL((cc_filter_kernel<true, true>), grid, block, 0, st, (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off,
                           (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank, (const unsigned long long *)nullptr, (u64)0, 0,
                           keep, (u32)n_local, (const u64 *)solid, (u64 *)out, (u64 *)tot + 2);
    else
        hipLaunchKernelGGL((cc_filter_kernel<true, false>), grid, block, 0, st, (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off,
                           (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank, (const unsigned long long *)nullptr, (u64)0, 0,
                           keep, (u32)n_local, (const u64 *)nullptr, (u64 *)out, (u64 *)tot + 2);
    return tomo_status();
}

TOMO_API int tomo_cc_filter_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *keep,
                                int64_t n_local, uint64_t *out, void *stream)
{
    return tomo_cc_fill_map(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, keep, n_local, nullptr, out, stream);
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
