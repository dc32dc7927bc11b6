// component_measures.hip -- what is measured per component on the run tables of components.hip: the measurement table
// (voxels, box, index sums), the selection and its slice histograms (voxels, or six moment sums, per component and slice),
// volume and centroid in mm, second moments and principal axes, Euler number, cavities and handles, surface area and
// mean breadth (Crofton), what a per-voxel array gives per component (the inscribed sphere from the distance map, voxels per
// thickness level), and caliper diameters along shared directions and along a component's own axes.
// Every pass over the rows is an accumulator for the row pass of cc_runs.h -- over the runs, or, where a voxel's neighbours
// decide (Euler number, surface area, mean breadth), over the words of the row with windows of the neighbour rows slid along;
// the integer tables are integer atomics only, the float results are sequential sums over those integers (nothing is
// contracted in this file: -ffp-contract=off).
#include "cc_runs.h"

// ---------------------------------------------------------------------------------------------- measurements per component
// table (device int64[cap][CC_COLS]), row c = component c + 1: [0] voxels  [1, 2] zmin, zmax  [3, 4] ymin, ymax  [5, 6] xmin,
// xmax (inclusive indices)  [7] sum of z over the voxels  [8] sum of y  [9] sum of x.  Every entry is a non-negative integer
// below 2^63, so the kernels work on it as u64 and the 64-bit unsigned min / max / add atomics keep it exact and the same on
// every run.  The count of components comes from tot[1]; more than the table's rows: nothing is touched (CC_F_CAP).

// the minima start at the largest int64 (a memset cannot give that), everything else at 0
__global__ __launch_bounds__(CC_THREADS) void cc_table_init_kernel(u64 *__restrict__ table, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= cap * CC_COLS) return;
    const int col = (int)(i % CC_COLS);
    table[i] = (col == 1 || col == 3 || col == 5) ? 0x7fffffffffffffffull : 0ull;
}

// what a thread, or a wave, flushes for ONE component
struct CcMeasureSum {
    u64 *table;
    u32 ncomp;
    u64 vox, sz, sy, sx;
    u32 z0, z1, y0, y1, x0, x1;
    __device__ bool any() const { return vox != 0; }
    __device__ void flush(u32 c) const
    {
        if (c >= ncomp) return;
        u64 *t = table + (int64_t)c * CC_COLS;
        atomicAdd(t + 0, vox);
        atomicMin(t + 1, (u64)z0);
        atomicMax(t + 2, (u64)z1);
        atomicMin(t + 3, (u64)y0);
        atomicMax(t + 4, (u64)y1);
        atomicMin(t + 5, (u64)x0);
        atomicMax(t + 6, (u64)x1);
        atomicAdd(t + 7, sz);
        atomicAdd(t + 8, sy);
        atomicAdd(t + 9, sx);
    }
};

// The accumulator of row (z, y): a run [s, e) adds len = e - s voxels and len * (s + e - 1) / 2 = s + (s + 1) + .. + (e - 1)
// (len or s + e - 1 is even: exact) and widens the box in x; the record multiplies the voxels by z and y.  A wave combines
// once whatever slices its rows lie in -- every lane brings its own z and y: ten atomics per 64 rows of one solid body.
struct CcMeasureAcc {
    u64 *table;
    u32 ncomp, z, y;
    u64 vox, sx;
    u32 x0, x1;
    __device__ bool any() const { return vox != 0; }
    __device__ u32 begin(u32 c, const CcRuns &a)
    {
        vox = sx = 0;
        x0 = (u32)a.s;
        return c;
    }
    __device__ void add(const CcRuns &a)
    {
        const u64 len = (u64)(a.e - a.s);
        vox += len;
        sx += len * (u64)(a.s + a.e - 1) / 2;
        x1 = (u32)(a.e - 1);                                // the runs ascend
    }
    __device__ CcMeasureSum record() const { return {table, ncomp, vox, vox * z, vox * y, sx, z, z, y, y, x0, x1}; }
    __device__ void flush(u32 c) const { record().flush(c); }
    __device__ CcMeasureSum combine(bool has, u32) const
    {
        const CcMeasureSum m = record();
        return {table, ncomp, wave_sum64(m.vox), wave_sum64(has ? m.sz : 0), wave_sum64(has ? m.sy : 0), wave_sum64(m.sx),
                wave_min32(has ? m.z0 : ~0u), wave_max32(has ? m.z1 : 0u), wave_min32(has ? m.y0 : ~0u), wave_max32(has ? m.y1 : 0u),
                wave_min32(has ? m.x0 : ~0u), wave_max32(has ? m.x1 : 0u)};       // vox and sx are 0 where nothing is held
    }
};

__global__ __launch_bounds__(CC_THREADS) void cc_measure_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                int64_t cap_runs, const u32 *__restrict__ parent,
                                                                const u32 *__restrict__ rank, u64 *__restrict__ table, int64_t cap,
                                                                u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    if (row == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    const bool live = row < nrows;
    CcMeasureAcc acc = {table, (u32)cc_ncomp(tot, cap), live ? (u32)(row / ny) : 0u, live ? (u32)(row % ny) : 0u, 0, 0, 0, 0};
    u32 comp = 0;
    if (live) comp = cc_row_walk<false>(bits, row, nx, wx, row_off, nruns, parent, rank, flags, acc);
    cc_wave_tail<false>(comp, acc.z, acc);
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
// The keep rule, in full: the size window min_voxels <= voxels <= max_voxels on column 0 -- largest: only the label in tot[3]
// -- and, with enclosed, only a component whose box touches no face of the stack (cc_enclosed): a cavity, where the table is
// the complement's.  Both scan kernels apply it through cc_selected, nothing else does.
struct CcRule {
    u64 min_voxels, max_voxels;
    int largest, enclosed;
    u64 nz, ny, nx;
};

// the inclusive index box of a row of the measurement table touches no face of the stack
__device__ static inline bool cc_enclosed(const u64 *__restrict__ box, u64 nz, u64 ny, u64 nx)
{
    return !(box[1] == 0 || box[2] + 1 >= nz || box[3] == 0 || box[4] + 1 >= ny || box[5] == 0 || box[6] + 1 >= nx);
}

__device__ static inline bool cc_selected(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t c, const CcRule &r)
{
    if (r.largest) return (u64)c + 1 == tot[3];
    const u64 *row = table + c * CC_COLS;
    return row[0] >= r.min_voxels && row[0] <= r.max_voxels && (!r.enclosed || cc_enclosed(row, r.nz, r.ny, r.nx));
}

// length of the segment of component c (0: not selected, or a box that is none)
__device__ static inline u64 cc_zspan(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t c, const CcRule &r, bool *sel)
{
    const u64 z0 = table[c * CC_COLS + 1], z1 = table[c * CC_COLS + 2];
    *sel = cc_selected(table, tot, c, r);
    return *sel && z1 >= z0 ? z1 - z0 + 1 : 0;
}


// per tile of CC_SCAN_TILE components: blk[b] = its counters, blk[nblk + b] = its selected components; sel[c] on the way
__global__ __launch_bounds__(CC_THREADS) void cc_zspan_blocksum_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                       int64_t cap, CcRule rule,
                                                                       uint8_t *__restrict__ sel, u64 *__restrict__ blk, int64_t nblk,
                                                                       u64 *flags)
{
    __shared__ u64 wsum[2][CC_THREADS / 64];
    const int64_t n = cc_ncomp(tot, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + 4 * threadIdx.x;
    u64 span = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n) {
            bool s;
            span += cc_zspan(table, tot, i0 + j, rule, &s);
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
                                                                    int64_t cap, CcRule rule,
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
        x[j] = i0 + j < n ? cc_zspan(table, tot, i0 + j, rule, &s) : 0;
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

TOMO_API int tomo_cc_select(const int64_t *table, int64_t cap, unsigned long long *tot, int64_t min_voxels, int64_t max_voxels,
                            int largest, int enclosed, int nz, int ny, int nx, uint8_t *sel, uint64_t *off, uint32_t *slot, uint64_t *blk,
                            void *stream)
{
    if (!table || !tot || !sel || !off || !slot || !blk || cap <= 0 || min_voxels < 0 || max_voxels < 0) return TOMO_E_ARG;
    if (largest && (enclosed || max_voxels != (int64_t)0x7fffffffffffffffll)) return TOMO_E_ARG;
    if (enclosed && (nz <= 0 || ny <= 0 || nx <= 0)) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const u64 *t = (const u64 *)table;
    u64 *tt = (u64 *)tot;
    const int64_t nblk = ceil_div64(cap, CC_SCAN_TILE);
    const CcRule rule = {(u64)min_voxels, (u64)max_voxels, largest ? 1 : 0, enclosed ? 1 : 0, (u64)nz, (u64)ny, (u64)nx};
    if (largest)                                            // no run table is read here: only the count of components is capped
        hipLaunchKernelGGL(cc_largest_kernel<CC_COLS>, dim3(1), dim3(1024), 0, st, (const unsigned long long *)t, tt, cap,
                           (int64_t)0x7fffffffffffffffll, (u64)min_voxels);
    hipLaunchKernelGGL(cc_zspan_blocksum_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, t, (const u64 *)tt, cap, rule, sel,
                       (u64 *)blk, nblk, tt + 2);
    hipLaunchKernelGGL(cc_scan1_kernel, dim3(1), dim3(1024), 0, st, (u64 *)blk, nblk, tt + 4, (u64 *)nullptr);
    hipLaunchKernelGGL(cc_scan1_kernel, dim3(1), dim3(1024), 0, st, (u64 *)blk + nblk, nblk, tt + 5, (u64 *)nullptr);
    hipLaunchKernelGGL(cc_zspan_apply_kernel, dim3((unsigned)nblk), dim3(CC_THREADS), 0, st, t, (const u64 *)tt, cap, rule,
                       (const u64 *)blk, nblk, (u64 *)off, (u32 *)slot);
    return tomo_status();
}

// the rule without an upper bound and without the face test
TOMO_API int tomo_cc_zhist_offsets(const int64_t *table, int64_t cap, unsigned long long *tot, int64_t min_voxels, int largest,
                                   uint8_t *sel, uint64_t *off, uint32_t *slot, uint64_t *blk, void *stream)
{
    return tomo_cc_select(table, cap, tot, min_voxels, (int64_t)0x7fffffffffffffffll, largest, 0, 0, 0, 0, sel, off, slot, blk, stream);
}

// ---------------------------------------------------------------------------------------------- sums per component and slice
// The segments of tomo_cc_zhist_offsets hold SUMS words per entry: hist[SUMS * (off[c] + z - zmin) + k].  One word is the
// count of voxels (tomo_cc_zhist).  CC_MOMS words are what second moments need (tomo_cc_moment_hist): a set voxel (k, j, i) of
// component c is a point mass at (zc[k], j * mm_y, i * mm_x) of weight w[k] = (mm_x * mm_y) * depth[k], and per slice of the
// component's box six integer sums over the slice's voxels of the component do, taken about the box corner (j' = j - ymin,
// i' = i - xmin) to keep them small: N, sum j', sum i', sum j'^2, sum i'^2, sum j' i'.
#define CC_MOMS 6                    // sums per component and slice
#define CC_MOMENT_COLS 22            // doubles per row of tomo_cc_moments' output
#define CC_JACOBI_SWEEPS 32          // limit of the cyclic Jacobi iteration (a 3 x 3 matrix is done in 5 or 6)

// 0^2 + 1^2 + .. + (n - 1)^2 = (n - 1) n (2 n - 1) / 6; n <= nx, and tomo_cc_moment_hist refuses max(ny, nx)^3 >= 2^63
__device__ static inline u64 cc_squares_below(u64 n)
{
    return (n - 1) * n * (2 * n - 1) / 6;                   // n = 0: the wrapped factor meets a 0
}

// The accumulator of row (z, y) of the histogram pass (cc_runs.h), over the runs (NR == 0); only the runs of selected components
// count.  A run [s, e) adds its length and, SUMS > 1, in closed form the sums of i' and i'^2 over it; the row supplies the factors
// j' when a record is made.  A voxel in front of the box corner (the bits changed since tomo_cc_measure) is CC_F_RANGE and adds
// nothing; with one sum the corner is never read.
template <int SUMS>
struct CcSliceAcc {
    using Extra = CcOneVolume;
    static constexpr int WORDS = SUMS, NR = 0;
    static constexpr bool UNLABELLED = false, WALKS_EMPTY = true, SQUARES = SUMS > 1;
    CcHist h;
    const uint8_t *sel;
    u32 ncomp, z, y;
    u64 n, si, sii;
    u64 x0, jp;                                             // the component's box corner in x, the row's j' in its box
    __device__ CcSliceAcc(const CcHistArgs &a, u64 total, u32 ncomp, u32 z, u32 y)
        : h{a.table, a.off, a.hist, total, a.flags}, sel(a.sel), ncomp(ncomp), z(z), y(y), n(0), si(0), sii(0), x0(0), jp(0)
    {
    }
    __device__ u32 filter(u32 c) const { return (c - 1 >= ncomp || !sel[c - 1]) ? 0u : c; }
    __device__ bool any() const { return n != 0; }
    __device__ u32 begin(u32 c, const CcRuns &)
    {
        n = si = sii = 0;
        if constexpr (SUMS > 1) {
            if (c) {
                const u64 y0 = h.table[(int64_t)(c - 1) * CC_COLS + 3];
                x0 = h.table[(int64_t)(c - 1) * CC_COLS + 5];
                jp = (u64)y - y0;
                if ((u64)y < y0) {
                    cc_flag(h.flags, CC_F_RANGE);
                    return 0;
                }
            }
        }
        return c;
    }
    __device__ void add(const CcRuns &a)
    {
        if constexpr (SUMS == 1) {
            n += (u64)(a.e - a.s);
        } else if ((u64)a.s < x0) {
            cc_flag(h.flags, CC_F_RANGE);
        } else {
            const u64 s = (u64)a.s - x0, e = (u64)a.e - x0, len = e - s;
            n += len;
            si += len * (s + e - 1) / 2;                    // len or s + e - 1 is even: exact
            sii += cc_squares_below(e) - cc_squares_below(s);
        }
    }
    __device__ CcSliceSum<SUMS> record() const
    {
        if constexpr (SUMS == 1) return {h, z, {n}};
        else return {h, z, {n, jp * n, si, jp * jp * n, sii, jp * si}};
    }
    __device__ void flush(u32 c) const { record().flush(c); }
    __device__ CcSliceSum<SUMS> combine(bool mine, u32 zz) const
    {
        const CcSliceSum<SUMS> r = record();
        CcSliceSum<SUMS> w = {h, zz};
#pragma unroll
        for (int k = 0; k < SUMS; k++) w.v[k] = wave_sum64(mine ? r.v[k] : 0);
        return w;
    }
};

TOMO_API int tomo_cc_zhist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                           const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                           const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, void *stream)
{
    return cc_hist_launch<CcSliceAcc<1>>(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, hist, hist_cap, true,
                                         {}, stream);
}

TOMO_API int tomo_cc_moment_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                 const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table,
                                 int64_t cap, const uint8_t *sel, const uint64_t *off, uint64_t *mom, int64_t hist_cap, void *stream)
{
    return cc_hist_launch<CcSliceAcc<CC_MOMS>>(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, mom, hist_cap,
                                               true, {}, stream);
}

// ---------------------------------------------------------------------------------------------- per selected component: its segment
struct CcSegment {
    u64 z0, z1, o;                                          // its slices and where their entries start
    u32 k;                                                  // its row in the compacted results
};

// One thread per component c -> true and the segment if c is selected and everything fits; thread 0 flags what does not fit
// (CC_F_CAP: nothing is written at all), a segment outside the stack or the histogram is CC_F_RANGE.
__device__ static inline bool cc_segment(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                         const uint8_t *__restrict__ sel, const u64 *__restrict__ off, const u32 *__restrict__ slot,
                                         int64_t hist_cap, int nz, int64_t cap_sel, int64_t c, u64 *flags, CcSegment &s)
{
    const u64 total = tot[4];
    if (!cc_selected(tot, cap, sel, slot, cap_sel, c, flags, s.k, total <= (u64)hist_cap)) return false;
    s.z0 = table[c * CC_COLS + 1];
    s.z1 = table[c * CC_COLS + 2];
    s.o = off[c];
    if (s.z1 < s.z0 || s.z1 >= (u64)nz || s.o + (s.z1 - s.z0) >= total) {
        cc_flag(flags, CC_F_RANGE);
        return false;
    }
    return true;
}

// ... and with table == NULL, the histogram of a call without labelling: thread 0 takes the slices 0 .. nz - 1 into row 0
__device__ static inline bool cc_slices(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                        const uint8_t *__restrict__ sel, const u64 *__restrict__ off, const u32 *__restrict__ slot,
                                        int64_t hist_cap, int nz, int64_t cap_sel, int64_t c, u64 *flags, CcSegment &s)
{
    if (table) return cc_segment(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, s);
    s = {0, (u64)nz - 1, 0, 0};
    return c == 0;
}

// The checks every finishing entry point makes of the arguments they share, the arguments first (TOMO_E_ARG), then the sizes
// (TOMO_E_SIZE).  ok: what the entry point asks of arguments of its own; words: uint64 per entry of the histogram, read only once
// ok holds.  unlabelled: the entry point has the form without tables -- table == NULL, hist_cap >= nz.
static int cc_finish_check(bool unlabelled, const void *table, int64_t cap, const void *tot, const void *sel, const void *off,
                           const void *slot, const void *hist, int64_t hist_cap, int nz, int64_t cap_sel, int64_t words, bool ok)
{
    const bool labelled = table || !unlabelled;
    if (!ok || !hist || hist_cap <= 0 || nz <= 0 || cap_sel <= 0) return TOMO_E_ARG;
    if (labelled && (!table || !tot || !sel || !off || !slot || cap <= 0)) return TOMO_E_ARG;
    if (!labelled && hist_cap < nz) return TOMO_E_ARG;
    if (cap_sel >= ((int64_t)1 << 31) || hist_cap >= ((int64_t)1 << 60) / words || (labelled && cap >= ((int64_t)1 << 31)))
        return TOMO_E_SIZE;
    return TOMO_OK;
}

// what `count` voxels of a slice of weight w, centred at zc, add to a component's volume and z moment -> the slice's volume.
// Plain sequential float64: over the slices in ascending z, vol is the float a host loop over the slices of the mask
// `labels == c` gives -- the slices outside the box add 0.0 there.
__device__ static inline double cc_slice_volume(u64 count, double w, double zc, double &vol, double &mz)
{
    const double v = (double)count * w;
    vol += v;
    mz += v * zc;
    return v;
}

// One thread per component; a selected one walks its slices in ascending z.  out[slot[c]] = (vol, mz), labels[slot[c]] = c + 1.
__global__ __launch_bounds__(CC_THREADS) void cc_zsums_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                                              const uint8_t *__restrict__ sel, const u64 *__restrict__ off,
                                                              const u32 *__restrict__ slot, const u64 *__restrict__ hist,
                                                              int64_t hist_cap, const double *__restrict__ w,
                                                              const double *__restrict__ zc, int nz, double *__restrict__ out,
                                                              int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    CcSegment s;
    if (!cc_segment(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, s)) return;
    double vol = 0.0, mz = 0.0;
    for (u64 z = s.z0; z <= s.z1; z++) cc_slice_volume(hist[s.o + (z - s.z0)], w[z], zc[z], vol, mz);
    out[2 * (int64_t)s.k] = vol;
    out[2 * (int64_t)s.k + 1] = mz;
    labels[s.k] = c + 1;
}

TOMO_API int tomo_cc_zsums(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                           const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *w, const double *zc, int nz,
                           double *out, int64_t *labels, int64_t cap_sel, void *stream)
{
    const int r = cc_finish_check(false, table, cap, tot, sel, off, slot, hist, hist_cap, nz, cap_sel, 1, w && zc && out && labels);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(cc_zsums_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot, (const u64 *)hist, hist_cap,
                       w, zc, nz, out, labels, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- second moments per component
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
// float64.  First walk: W and the z moment by cc_zsums_kernel's very additions (cc_slice_volume), and
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
    CcSegment seg;
    if (!cc_segment(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, seg)) return;
    const u64 z0 = seg.z0, z1 = seg.z1;
    const u32 k = seg.k;
    const u64 *m = mom + CC_MOMS * seg.o;
    const double zo = zc[z0];
    double vol = 0.0, mz = 0.0, sz = 0.0, sy = 0.0, sx = 0.0;
    for (u64 z = z0; z <= z1; z++) {
        const u64 *s = m + CC_MOMS * (z - z0);
        const double v = cc_slice_volume(s[0], w[z], zc[z], vol, mz);
        sz += v * (zc[z] - zo);
        sy += w[z] * (double)s[1];
        sx += w[z] * (double)s[2];
    }
    if (!(vol > 0.0)) {                                     // no voxel arrived in the segment: the bits changed
        cc_flag(flags, CC_F_RANGE);
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
    // (a NaN fails every comparison)
    const bool ok = w && zc && out && labels && mm_y > 0.0 && mm_y < __builtin_inf() && mm_x > 0.0 && mm_x < __builtin_inf();
    const int r = cc_finish_check(false, table, cap, tot, sel, off, slot, mom, hist_cap, nz, cap_sel, CC_MOMS, ok);
    if (r != TOMO_OK) return r;
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
// (CcWin, cc_xp, cc_xm and the window walk itself: cc_runs.h)
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

// the rows cc_euler_terms reads, in the order of its win[]
template <int K>
struct CcEulerRows;
template <>
struct CcEulerRows<6> {
    static constexpr int NR = 4;
    static constexpr CcRowAt ROWS[NR] = {{0, 0, 0}, {0, 1, 0}, {1, 0, 0}, {1, 1, 0}};
};
template <>
struct CcEulerRows<26> {
    static constexpr int NR = 5;
    static constexpr CcRowAt ROWS[NR] = {{0, 0, 0}, {0, -1, 0}, {-1, 0, 0}, {-1, -1, 0}, {-1, 1, 0}};
};

// chi per component: the terms of a word once, their popcounts under every run's mask
template <int K>
struct CcEulerAcc : CcSumAcc {
    u64 pos[CC_EULER_POS], neg[CC_EULER_NEG];
    __device__ void word(const CcWin *win) { cc_euler_terms<K>(win, pos, neg); }
    __device__ void add(const CcWin *, u64 mask) { sum += cc_euler_under(pos, neg, mask); }
};

// The window walk with the rows the terms of chi read; a wave whose lanes all hold the same component adds once, then one signed
// 64-bit atomic add (two's complement on u64) into euler[rank[parent[run]]].  Not LABELLED: everything goes to euler[0] -- the
// Euler number of the whole volume.
template <int K, bool LABELLED>
__global__ __launch_bounds__(CC_THREADS) void cc_euler_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                              const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                              int64_t cap_runs, const u32 *__restrict__ parent,
                                                              const u32 *__restrict__ rank, unsigned long long *__restrict__ euler,
                                                              int64_t cap, u64 *flags)
{
    constexpr int NR = CcEulerRows<K>::NR;
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = LABELLED ? (u32)cc_count(tot, cap_runs) : 0u;
    const u32 ncomp = LABELLED ? (u32)cc_ncomp(tot, cap) : 1u;
    if (LABELLED && row == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    u32 comp = 0;                                           // component + 1 the thread is adding up, 0: none
    CcEulerAcc<K> acc = {{euler, ncomp, 0}, {}, {}};
    if (row < nrows) {
        const u64 *r[NR];
        cc_rows<CcEulerRows<K>>(r, bits, nullptr, row, nrows, ny, wx, (int)(row % ny));
        comp = cc_window_walk<NR, LABELLED, false>(r, nx, wx, LABELLED ? row_off[row] : 0u, nruns, parent, rank, flags, acc);
    }
    cc_wave_tail<false>(comp, 0u, acc);
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

// The tables both sides of a cavity: the volume's (bits .. cap) and those of the BACKGROUND (the complement, labelled under the
// complementary connectivity; bg_table = its measurement table).
struct CcCavityIn {
    const u64 *bits;
    int64_t nrows;
    int ny, nx, wx;
    const u32 *row_off;
    const u64 *tot;
    int64_t cap_runs;
    const u32 *parent, *rank;
    int64_t cap;
    const u64 *bg_bits;
    const u32 *bg_row_off;
    const u64 *bg_tot;
    int64_t bg_cap_runs;
    const u32 *bg_parent, *bg_rank;
    const u64 *bg_table;
    int64_t bg_cap;
};

// Background run i.  A run that is its own root is the first run of its component in raster order; if the component's box
// touches no face of the stack it is a cavity, the voxel left of the run's start is set and belongs to the foreground
// component that encloses it: its run is found as cc_expand_kernel maps a bit to a run.  -> true: *bc = the background
// component, *fc = its owner (both 0-based, both inside their tables).  The guards of the tables are flagged here.
__device__ static inline bool cc_cavity_owner(const CcCavityIn &a, int64_t i, u32 *bc, u32 *fc, u64 *flags)
{
    if (i == 0 && (a.tot[0] > (u64)a.cap_runs || a.tot[1] > (u64)a.cap || a.bg_tot[0] > (u64)a.bg_cap_runs || a.bg_tot[1] > (u64)a.bg_cap))
        cc_flag(flags, CC_F_CAP);
    const u32 nruns = (u32)cc_count(a.tot, a.cap_runs), ncomp = (u32)cc_ncomp(a.tot, a.cap);
    const u32 nbg_comp = (u32)cc_ncomp(a.bg_tot, a.bg_cap);
    if (i >= cc_count(a.bg_tot, a.bg_cap_runs) || nruns == 0 || ncomp == 0 || nbg_comp == 0) return false;
    const u32 run = (u32)i;
    if (a.bg_parent[run] != run) return false;
    const u32 c = a.bg_rank[run];
    if (c >= nbg_comp) {
        cc_flag(flags, CC_F_RANGE);
        return false;
    }
    if (!cc_enclosed(a.bg_table + (int64_t)c * CC_COLS, (u64)(a.nrows / a.ny), (u64)a.ny, (u64)a.nx)) return false;
    int64_t lo = 0, hi = a.nrows - 1;                       // the row of the run: the last one with bg_row_off[row] <= run
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.bg_row_off[mid] <= run) lo = mid;
        else hi = mid - 1;
    }
    const u32 first = a.bg_row_off[lo];
    const int s = first <= run ? cc_run_start(a.bg_bits + lo * a.wx, a.nx, a.wx, run - first) : -1;
    bool ok = s > 0;
    if (ok) {
        const int x = s - 1, wj = x >> 6, b = x & 63;
        const u64 *r = a.bits + lo * a.wx;
        const u64 cur = cc_word(r, a.nx, a.wx, wj);
        ok = ((cur >> b) & 1) != 0;
        if (ok) {
            const u32 fr = cc_run_of_bit(r, a.nx, a.wx, wj, b, a.row_off[lo]);
            ok = fr < nruns;
            if (ok) {
                *fc = cc_component(a.parent, a.rank, fr);
                *bc = c;
                ok = *fc < ncomp;
            }
        }
    }
    if (!ok) cc_flag(flags, CC_F_RANGE);
    return ok;
}

// one thread per run of the background: the owner of a cavity counts one more
__global__ __launch_bounds__(CC_THREADS) void cc_cavities_kernel(CcCavityIn a, unsigned long long *__restrict__ topo, u64 *flags)
{
    u32 bc, fc;
    if (cc_cavity_owner(a, (int64_t)blockIdx.x * CC_THREADS + threadIdx.x, &bc, &fc, flags)) atomicAdd(topo + 3 * (int64_t)fc + 1, 1ull);
}

// ... or is written down: owner[c] = the label of the owner of background component c + 1 (one root per component: one store)
__global__ __launch_bounds__(CC_THREADS) void cc_cavity_owners_kernel(CcCavityIn a, u64 *__restrict__ owner, u64 *flags)
{
    u32 bc, fc;
    if (cc_cavity_owner(a, (int64_t)blockIdx.x * CC_THREADS + threadIdx.x, &bc, &fc, flags)) owner[bc] = (u64)fc + 1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_zero64_kernel(u64 *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n) out[i] = 0;
}

// handles = 1 - euler + cavities
__global__ __launch_bounds__(CC_THREADS) void cc_handles_kernel(const u64 *__restrict__ tot, int64_t cap, u64 *__restrict__ topo)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= cc_ncomp(tot, cap)) return;
    topo[3 * c + 2] = 1ull - topo[3 * c] + topo[3 * c + 1];
}

// the argument head tomo_cc_cavities and tomo_cc_cavity_owners share: checked, then gathered for the kernels
static int cc_cavity_in(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                        const uint32_t *rank, const unsigned long long *tot, int64_t cap, const uint64_t *bg_bits,
                        const uint32_t *bg_row_off, int64_t bg_cap_runs, const uint32_t *bg_parent, const uint32_t *bg_rank,
                        const unsigned long long *bg_tot, const int64_t *bg_table, int64_t bg_cap, CcCavityIn *a)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || cap_runs <= 0 || cap <= 0 || bg_cap_runs < 0) return TOMO_E_ARG;
    if (bg_cap_runs > 0 && (!bg_bits || !bg_row_off || !bg_parent || !bg_rank || !bg_tot || !bg_table || bg_cap <= 0)) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || bg_cap_runs >= ((int64_t)1 << 31) || bg_cap >= ((int64_t)1 << 31))
        return TOMO_E_SIZE;
    *a = {(const u64 *)bits, nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank,
          cap, (const u64 *)bg_bits, (const u32 *)bg_row_off, (const u64 *)bg_tot, bg_cap_runs, (const u32 *)bg_parent,
          (const u32 *)bg_rank, (const u64 *)bg_table, bg_cap};
    return TOMO_OK;
}

TOMO_API int tomo_cc_cavities(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                              const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap,
                              const uint64_t *bg_bits, const uint32_t *bg_row_off, int64_t bg_cap_runs, const uint32_t *bg_parent,
                              const uint32_t *bg_rank, const unsigned long long *bg_tot, const int64_t *bg_table, int64_t bg_cap,
                              const int64_t *euler, int64_t *topo, void *stream)
{
    CcCavityIn a;
    const int g = cc_cavity_in(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, bg_bits, bg_row_off, bg_cap_runs, bg_parent,
                               bg_rank, bg_tot, bg_table, bg_cap, &a);
    if (g != TOMO_OK) return g;
    if (!euler || !topo) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned comp_blocks = (unsigned)ceil_div64(cap, CC_THREADS);
    hipLaunchKernelGGL(cc_topology_init_kernel, dim3(comp_blocks), dim3(CC_THREADS), 0, st, (const u64 *)euler, (const u64 *)tot, cap,
                       (u64 *)topo);
    if (bg_cap_runs > 0)                                    // a full volume has no background run: nothing to attribute
        hipLaunchKernelGGL(cc_cavities_kernel, dim3((unsigned)ceil_div64(bg_cap_runs, CC_THREADS)), dim3(CC_THREADS), 0, st, a,
                           (unsigned long long *)topo, (u64 *)tot + 2);
    hipLaunchKernelGGL(cc_handles_kernel, dim3(comp_blocks), dim3(CC_THREADS), 0, st, (const u64 *)tot, cap, (u64 *)topo);
    return tomo_status();
}

TOMO_API int tomo_cc_cavity_owners(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                   const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap,
                                   const uint64_t *bg_bits, const uint32_t *bg_row_off, int64_t bg_cap_runs, const uint32_t *bg_parent,
                                   const uint32_t *bg_rank, const unsigned long long *bg_tot, const int64_t *bg_table, int64_t bg_cap,
                                   int64_t *owner, void *stream)
{
    CcCavityIn a;
    const int g = cc_cavity_in(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, bg_bits, bg_row_off, bg_cap_runs, bg_parent,
                               bg_rank, bg_tot, bg_table, bg_cap, &a);
    if (g != TOMO_OK) return g;
    if (bg_cap_runs == 0) return TOMO_OK;                   // a full volume has no background component: nothing to write
    if (!owner) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_zero64_kernel, dim3((unsigned)ceil_div64(bg_cap, CC_THREADS)), dim3(CC_THREADS), 0, st, (u64 *)owner, bg_cap);
    hipLaunchKernelGGL(cc_cavity_owners_kernel, dim3((unsigned)ceil_div64(bg_cap_runs, CC_THREADS)), dim3(CC_THREADS), 0, st, a,
                       (u64 *)owner, (u64 *)tot + 2);
    return tomo_status();
}

// out[slot[c]] = (c + 1, voxels, euler, cavities, handles) for every selected component c (sel, slot, tot[5]: tomo_cc_zhist_offsets)
struct CcTopologyRow {
    static constexpr int COLS = 5;
    const u64 *__restrict__ table, *__restrict__ topo;
    __device__ void write(u64 *__restrict__ o, int64_t c) const
    {
        o[0] = (u64)c + 1;
        o[1] = table[c * CC_COLS];
        o[2] = topo[3 * c];
        o[3] = topo[3 * c + 1];
        o[4] = topo[3 * c + 2];
    }
};

TOMO_API int tomo_cc_topology_rows(const int64_t *table, const int64_t *topo, int64_t cap, unsigned long long *tot, const uint8_t *sel,
                                   const uint32_t *slot, int64_t *out, int64_t cap_sel, void *stream)
{
    return cc_rows_launch(CcTopologyRow{(const u64 *)table, (const u64 *)topo}, table && topo, cap, tot, sel, slot, out, cap_sel, stream);
}

// ---------------------------------------------------------------------------------------------- surface area (Crofton)
// The discretised Crofton formula: per set voxel p of slice k and each of its 26 neighbours q that is clear or outside the
// stack, one count in column c of slice k, for the component of p; c by (|dz|, |dy|, |dx|) of q - p and the sign of dz:
//   0, 1, 2: x, y, xy in the slice    3 .. 6: z, xz, yz, xyz towards slice k + 1    7 .. 10: the same towards slice k - 1
// A set neighbour of another component (diagonal contact under connectivity 6) is no transition, so only the bits decide: per
// word the 26 words `t & ~neighbour`, popcounted under each run's mask.  The area is the sequential float64 sum over the
// slices of count * factor (tomo_cc_surface); the factors carry the spacing and the direction weights (pipeline.py).
// (CC_SURF counters per component and slice, CC_SURF_CLASSES with up and down folded: cc_runs.h)
// the bits of mask whose neighbour in row r is clear: at the same x -> centre, at x + 1 and at x - 1 -> side
__device__ static inline void cc_clear_beside(const CcWin &r, u64 mask, u64 &centre, u64 &side)
{
    centre += (u64)__popcll(mask & ~r.cur);
    side += (u64)(__popcll(mask & ~cc_xp(r)) + __popcll(mask & ~cc_xm(r)));
}

// The accumulator of row (z, y) of the histogram pass (cc_runs.h), for the window walk over the row, (z, y - 1), (z, y + 1), then
// (z + 1, y - 1 .. y + 1), then (z - 1, y - 1 .. y + 1).  Every run ends at a clear bit or at the edge of the stack, so n[0] != 0
// wherever a voxel was seen.
struct CcSurfaceAcc : CcCounts<CC_SURF, false> {
    using CcCounts::CcCounts;
    using Extra = CcOneVolume;
    static constexpr bool UNLABELLED = true;
    static constexpr int NR = 9;
    static constexpr CcRowAt ROWS[NR] = {{0, 0, 0}, {0, -1, 0}, {0, 1, 0}, {1, -1, 0}, {1, 0, 0}, {1, 1, 0}, {-1, -1, 0}, {-1, 0, 0}, {-1, 1, 0}};
    __device__ void add(const CcWin *win, u64 mask)
    {
        u64 self = 0;                                       // a bit of the mask is set in the row itself
        cc_clear_beside(win[0], mask, self, n[0]);
        cc_clear_beside(win[1], mask, n[1], n[2]);
        cc_clear_beside(win[2], mask, n[1], n[2]);
        cc_clear_beside(win[3], mask, n[5], n[6]);
        cc_clear_beside(win[4], mask, n[3], n[4]);
        cc_clear_beside(win[5], mask, n[5], n[6]);
        cc_clear_beside(win[6], mask, n[9], n[10]);
        cc_clear_beside(win[7], mask, n[7], n[8]);
        cc_clear_beside(win[8], mask, n[9], n[10]);
    }
};

TOMO_API int tomo_cc_surface_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                  const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table,
                                  int64_t cap, const uint8_t *sel, const uint64_t *off, uint64_t *surf, int64_t hist_cap, void *stream)
{
    return cc_hist_launch<CcSurfaceAcc>(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, surf, hist_cap, true,
                                        {}, stream);
}

// One thread per component, as cc_zsums_kernel; a selected one walks its slices in ascending z and the columns 0 .. 10 of
// each: S += (double)count * F[z][column], plain sequential float64.  directions == 3: only the columns of x, y and z enter the
// sum (the factors of the others are 0 there).  table == NULL: no labelling, thread 0 sums the slices 0 .. nz - 1 into row 0.
__global__ __launch_bounds__(CC_THREADS) void cc_surface_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                                                const uint8_t *__restrict__ sel, const u64 *__restrict__ off,
                                                                const u32 *__restrict__ slot, const u64 *__restrict__ surf,
                                                                int64_t hist_cap, const double *__restrict__ F, int nz, int directions,
                                                                double *__restrict__ out, u64 *__restrict__ counts,
                                                                int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    CcSegment s;
    if (!cc_slices(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, s)) return;
    const u64 *m = surf + CC_SURF * s.o;
    double area = 0.0;
    u64 n[CC_SURF_CLASSES] = {};
    for (u64 z = s.z0; z <= s.z1; z++) {
#pragma unroll
        for (int k = 0; k < CC_SURF; k++) {
            const u64 v = m[CC_SURF * (z - s.z0) + k];
            if (directions == 13 || k == 0 || k == 1 || k == 3 || k == 7) area += (double)v * F[CC_SURF * z + k];
            n[k < CC_SURF_CLASSES ? k : k - 4] += v;
        }
    }
    out[s.k] = area;
#pragma unroll
    for (int k = 0; k < CC_SURF_CLASSES; k++) counts[CC_SURF_CLASSES * (int64_t)s.k + k] = n[k];
    labels[s.k] = c + 1;
}

TOMO_API int tomo_cc_surface(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                             const uint32_t *slot, const uint64_t *surf, int64_t hist_cap, const double *F, int nz, int directions,
                             double *out, int64_t *counts, int64_t *labels, int64_t cap_sel, void *stream)
{
    const bool ok = F && out && counts && labels && (directions == 3 || directions == 13);
    const int r = cc_finish_check(true, table, cap, tot, sel, off, slot, surf, hist_cap, nz, cap_sel, CC_SURF, ok);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(cc_surface_kernel, dim3(table ? (unsigned)ceil_div64(cap, CC_THREADS) : 1u), dim3(CC_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot,
                       (const u64 *)surf, hist_cap, F, nz, directions, out, (u64 *)counts, labels, cap_sel,
                       tot ? (u64 *)tot + 2 : (u64 *)nullptr);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- mean breadth (Crofton)
// The fourth Minkowski functional: b = sum over the 13 families m of lattice planes of c_m * delta_m * chi_m, chi_m the sum over
// the planes of the family of the 2-D Euler number V - E + F of the section (include/tomo_hip.h has the cells per family).  Every
// cell is anchored at its raster-first corner p: filed in the slice of p, for the component of p, its other corners being any
// set bits of the forward neighbourhood -- the row at x + 1, row (z, y + 1) and the rows (z + 1, y - 1 .. y + 1) at x - 1 ..
// x + 1: five windows.  Per word the cells are ANDs of the run's mask with the shifted forward words, popcounted.
// An entry of the histogram holds CC_BREADTH words (cc_runs.h):
//   0 .. 5   the cells inside the slice, raw: voxels, edges along x, along y, along (0, 1, 1), along (0, 1, -1), squares x y
//   6 .. 17  chi_m^cross = faces - edges of the cells with corners in slice k + 1, signed (two's complement, wrapping adds), for
//            the families in ascending order without (1, 0, 0), which has no such cell
// tomo_cc_breadth forms chi_m^in = voxels - edges (+ squares for (1, 0, 0)) from the six raw counts.
// The accumulator of row (z, y) of the histogram pass (cc_runs.h); n[0] counts the voxels themselves.
struct CcBreadthAcc : CcCounts<CC_BREADTH, false> {
    using CcCounts::CcCounts;
    using Extra = CcOneVolume;
    static constexpr bool UNLABELLED = true;
    static constexpr int NR = 5;
    // win: 0 the row, 1 row (z, y + 1), 2 .. 4 rows (z + 1, y - 1), (z + 1, y), (z + 1, y + 1)
    static constexpr CcRowAt ROWS[NR] = {{0, 0, 0}, {0, 1, 0}, {1, -1, 0}, {1, 0, 0}, {1, 1, 0}};
    __device__ void add(const CcWin *win, u64 t)
    {
        const u64 a = t & cc_xp(win[0]);                                        // p and p + x
        const u64 Bc = win[1].cur, Bp = cc_xp(win[1]), Bm = cc_xm(win[1]);
        const u64 Dc = win[2].cur, Dp = cc_xp(win[2]);
        const u64 Ec = win[3].cur, Ep = cc_xp(win[3]), Em = cc_xm(win[3]);
        const u64 Gc = win[4].cur, Gp = cc_xp(win[4]), Gm = cc_xm(win[4]);
        const u64 tz = t & Ec, tEp = t & Ep, tEm = t & Em, tDc = t & Dc, tGc = t & Gc, ty = t & Bc;
        const u64 ez = (u64)__popcll(tz), eEp = (u64)__popcll(tEp), eEm = (u64)__popcll(tEm), eDc = (u64)__popcll(tDc),
                  eGc = (u64)__popcll(tGc);
        n[0] += (u64)__popcll(t);
        n[1] += (u64)__popcll(a);
        n[2] += (u64)__popcll(ty);
        n[3] += (u64)__popcll(t & Bp);
        n[4] += (u64)__popcll(t & Bm);
        n[5] += (u64)__popcll(a & Bc & Bp);
        n[6] += (u64)__popcll(ty & Ec & Gc) - ez;                               // (0, 0, 1): squares y z - edges z
        n[7] += (u64)__popcll(tz & Bp & Gp) - ez;                               // (0, 1, -1): rectangles z, (0, 1, 1)
        n[8] += (u64)__popcll(a & Ec & Ep) - ez;                                // (0, 1, 0): squares x z
        n[9] += (u64)__popcll(tz & Bm & Gm) - ez;                               // (0, 1, 1): rectangles z, (0, 1, -1)
        n[10] += (u64)__popcll(tGc & Bm) + (u64)__popcll(tGc & Ep) - eGc - eEp; // (1, -1, -1): (0, 1, -1), (1, 1, 0), (1, 0, 1)
        n[11] += (u64)__popcll(a & Gc & Gp) - eGc;                              // (1, -1, 0): rectangles x, (1, 1, 0)
        n[12] += (u64)__popcll(tGc & Bp) + (u64)__popcll(tGc & Em) - eGc - eEm; // (1, -1, 1): (0, 1, 1), (1, 1, 0), (1, 0, -1)
        n[13] += (u64)__popcll(ty & Ep & Gp) - eEp;                             // (1, 0, -1): rectangles y, (1, 0, 1)
        n[14] += (u64)__popcll(ty & Em & Gm) - eEm;                             // (1, 0, 1): rectangles y, (1, 0, -1)
        n[15] += (u64)__popcll(tEp & Bp) + (u64)__popcll(tEp & Dc) - eEp - eDc; // (1, 1, -1): (0, 1, 1), (1, 0, 1), (1, -1, 0)
        n[16] += (u64)__popcll(a & Dc & Dp) - eDc;                              // (1, 1, 0): rectangles x, (1, -1, 0)
        n[17] += (u64)__popcll(tEm & Bm) + (u64)__popcll(tEm & Dc) - eEm - eDc; // (1, 1, 1): (0, 1, -1), (1, 0, -1), (1, -1, 0)
    }
};

TOMO_API int tomo_cc_breadth_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                  const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table,
                                  int64_t cap, const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, void *stream)
{
    return cc_hist_launch<CcBreadthAcc>(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, hist, hist_cap, true,
                                        {}, stream);
}

// One thread per component, as cc_surface_kernel; a selected one walks its slices in ascending z and per slice the columns
// 0 .. 25 of B: 0 .. 12 the families' chi^in at the slice's own depth, 13 .. 25 their chi^cross at the mean depth towards slice
// k + 1: b += (double)(int64)chi * B[z][column], plain sequential float64.  directions == 3: only the columns of (0, 0, 1),
// (0, 1, 0) and (1, 0, 0) enter.  table == NULL: no labelling, thread 0 sums the slices 0 .. nz - 1 into row 0.
__global__ __launch_bounds__(CC_THREADS) void cc_breadth_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot, int64_t cap,
                                                                const uint8_t *__restrict__ sel, const u64 *__restrict__ off,
                                                                const u32 *__restrict__ slot, const u64 *__restrict__ hist,
                                                                int64_t hist_cap, const double *__restrict__ B, int nz, int directions,
                                                                double *__restrict__ out, u64 *__restrict__ euler,
                                                                int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    CcSegment s;
    if (!cc_slices(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, s)) return;
    double b = 0.0;
    u64 chi[CC_BREADTH_FAMILIES] = {};
    for (u64 z = s.z0; z <= s.z1; z++) {
        const u64 *m = hist + CC_BREADTH * (s.o + (z - s.z0));
        const double *F = B + 2 * CC_BREADTH_FAMILIES * z;
        const u64 v = m[0], ex = m[1], ey = m[2], ep = m[3], em = m[4];
        const u64 in[CC_BREADTH_FAMILIES] = {v - ey, v - ep, v - ex, v - em, v - em, v - ex, v - ep, v - ey, v - ex - ey + m[5],
                                             v - ey, v - ep, v - ex, v - em};
#pragma unroll
        for (int f = 0; f < CC_BREADTH_FAMILIES; f++) {
            if (directions == 13 || f == 0 || f == 2 || f == 8) b += (double)(int64_t)in[f] * F[f];
            chi[f] += in[f];
        }
#pragma unroll
        for (int f = 0; f < CC_BREADTH_FAMILIES; f++) {
            const u64 x = f == 8 ? 0ull : m[CC_BREADTH_IN + (f < 8 ? f : f - 1)];
            if (directions == 13 || f == 0 || f == 2 || f == 8) b += (double)(int64_t)x * F[CC_BREADTH_FAMILIES + f];
            chi[f] += x;
        }
    }
    out[s.k] = b;
#pragma unroll
    for (int f = 0; f < CC_BREADTH_FAMILIES; f++) euler[CC_BREADTH_FAMILIES * (int64_t)s.k + f] = chi[f];
    labels[s.k] = c + 1;
}

TOMO_API int tomo_cc_breadth(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                             const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *B, int nz, int directions,
                             double *out, int64_t *section_euler, int64_t *labels, int64_t cap_sel, void *stream)
{
    const bool ok = B && out && section_euler && labels && (directions == 3 || directions == 13);
    const int r = cc_finish_check(true, table, cap, tot, sel, off, slot, hist, hist_cap, nz, cap_sel, CC_BREADTH, ok);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(cc_breadth_kernel, dim3(table ? (unsigned)ceil_div64(cap, CC_THREADS) : 1u), dim3(CC_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot,
                       (const u64 *)hist, hist_cap, B, nz, directions, out, (u64 *)section_euler, labels, cap_sel,
                       tot ? (u64 *)tot + 2 : (u64 *)nullptr);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- per-voxel values: inscribed sphere, thickness
// What a per-voxel array gives per component: the maximum of the inside distance with the first voxel that attains it (the
// inscribed sphere), and the voxels per slice and thickness level.  Distance and local thickness are local to a component --
// the nearest site of a voxel of A is never a voxel of another component, and a ball that fits lies in the component of its
// centre -- so ONE transform of the whole volume serves every component, and what is left is a reduction over the run tables.
// The WORD PASS (cc_runs.h): one wave per 64-bit word of a row, one lane per bit (edt_at_least_kernel's shape), so that the
// per-voxel array is read in whole 256- or 512-byte rows.  The runs that touch the word are walked by all lanes together
// (CcWordRuns: the word, hence every run and its component, is wave-uniform); a lane takes part under the run's mask.

// the float32 bits of the value of a SET voxel: the distance map itself, or (float)sqrt(d2) -- what EDT_TAIL_FLOAT stores
__device__ static inline u32 cc_value_bits(const float *__restrict__ dist, const double *__restrict__ d2, int64_t at)
{
    return __float_as_uint(dist ? dist[at] : (float)sqrt(d2[at]));
}

// best[c] = the largest float32 bit pattern over component c + 1 (values >= 0: unsigned order is float order); FIRST: first[c] =
// the smallest flat index whose value has the bits best[c].  Per run of the word one wave reduction and at most one atomic: a
// maximum that does not beat what best[c] already holds is not sent (one solid body would otherwise queue every word of the
// volume on one address), and only the runs that attain the maximum send an index -- and of those only the ones whose index is
// below what first[c] already shows (a map that is constant over a body, all 0.0 or all +inf, would queue every word again).
template <bool FIRST>
struct CcValuePass {
    using Lane = u32;
    static constexpr bool SELECTED = false;
    const float *__restrict__ dist;
    const double *__restrict__ d2;
    u32 *best;
    unsigned long long *__restrict__ first;
    __device__ bool fits(const u64 *) const { return true; }
    __device__ u32 load(const CcWordArgs &, const u64 *, const CcWordAt &, bool set, int64_t at) const { return set ? cc_value_bits(dist, d2, at) : 0u; }
    __device__ void run(const CcWordArgs &, const CcWordAt &w, u32 c, bool mine, u32 v, int64_t at) const
    {
        if constexpr (!FIRST) {
            const u32 top = wave_max32(mine ? v : 0u);          // best[c] only rises: a stale read costs an atomic, never the answer
            if (w.bit == 0 && top > cc_load(best + c)) atomicMax(best + c, top);
        } else {
            const u64 hit = __ballot(mine && v == best[c]);
            if (hit && w.bit == 0) {                            // first[c] only falls: a stale read costs an atomic, never the answer
                const u64 cand = (u64)(at + (__ffsll((long long)hit) - 1));     // at is the flat index of the word's bit 0 here
                if (cand < cc_load64((const u64 *)first + c)) atomicMin(first + c, (unsigned long long)cand);
            }
        }
    }
    std::array<CcClear, 1> clears(int64_t cap) const
    {
        return {FIRST ? CcClear{first, 0xff, (size_t)cap * sizeof(u64)} : CcClear{best, 0, (size_t)cap * sizeof(u32)}};
    }
    // host: the arrays are given; dist and d2 both given, or both NULL, is refused
    bool ok(const void *) const { return best && (!FIRST || first) && (dist != nullptr) != (d2 != nullptr); }
};

TOMO_API int tomo_cc_value_max(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                               const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *dist,
                               const double *d2, uint32_t *best, int64_t cap, void *stream)
{
    const CcValuePass<false> p = {dist, d2, (u32 *)best, nullptr};
    return cc_word_launch(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

TOMO_API int tomo_cc_value_first(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                 const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *dist,
                                 const double *d2, const uint32_t *best, uint64_t *first, int64_t cap, void *stream)
{
    if ((const void *)best == (const void *)first) return TOMO_E_ARG;       // before the geometry is judged
    const CcValuePass<true> p = {dist, d2, (u32 *)best, (unsigned long long *)first};
    return cc_word_launch(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

// out[slot[c]] = (c + 1, voxels, best[c], first[c]) for every selected component c (sel, slot, tot[5]: tomo_cc_select)
struct CcValueRow {
    static constexpr int COLS = 4;
    const u64 *__restrict__ table;
    const u32 *__restrict__ best;
    const u64 *__restrict__ first;
    __device__ void write(u64 *__restrict__ o, int64_t c) const
    {
        o[0] = (u64)c + 1;
        o[1] = table[c * CC_COLS];
        o[2] = best[c];
        o[3] = first[c];
    }
};

TOMO_API int tomo_cc_value_rows(const int64_t *table, const uint32_t *best, const uint64_t *first, int64_t cap, unsigned long long *tot,
                                const uint8_t *sel, const uint32_t *slot, int64_t *out, int64_t cap_sel, void *stream)
{
    return cc_rows_launch(CcValueRow{(const u64 *)table, (const u32 *)best, (const u64 *)first}, table && best && first, cap, tot, sel,
                          slot, out, cap_sel, stream);
}

// hist[(K + 1) * (off[c] + z - zmin[c]) + level] += 1 for every set voxel of a selected component; level: the int32 level map of
// the local thickness, outside 0 .. K it counts as 0.  The word pass; inside a run the lanes are aggregated by level: the first
// lane still to count names its level, the lanes that share it are balloted, the leader adds their number, they retire -- a
// solid body costs one or two atomics per word, not 64.
struct CcLevelPass {
    struct Lane {
        int l;                                              // the level of the lane's voxel
        u64 z, total;                                       // wave-uniform, computed once per word: its slice, the histogram's entries
    };
    static constexpr bool SELECTED = true;
    const u64 *__restrict__ table;
    const uint8_t *__restrict__ sel;
    const u64 *__restrict__ off;
    unsigned long long *__restrict__ hist;
    int64_t hist_cap;
    const int32_t *__restrict__ level;
    int K;
    __device__ bool fits(const u64 *tot) const { return tot[4] <= (u64)hist_cap; }      // a histogram that is too short: nothing is touched
    __device__ Lane load(const CcWordArgs &a, const u64 *tot, const CcWordAt &w, bool set, int64_t at) const
    {
        const int l = set ? level[at] : 0;
        return {(unsigned)l > (unsigned)K ? 0 : l, (u64)(w.row / a.ny), tot[4]};      // nothing writes such a level; never index past the entry
    }
    __device__ void run(const CcWordArgs &a, const CcWordAt &w, u32 c, bool, const Lane &v, int64_t) const
    {
        const u64 z0 = table[(int64_t)c * CC_COLS + 1], z1 = table[(int64_t)c * CC_COLS + 2];
        const u64 pos = off[c] + (v.z - z0);
        if (v.z < z0 || v.z > z1 || pos >= v.total) {       // a slice outside the component's box: the bits changed
            if (w.bit == 0) cc_flag(a.flags, CC_F_RANGE);
            return;
        }
        unsigned long long *entry = hist + (u64)(K + 1) * pos;
        u64 left = w.it.mask;                               // the lanes still to count, wave-uniform
        while (left) {                                      // every turn retires at least the leader: at most 64 turns
            const int leader = __ffsll((long long)left) - 1;
            const int ll = __shfl(v.l, leader, 64);
            const u64 same = __ballot(v.l == ll) & left;
            if (w.bit == leader) atomicAdd(entry + ll, (unsigned long long)__popcll(same));
            left &= ~same;
        }
    }
    std::array<CcClear, 1> clears(int64_t) const { return {CcClear{hist, 0, (size_t)hist_cap * ((size_t)K + 1) * sizeof(u64)}}; }
};

TOMO_API int tomo_cc_level_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                                const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, const int32_t *level,
                                int levels, void *stream)
{
    int64_t nrows;
    int wx;
    const bool ok = level && levels >= 0 && (const void *)hist != (const void *)level;
    const int r = cc_hist_check(false, bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, table, cap, sel, off, hist, hist_cap,
                                (int64_t)levels + 1, ok, &nrows, &wx);
    if (r != TOMO_OK) return r;
    const CcLevelPass p = {(const u64 *)table, sel, (const u64 *)off, (unsigned long long *)hist, hist_cap, level, levels};
    return cc_word_go(bits, nrows, ny, nx, wx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

// One thread per (component, level); a selected component walks its slices in ascending z: voxels[slot[c]][level] = the sum of the
// counts, volume[slot[c]][level - 1] = acc, acc = acc + (double)count * w[z], plain sequential float64 (cc_zsums_kernel's
// discipline: the float a host loop over ALL slices of the mask gives, the slices outside the box add 0.0 there).
__global__ __launch_bounds__(CC_THREADS) void cc_level_sums_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                   int64_t cap, const uint8_t *__restrict__ sel,
                                                                   const u64 *__restrict__ off, const u32 *__restrict__ slot,
                                                                   const u64 *__restrict__ hist, int64_t hist_cap,
                                                                   const double *__restrict__ w, int nz, int K,
                                                                   u64 *__restrict__ voxels, double *__restrict__ volume,
                                                                   int64_t *__restrict__ labels, int64_t cap_sel, u64 *flags)
{
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int64_t c = t / (K + 1);
    const int level = (int)(t - c * (K + 1));
    if (c >= cap) return;
    CcSegment s;
    if (!cc_segment(table, tot, cap, sel, off, slot, hist_cap, nz, cap_sel, c, flags, s)) return;
    const u64 *m = hist + (u64)(K + 1) * s.o + level;
    u64 n = 0;
    double acc = 0.0;
    for (u64 z = s.z0; z <= s.z1; z++) {
        const u64 count = m[(u64)(K + 1) * (z - s.z0)];
        n += count;
        acc = acc + (double)count * w[z];
    }
    voxels[(int64_t)(K + 1) * s.k + level] = n;
    if (level > 0) volume[(int64_t)K * s.k + (level - 1)] = acc;
    else labels[s.k] = c + 1;
}

TOMO_API int tomo_cc_level_sums(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                                const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *w, int nz, int levels,
                                int64_t *voxels, double *volume, int64_t *labels, int64_t cap_sel, void *stream)
{
    const int64_t per = (int64_t)levels + 1;
    const bool ok = w && voxels && labels && levels >= 0 && (levels == 0 || volume);
    const int r = cc_finish_check(false, table, cap, tot, sel, off, slot, hist, hist_cap, nz, cap_sel, per, ok);
    if (r != TOMO_OK) return r;
    if (ceil_div64(cap * per, CC_THREADS) >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_level_sums_kernel, dim3((unsigned)ceil_div64(cap * per, CC_THREADS)), dim3(CC_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)table, (const u64 *)tot, cap, sel, (const u64 *)off, (const u32 *)slot,
                       (const u64 *)hist, hist_cap, w, nz, levels, (u64 *)voxels, volume, labels, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// ---------------------------------------------------------------------------------------------- caliper (Feret) diameters
// The extent of a component between two parallel planes with normal u: width = hi - lo, hi / lo the largest / smallest
// projection p of its voxels on u (centres), or of p + H / p - H with H half the width of the voxel's own box along u (voxels).
// p is a sum of three table entries (shared directions) or of three products (the component's own axes), rounded one by one
// in a fixed order, + 0.0 so that no -0.0 reaches the keys -- include/tomo_hip.h has the definition.  Every term is monotone
// in x, so a run [s, e) attains its extremes at s or at e - 1: the row pass evaluates the two ends of every run, whatever its
// length.  A float64 that is no NaN becomes a uint64 key whose unsigned order is the float order; the extremes of a thread's
// row, then of a wave whose lanes hold one component, go to hi / lo [slot[c]][m] by 64-bit atomicMax / atomicMin -- only where
// they beat what a plain load of the cell shows (the cells only rise / fall: a stale read costs an atomic, never the answer;
// one solid body would otherwise queue every wave of the volume on 2 M addresses).  Integer atomics only: the same bytes on
// every run.  Results are compacted: nothing here has a row per component of the volume.
#define CC_CAL_BATCH 8               // shared directions per workgroup row (blockIdx.y): 4 float64 per direction in registers

__device__ static inline u64 cc_f64_key(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | (1ull << 63);
}

__device__ static inline double cc_key_f64(u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k));
}

struct CcCaliperOut {
    u64 *hi, *lo;                                           // keys [cap_sel][M]
    const uint8_t *sel;
    const u32 *slot;
    u32 ncomp;
    int64_t cap_sel;
    int M, m0, nb;                                          // directions per row; the first of this batch, how many it holds
    u64 *flags;
};

// what a thread, or a wave, flushes for ONE component: the keys of D directions, the first o.nb of them real
template <int D>
struct CcCaliperKeys {
    const CcCaliperOut &o;
    u64 hi[D], lo[D];
    bool has;
    __device__ bool any() const { return has; }
    __device__ void flush(u32 c) const
    {
        if (c >= o.ncomp) return;
        const u32 k = o.slot[c];
        if ((int64_t)k >= o.cap_sel) {
            cc_flag(o.flags, CC_F_RANGE);
            return;
        }
        u64 *h = o.hi + (int64_t)k * o.M + o.m0, *l = o.lo + (int64_t)k * o.M + o.m0;
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (d >= o.nb) break;
            if (hi[d] > cc_load64(h + d)) atomicMax(h + d, hi[d]);
            if (lo[d] < cc_load64(l + d)) atomicMin(l + d, lo[d]);
        }
    }
};

// the part the two accumulators share: the extremes of D directions as float64 (no NaN, no -0.0), their keys when they leave
template <int D>
struct CcCaliperExtremes {
    CcCaliperOut o;
    double hi[D], lo[D];
    bool has;
    __device__ u32 filter(u32 c) const { return (c - 1 >= o.ncomp || !o.sel[c - 1]) ? 0u : c; }
    __device__ bool any() const { return has; }
    __device__ void reset()
    {
        has = false;
#pragma unroll
        for (int d = 0; d < D; d++) {
            hi[d] = -__builtin_inf();
            lo[d] = __builtin_inf();
        }
    }
    __device__ void widen(int d, double ps, double pe, double h)
    {
        hi[d] = fmax(hi[d], fmax(ps + h, pe + h));
        lo[d] = fmin(lo[d], fmin(ps - h, pe - h));
    }
    __device__ void flush(u32 c) const
    {
        CcCaliperKeys<D> k = {o, {}, {}, has};
#pragma unroll
        for (int d = 0; d < D; d++) {
            k.hi[d] = cc_f64_key(hi[d]);
            k.lo[d] = cc_f64_key(lo[d]);
        }
        k.flush(c);
    }
    __device__ CcCaliperKeys<D> combine(bool mine, u32) const
    {
        CcCaliperKeys<D> k = {o, {}, {}, __any(mine) != 0};
#pragma unroll
        for (int d = 0; d < D; d++) {
            k.hi[d] = wave_max64(mine ? cc_f64_key(hi[d]) : 0ull);
            k.lo[d] = wave_min64(mine ? cc_f64_key(lo[d]) : ~0ull);
        }
        return k;
    }
};

// shared directions: the row brings base = PZ[m][z] + PY[m][y] and h = H[m][z] per direction of the batch, a run adds PX[m][x]
// at its two ends.  A batch that is not full repeats its last direction (every load stays inside the tables); the flush
// leaves the repeats out.
struct CcCaliperAcc : CcCaliperExtremes<CC_CAL_BATCH> {
    const double *px;                                       // PX of the first direction of the batch
    int nx;
    double base[CC_CAL_BATCH], h[CC_CAL_BATCH];
    __device__ u32 begin(u32 c, const CcRuns &)
    {
        reset();
        return c;
    }
    __device__ void add(const CcRuns &a)
    {
        has = true;
#pragma unroll
        for (int d = 0; d < CC_CAL_BATCH; d++) {
            const double *t = px + (int64_t)(d < o.nb ? d : o.nb - 1) * nx;
            widen(d, (base[d] + t[a.s]) + 0.0, (base[d] + t[a.e - 1]) + 0.0, h[d]);
        }
    }
};

__global__ __launch_bounds__(CC_THREADS) void cc_caliper_kernel(const u64 *__restrict__ bits, int64_t nrows, int nz, int ny, int nx,
                                                                int wx, const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                int64_t cap_runs, const u32 *__restrict__ parent,
                                                                const u32 *__restrict__ rank, const uint8_t *__restrict__ sel,
                                                                const u32 *__restrict__ slot, int64_t cap,
                                                                const double *__restrict__ pz, const double *__restrict__ py,
                                                                const double *__restrict__ px, const double *__restrict__ ph, int M,
                                                                u64 *hi, u64 *lo, int64_t cap_sel, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const bool fits = cc_sel_fits(tot, cap, cap_sel, row == 0 && blockIdx.y == 0, flags);
    const bool live = row < nrows;
    const int m0 = (int)blockIdx.y * CC_CAL_BATCH, nb = M - m0 < CC_CAL_BATCH ? M - m0 : CC_CAL_BATCH;      // nb >= 1: the grid
    const int64_t z = live ? row / ny : 0, y = live ? row % ny : 0;
    CcCaliperAcc acc;
    acc.o = {hi, lo, sel, slot, fits ? (u32)cc_ncomp(tot, cap) : 0u, cap_sel, M, m0, nb, flags};
    acc.px = px + (int64_t)m0 * nx;
    acc.nx = nx;
    acc.reset();
#pragma unroll
    for (int d = 0; d < CC_CAL_BATCH; d++) {
        const int64_t m = m0 + (d < nb ? d : nb - 1);
        acc.base[d] = pz[m * nz + z] + py[m * ny + y];
        acc.h[d] = ph ? ph[m * nz + z] : 0.0;
    }
    u32 comp = 0;
    if (live) comp = cc_row_walk<true>(bits, row, nx, wx, row_off, nruns, parent, rank, flags, acc);
    cc_wave_tail<false>(comp, 0u, acc);
}

// a 2^57 cells bound keeps the byte counts of the memsets below 2^60
static int cc_caliper_args(const void *bits, int nz, int ny, int nx, const void *row_off, int64_t cap_runs, const void *parent,
                           const void *rank, const void *tot, const void *sel, const void *slot, int64_t cap, int M, const void *hi,
                           const void *lo, int64_t cap_sel, int64_t *nrows, int *wx)
{
    const int g = cc_geometry(bits, nz, ny, nx, nrows, wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !sel || !slot || !hi || !lo || hi == lo || cap_runs <= 0 || cap <= 0 || cap_sel <= 0 ||
        M <= 0)
        return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31) ||
        M > 65535 * CC_CAL_BATCH || cap_sel * M >= ((int64_t)1 << 57))
        return TOMO_E_SIZE;
    return TOMO_OK;
}

static int cc_caliper_init(u64 *hi, u64 *lo, int64_t cells, hipStream_t st)
{
    if (hipMemsetAsync(hi, 0, (size_t)cells * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;         // below every key
    if (hipMemsetAsync(lo, 0xff, (size_t)cells * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;      // above every key
    return TOMO_OK;
}

TOMO_API int tomo_cc_caliper(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                             const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *sel,
                             const uint32_t *slot, int64_t cap, const double *pz, const double *py, const double *px, const double *ph,
                             int M, uint64_t *hi, uint64_t *lo, int64_t cap_sel, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_caliper_args(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, sel, slot, cap, M, hi, lo, cap_sel, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!pz || !py || !px) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int i = cc_caliper_init((u64 *)hi, (u64 *)lo, cap_sel * M, st);
    if (i != TOMO_OK) return i;
    const dim3 grid((unsigned)ceil_div64(nrows, CC_THREADS), (unsigned)((M + CC_CAL_BATCH - 1) / CC_CAL_BATCH));
    hipLaunchKernelGGL(cc_caliper_kernel, grid, dim3(CC_THREADS), 0, st, (const u64 *)bits, nrows, nz, ny, nx, wx, (const u32 *)row_off,
                       (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank, sel, (const u32 *)slot, cap, pz, py, px, ph, M,
                       (u64 *)hi, (u64 *)lo, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// the component's own three directions: rows of axes[slot[c]] as (a_z, a_y, a_x).  There is no table per component, so the
// projection is three products, p = ((zc[z] * a_z + yt[y] * a_y) + xt[x] * a_x) + 0.0, every product and sum rounded on its
// own (-ffp-contract=off: an FMA would break the equality with a host that multiplies and adds), and
// H = 0.5 * ((|a_z| * depth[z] + |a_y| * mm_y) + |a_x| * mm_x); depth == NULL: centres, H = 0.
struct CcCaliperAxesAcc : CcCaliperExtremes<3> {
    const double *axes, *xt, *depth;
    double zc, yt, dk, mm_y, mm_x;                          // of the thread's row
    double ax[3], base[3], h[3];
    __device__ u32 begin(u32 c, const CcRuns &)
    {
        reset();
        if (c) {
            const u32 k = o.slot[c - 1];
            if ((int64_t)k >= o.cap_sel) {
                cc_flag(o.flags, CC_F_RANGE);
                return 0;
            }
            const double *a = axes + 9 * (int64_t)k;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double az = a[3 * r], ay = a[3 * r + 1];
                ax[r] = a[3 * r + 2];
                base[r] = zc * az + yt * ay;
                h[r] = depth ? 0.5 * ((fabs(az) * dk + fabs(ay) * mm_y) + fabs(ax[r]) * mm_x) : 0.0;
            }
        }
        return c;
    }
    __device__ void add(const CcRuns &a)
    {
        has = true;
        const double xs = xt[a.s], xe = xt[a.e - 1];
#pragma unroll
        for (int r = 0; r < 3; r++) widen(r, (base[r] + xs * ax[r]) + 0.0, (base[r] + xe * ax[r]) + 0.0, h[r]);
    }
};

__global__ __launch_bounds__(CC_THREADS) void cc_caliper_axes_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                     const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                     int64_t cap_runs, const u32 *__restrict__ parent,
                                                                     const u32 *__restrict__ rank, const uint8_t *__restrict__ sel,
                                                                     const u32 *__restrict__ slot, int64_t cap,
                                                                     const double *__restrict__ axes, const double *__restrict__ zc,
                                                                     const double *__restrict__ yt, const double *__restrict__ xt,
                                                                     const double *__restrict__ depth, double mm_y, double mm_x,
                                                                     u64 *hi, u64 *lo, int64_t cap_sel, u64 *flags)
{
    const int64_t row = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const u32 nruns = (u32)cc_count(tot, cap_runs);
    const bool fits = cc_sel_fits(tot, cap, cap_sel, row == 0, flags);
    const bool live = row < nrows;
    const int64_t z = live ? row / ny : 0, y = live ? row % ny : 0;
    CcCaliperAxesAcc acc;
    acc.o = {hi, lo, sel, slot, fits ? (u32)cc_ncomp(tot, cap) : 0u, cap_sel, 3, 0, 3, flags};
    acc.axes = axes;
    acc.xt = xt;
    acc.depth = depth;
    acc.zc = zc[z];
    acc.yt = yt[y];
    acc.dk = depth ? depth[z] : 0.0;
    acc.mm_y = mm_y;
    acc.mm_x = mm_x;
    acc.reset();
    u32 comp = 0;
    if (live) comp = cc_row_walk<true>(bits, row, nx, wx, row_off, nruns, parent, rank, flags, acc);
    cc_wave_tail<false>(comp, 0u, acc);
}

TOMO_API int tomo_cc_caliper_axes(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                  const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *sel,
                                  const uint32_t *slot, int64_t cap, const double *axes, const double *zc, const double *yt,
                                  const double *xt, const double *depth, double mm_y, double mm_x, uint64_t *hi, uint64_t *lo,
                                  int64_t cap_sel, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_caliper_args(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, sel, slot, cap, 3, hi, lo, cap_sel, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!axes || !zc || !yt || !xt) return TOMO_E_ARG;
    if (depth && (!(mm_y > 0.0 && mm_y < __builtin_inf()) || !(mm_x > 0.0 && mm_x < __builtin_inf()))) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int i = cc_caliper_init((u64 *)hi, (u64 *)lo, cap_sel * 3, st);
    if (i != TOMO_OK) return i;
    hipLaunchKernelGGL(cc_caliper_axes_kernel, dim3((unsigned)ceil_div64(nrows, CC_THREADS)), dim3(CC_THREADS), 0, st, (const u64 *)bits,
                       nrows, ny, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent, (const u32 *)rank, sel,
                       (const u32 *)slot, cap, axes, zc, yt, xt, depth, mm_y, mm_x, (u64 *)hi, (u64 *)lo, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}

// One thread per component; a selected one decodes its M keys IN PLACE (hi / lo hold float64 afterwards), writes width = hi - lo
// and finds the largest and the smallest width, the lowest direction index among equals.  rows[slot[c]] = (c + 1, voxels, index
// of the largest width, index of the smallest), ext[slot[c]] = (largest width, smallest width).  A cell no voxel reached (the
// bits changed since the selection) is CC_F_RANGE.
__global__ __launch_bounds__(CC_THREADS) void cc_caliper_rows_kernel(const u64 *__restrict__ table, const u64 *__restrict__ tot,
                                                                     int64_t cap, const uint8_t *__restrict__ sel,
                                                                     const u32 *__restrict__ slot, u64 *hi, u64 *lo, int M,
                                                                     double *__restrict__ width, int64_t *__restrict__ rows,
                                                                     double *__restrict__ ext, int64_t cap_sel, u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    u32 k;
    if (!cc_selected(tot, cap, sel, slot, cap_sel, c, flags, k)) return;
    u64 *h = hi + (int64_t)k * M, *l = lo + (int64_t)k * M;
    double *w = width + (int64_t)k * M;
    double wmax = 0.0, wmin = 0.0;
    int imax = 0, imin = 0;
    bool reached = true;
    for (int m = 0; m < M; m++) {
        const u64 kh = h[m], kl = l[m];
        if (kh == 0ull || kl == ~0ull) reached = false;
        const double a = cc_key_f64(kh), b = cc_key_f64(kl), d = a - b;
        ((double *)h)[m] = a;
        ((double *)l)[m] = b;
        w[m] = d;
        if (m == 0 || d > wmax) { wmax = d; imax = m; }
        if (m == 0 || d < wmin) { wmin = d; imin = m; }
    }
    if (!reached) cc_flag(flags, CC_F_RANGE);
    rows[4 * (int64_t)k] = c + 1;
    rows[4 * (int64_t)k + 1] = (int64_t)table[c * CC_COLS];
    rows[4 * (int64_t)k + 2] = imax;
    rows[4 * (int64_t)k + 3] = imin;
    ext[2 * (int64_t)k] = wmax;
    ext[2 * (int64_t)k + 1] = wmin;
}

TOMO_API int tomo_cc_caliper_rows(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                                  uint64_t *hi, uint64_t *lo, int M, double *width, int64_t *rows, double *ext, int64_t cap_sel,
                                  void *stream)
{
    if (!table || !tot || !sel || !slot || !hi || !lo || hi == lo || !width || !rows || !ext || cap <= 0 || cap_sel <= 0 || M <= 0)
        return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31) || M > 65535 * CC_CAL_BATCH || cap_sel * M >= ((int64_t)1 << 57))
        return TOMO_E_SIZE;
    hipLaunchKernelGGL(cc_caliper_rows_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u64 *)tot, cap, sel, (const u32 *)slot, (u64 *)hi, (u64 *)lo, M, width, rows, ext,
                       cap_sel, (u64 *)tot + 2);
    return tomo_status();
}
