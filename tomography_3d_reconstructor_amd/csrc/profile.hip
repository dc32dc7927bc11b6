// profile.hip -- what a float32 map gives per component of a labelled volume beyond its maximum (no counterpart in the
// reference): the smallest and the largest value, the first voxel that attains each, and a fixed-point sum for the mean.  Made
// for the radius along the branches of a skeleton -- the tables of the regular voxels, the distance map of the object --, it
// serves any run tables.  Definition and contract: include/tomo_hip.h.
//
// All three passes are the WORD PASS of cc_runs.h: a wave is a word, a lane a bit, the runs of the word and their components are
// wave-uniform.  A skeleton word holds one to three bits, so most of a wave idles in the reductions; what the pass pays for is
// the words it looks at, and a word without a set bit leaves before the map is touched.
// Min and max travel as float32 bit patterns (admitted values are >= +0.0: unsigned order is float order), the sum as int64 of
// q(v) = rint(v * 2^16): the product is exact in float64, the rounding is half to even, and integer adds commute -- the same
// bytes on every run.  A minimum or maximum is sent only where it beats what a plain load shows (cc_value_kernel's discipline:
// lo only falls, hi only rises, so a stale read costs an atomic, never the answer).
#include "cc_runs.h"

#define PROFILE_ADMITTED 0x49800000u                 // float32 bit patterns below it: 0.0 <= v < 2^20, finite, not -0.0
#define PROFILE_F_VALUE 8ull                         // bit of tot[2]: a set voxel with a value outside that window
#define PROFILE_COLS 7                               // columns of a row of tomo_profile_rows

// the float32 bits of the lane's voxel and whether they are admitted; an unset voxel reads nothing
__device__ static inline bool profile_value(const CcWordAt &a, const float *__restrict__ values, int64_t at, u32 &v)
{
    const bool set = (a.cur >> a.bit) & 1;
    v = set ? __float_as_uint(values[at]) : 0u;            // a set bit lies below nx: inside the array
    return set && v < PROFILE_ADMITTED;
}

__global__ __launch_bounds__(CC_THREADS) void profile_stats_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                                   const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                   int64_t cap_runs, const u32 *__restrict__ parent,
                                                                   const u32 *__restrict__ rank, const float *__restrict__ values,
                                                                   u32 *lo, u32 *hi, unsigned long long *sum, int64_t cap, u64 *flags)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    CcWordAt a;
    if (!cc_word_at(bits, nwords, nx, wx, row_off, a)) return;
    const u32 nruns = (u32)cc_count(tot, cap_runs), ncomp = (u32)cc_ncomp(tot, cap);
    const int64_t at = a.row * nx + 64 * a.wj + a.bit;
    u32 v;
    const bool ok = profile_value(a, values, at, v);
    if (__ballot(((a.cur >> a.bit) & 1) && !ok) && a.bit == 0) cc_flag(flags, PROFILE_F_VALUE);
    const u64 q = ok ? (u64)(int64_t)rint((double)__uint_as_float(v) * 65536.0) : 0ull;
    while (cc_word_runs_next(a.it)) {                       // wave-uniform
        if (a.it.run >= nruns) {
            if (a.bit == 0) cc_flag(flags, CC_F_RANGE);
            continue;
        }
        const u32 c = cc_component(parent, rank, a.it.run);
        if (c >= ncomp) continue;                           // more components than the tables hold: CC_F_CAP, above
        const bool mine = ((a.it.mask >> a.bit) & 1) && ok;
        if (!__ballot(mine)) continue;                      // a run of inadmissible values only
        const u32 least = wave_min32(mine ? v : ~0u), most = wave_max32(mine ? v : 0u);
        const u64 s = wave_sum64(mine ? q : 0ull);
        if (a.bit == 0) {
            if (least < cc_load(lo + c)) atomicMin(lo + c, least);
            if (most > cc_load(hi + c)) atomicMax(hi + c, most);
            if (s) atomicAdd(sum + c, (unsigned long long)s);
        }
    }
}

// lo_first[c] / hi_first[c] = the smallest flat index whose value has the bits lo[c] / hi[c]: cc_value_kernel<true> on both sides.
// Only the runs that attain an extreme send, and of those only the ones below what the array already shows.
__global__ __launch_bounds__(CC_THREADS) void profile_where_kernel(const u64 *__restrict__ bits, int64_t nwords, int nx, int wx,
                                                                   const u32 *__restrict__ row_off, const u64 *__restrict__ tot,
                                                                   int64_t cap_runs, const u32 *__restrict__ parent,
                                                                   const u32 *__restrict__ rank, const float *__restrict__ values,
                                                                   const u32 *__restrict__ lo, const u32 *__restrict__ hi,
                                                                   unsigned long long *lo_first, unsigned long long *hi_first,
                                                                   int64_t cap, u64 *flags)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && tot[1] > (u64)cap) cc_flag(flags, CC_F_CAP);
    CcWordAt a;
    if (!cc_word_at(bits, nwords, nx, wx, row_off, a)) return;
    const u32 nruns = (u32)cc_count(tot, cap_runs), ncomp = (u32)cc_ncomp(tot, cap);
    const int64_t at = a.row * nx + 64 * a.wj + a.bit;
    u32 v;
    const bool ok = profile_value(a, values, at, v);
    while (cc_word_runs_next(a.it)) {                       // wave-uniform
        if (a.it.run >= nruns) {
            if (a.bit == 0) cc_flag(flags, CC_F_RANGE);
            continue;
        }
        const u32 c = cc_component(parent, rank, a.it.run);
        if (c >= ncomp) continue;
        const bool mine = ((a.it.mask >> a.bit) & 1) && ok;
        const u64 low = __ballot(mine && v == lo[c]), high = __ballot(mine && v == hi[c]);
        if (a.bit == 0 && low) {                            // at is the flat index of the word's bit 0 here
            const u64 cand = (u64)(at + (__ffsll((long long)low) - 1));
            if (cand < cc_load64((const u64 *)lo_first + c)) atomicMin(lo_first + c, (unsigned long long)cand);
        }
        if (a.bit == 0 && high) {
            const u64 cand = (u64)(at + (__ffsll((long long)high) - 1));
            if (cand < cc_load64((const u64 *)hi_first + c)) atomicMin(hi_first + c, (unsigned long long)cand);
        }
    }
}

// two arrays of the call are one, or one of them lies over the bits or the map
static bool profile_aliased(const void *bits, const void *values, const void *const *arrays, int n)
{
    for (int i = 0; i < n; i++) {
        if (arrays[i] == bits || arrays[i] == values) return true;
        for (int j = 0; j < i; j++)
            if (arrays[i] == arrays[j]) return true;
    }
    return false;
}

// the checks both passes share -> the words of the volume in *nwords
static int profile_args(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                        const uint32_t *rank, const unsigned long long *tot, const float *values, const void *const *arrays, int n,
                        int64_t cap, int64_t *nwords, int *wx)
{
    int64_t nrows;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, wx);
    if (g != TOMO_OK) return g;
    if (!row_off || !parent || !rank || !tot || !values || cap_runs <= 0 || cap <= 0) return TOMO_E_ARG;
    for (int i = 0; i < n; i++)
        if (!arrays[i]) return TOMO_E_ARG;
    if (profile_aliased(bits, values, arrays, n)) return TOMO_E_ARG;
    if (cap_runs >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    *nwords = nrows * *wx;                                  // < 2^31 (cc_geometry): the grids have fewer than 2^29 workgroups
    return TOMO_OK;
}

TOMO_API int tomo_profile_stats(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *values,
                                uint32_t *lo, uint32_t *hi, int64_t *sum, int64_t cap, void *stream)
{
    const void *const arrays[3] = {lo, hi, sum};
    int64_t nwords;
    int wx;
    const int r = profile_args(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, values, arrays, 3, cap, &nwords, &wx);
    if (r != TOMO_OK) return r;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(lo, 0xff, (size_t)cap * sizeof(u32), st) != hipSuccess || hipMemsetAsync(hi, 0, (size_t)cap * sizeof(u32), st) != hipSuccess ||
        hipMemsetAsync(sum, 0, (size_t)cap * sizeof(int64_t), st) != hipSuccess)
        return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(profile_stats_kernel, dim3((unsigned)ceil_div64(nwords * 64, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, values, (u32 *)lo, (u32 *)hi, (unsigned long long *)sum, cap, (u64 *)tot + 2);
    return tomo_status();
}

TOMO_API int tomo_profile_where(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *values,
                                const uint32_t *lo, const uint32_t *hi, uint64_t *lo_first, uint64_t *hi_first, int64_t cap, void *stream)
{
    const void *const arrays[4] = {lo, hi, lo_first, hi_first};
    int64_t nwords;
    int wx;
    const int r = profile_args(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, values, arrays, 4, cap, &nwords, &wx);
    if (r != TOMO_OK) return r;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(lo_first, 0xff, (size_t)cap * sizeof(u64), st) != hipSuccess ||
        hipMemsetAsync(hi_first, 0xff, (size_t)cap * sizeof(u64), st) != hipSuccess)
        return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(profile_where_kernel, dim3((unsigned)ceil_div64(nwords * 64, CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const u64 *)bits, nwords, nx, wx, (const u32 *)row_off, (const u64 *)tot, cap_runs, (const u32 *)parent,
                       (const u32 *)rank, values, (const u32 *)lo, (const u32 *)hi, (unsigned long long *)lo_first,
                       (unsigned long long *)hi_first, cap, (u64 *)tot + 2);
    return tomo_status();
}

// out[slot[c]] = (c + 1, voxels, lo[c], hi[c], sum[c], lo_first[c], hi_first[c]) for every selected component c: cc_value_rows_kernel
__global__ __launch_bounds__(CC_THREADS) void profile_rows_kernel(const u64 *__restrict__ table, const u32 *__restrict__ lo,
                                                                  const u32 *__restrict__ hi, const u64 *__restrict__ sum,
                                                                  const u64 *__restrict__ lo_first, const u64 *__restrict__ hi_first,
                                                                  const u64 *__restrict__ tot, int64_t cap, const uint8_t *__restrict__ sel,
                                                                  const u32 *__restrict__ slot, u64 *__restrict__ out, int64_t cap_sel,
                                                                  u64 *flags)
{
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const bool fits = tot[5] <= (u64)cap_sel && tot[1] <= (u64)cap;
    if (c == 0 && !fits) cc_flag(flags, CC_F_CAP);
    if (!fits || c >= cc_ncomp(tot, cap) || !sel[c]) return;
    const u32 k = slot[c];
    if ((int64_t)k >= cap_sel) {
        cc_flag(flags, CC_F_RANGE);
        return;
    }
    u64 *o = out + PROFILE_COLS * (int64_t)k;
    o[0] = (u64)c + 1;
    o[1] = table[c * CC_COLS];
    o[2] = lo[c];
    o[3] = hi[c];
    o[4] = sum[c];
    o[5] = lo_first[c];
    o[6] = hi_first[c];
}

TOMO_API int tomo_profile_rows(const int64_t *table, const uint32_t *lo, const uint32_t *hi, const int64_t *sum, const uint64_t *lo_first,
                               const uint64_t *hi_first, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                               int64_t *out, int64_t cap_sel, void *stream)
{
    const void *const arrays[6] = {lo, hi, sum, lo_first, hi_first, out};
    if (!table || !tot || !sel || !slot || cap <= 0 || cap_sel <= 0) return TOMO_E_ARG;
    for (int i = 0; i < 6; i++)
        if (!arrays[i]) return TOMO_E_ARG;
    if (profile_aliased(table, nullptr, arrays, 6)) return TOMO_E_ARG;
    if (cap >= ((int64_t)1 << 31) || cap_sel >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(profile_rows_kernel, dim3((unsigned)ceil_div64(cap, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream,
                       (const u64 *)table, (const u32 *)lo, (const u32 *)hi, (const u64 *)sum, (const u64 *)lo_first,
                       (const u64 *)hi_first, (const u64 *)tot, cap, sel, (const u32 *)slot, (u64 *)out, cap_sel, (u64 *)tot + 2);
    return tomo_status();
}
