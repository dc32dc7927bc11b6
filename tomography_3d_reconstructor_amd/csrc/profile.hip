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
// bytes on every run.  A minimum or maximum is sent only where it beats what a plain load shows (CcValuePass's discipline:
// lo only falls, hi only rises, so a stale read costs an atomic, never the answer).
#include "cc_runs.h"

#define PROFILE_ADMITTED 0x49800000u                 // float32 bit patterns below it: 0.0 <= v < 2^20, finite, not -0.0
#define PROFILE_F_VALUE 8ull                         // bit of tot[2]: a set voxel with a value outside that window
#define PROFILE_COLS 7                               // columns of a row of tomo_profile_rows

// every array of the call is given, no two of them are one, and none lies over the bits (the table) or the map
static bool profile_arrays(const void *bits, const void *values, std::initializer_list<const void *> arrays)
{
    for (const void *const *x = arrays.begin(); x != arrays.end(); x++) {
        if (!*x || *x == bits || *x == values) return false;
        for (const void *const *y = arrays.begin(); y != x; y++)
            if (*x == *y) return false;
    }
    return true;
}

// what both passes share: the float32 bits of the lane's voxel and whether they are admitted; an unset voxel reads nothing
struct ProfilePass {
    struct Value {
        u32 v;
        bool ok;
    };
    static constexpr bool SELECTED = false;
    const float *__restrict__ values;
    __device__ bool fits(const u64 *) const { return true; }
    __device__ Value value(bool set, int64_t at) const
    {
        const u32 v = set ? __float_as_uint(values[at]) : 0u;
        return {v, set && v < PROFILE_ADMITTED};
    }
};

// lo[c], hi[c], sum[c] over the admitted values of component c + 1.  A set voxel whose value is not admitted raises
// PROFILE_F_VALUE before the run loop and counts nowhere; a run that holds only such values is skipped.
struct ProfileStats : ProfilePass {
    struct Lane : Value {
        u64 q;                                              // q(v), 0 for a voxel that does not count
    };
    u32 *lo, *hi;
    unsigned long long *sum;
    __device__ Lane load(const CcWordArgs &a, const u64 *, const CcWordAt &w, bool set, int64_t at) const
    {
        const Value x = value(set, at);
        if (__ballot(set && !x.ok) && w.bit == 0) cc_flag(a.flags, PROFILE_F_VALUE);
        return {x, x.ok ? (u64)(int64_t)rint((double)__uint_as_float(x.v) * 65536.0) : 0ull};
    }
    __device__ void run(const CcWordArgs &, const CcWordAt &w, u32 c, bool mine, const Lane &l, int64_t) const
    {
        mine = mine && l.ok;
        if (!__ballot(mine)) return;                        // a run of inadmissible values only
        const u32 least = wave_min32(mine ? l.v : ~0u), most = wave_max32(mine ? l.v : 0u);
        const u64 s = wave_sum64(mine ? l.q : 0ull);
        if (w.bit == 0) {
            if (least < cc_load(lo + c)) atomicMin(lo + c, least);
            if (most > cc_load(hi + c)) atomicMax(hi + c, most);
            if (s) atomicAdd(sum + c, (unsigned long long)s);
        }
    }
    bool ok(const void *bits) const { return values && profile_arrays(bits, values, {lo, hi, sum}); }
    std::array<CcClear, 3> clears(int64_t cap) const
    {
        return {CcClear{lo, 0xff, (size_t)cap * sizeof(u32)}, {hi, 0, (size_t)cap * sizeof(u32)}, {sum, 0, (size_t)cap * sizeof(int64_t)}};
    }
};

// lo_first[c] / hi_first[c] = the smallest flat index whose value has the bits lo[c] / hi[c]: CcValuePass<true> on both sides.
// Only the runs that attain an extreme send, and of those only the ones below what the array already shows.
struct ProfileWhere : ProfilePass {
    using Lane = Value;
    const u32 *__restrict__ lo, *__restrict__ hi;
    unsigned long long *lo_first, *hi_first;
    __device__ Lane load(const CcWordArgs &, const u64 *, const CcWordAt &, bool set, int64_t at) const { return value(set, at); }
    __device__ void run(const CcWordArgs &, const CcWordAt &w, u32 c, bool mine, const Lane &l, int64_t at) const
    {
        mine = mine && l.ok;
        const u64 low = __ballot(mine && l.v == lo[c]), high = __ballot(mine && l.v == hi[c]);
        if (w.bit == 0 && low) {                            // at is the flat index of the word's bit 0 here
            const u64 cand = (u64)(at + (__ffsll((long long)low) - 1));
            if (cand < cc_load64((const u64 *)lo_first + c)) atomicMin(lo_first + c, (unsigned long long)cand);
        }
        if (w.bit == 0 && high) {
            const u64 cand = (u64)(at + (__ffsll((long long)high) - 1));
            if (cand < cc_load64((const u64 *)hi_first + c)) atomicMin(hi_first + c, (unsigned long long)cand);
        }
    }
    bool ok(const void *bits) const { return values && profile_arrays(bits, values, {lo, hi, lo_first, hi_first}); }
    std::array<CcClear, 2> clears(int64_t cap) const
    {
        return {CcClear{lo_first, 0xff, (size_t)cap * sizeof(u64)}, {hi_first, 0xff, (size_t)cap * sizeof(u64)}};
    }
};

TOMO_API int tomo_profile_stats(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *values,
                                uint32_t *lo, uint32_t *hi, int64_t *sum, int64_t cap, void *stream)
{
    const ProfileStats p = {{values}, (u32 *)lo, (u32 *)hi, (unsigned long long *)sum};
    return cc_word_launch(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

TOMO_API int tomo_profile_where(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                                const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *values,
                                const uint32_t *lo, const uint32_t *hi, uint64_t *lo_first, uint64_t *hi_first, int64_t cap, void *stream)
{
    const ProfileWhere p = {{values}, (const u32 *)lo, (const u32 *)hi, (unsigned long long *)lo_first, (unsigned long long *)hi_first};
    return cc_word_launch(bits, nz, ny, nx, row_off, cap_runs, parent, rank, tot, cap, p, stream);
}

// out[slot[c]] = (c + 1, voxels, lo[c], hi[c], sum[c], lo_first[c], hi_first[c]) for every selected component c
struct ProfileRow {
    static constexpr int COLS = PROFILE_COLS;
    const u64 *__restrict__ table;
    const u32 *__restrict__ lo, *__restrict__ hi;
    const u64 *__restrict__ sum, *__restrict__ lo_first, *__restrict__ hi_first;
    __device__ void write(u64 *__restrict__ o, int64_t c) const
    {
        o[0] = (u64)c + 1;
        o[1] = table[c * CC_COLS];
        o[2] = lo[c];
        o[3] = hi[c];
        o[4] = sum[c];
        o[5] = lo_first[c];
        o[6] = hi_first[c];
    }
};

TOMO_API int tomo_profile_rows(const int64_t *table, const uint32_t *lo, const uint32_t *hi, const int64_t *sum, const uint64_t *lo_first,
                               const uint64_t *hi_first, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                               int64_t *out, int64_t cap_sel, void *stream)
{
    const ProfileRow w = {(const u64 *)table, (const u32 *)lo, (const u32 *)hi, (const u64 *)sum, (const u64 *)lo_first, (const u64 *)hi_first};
    const bool ok = table && profile_arrays(table, nullptr, {lo, hi, sum, lo_first, hi_first, out});
    return cc_rows_launch(w, ok, cap, tot, sel, slot, out, cap_sel, stream);
}
