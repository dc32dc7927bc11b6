// contacts.hip -- the contact table between zones (no counterpart in the reference): per unordered pair of zone labels the number
// of 26-adjacent voxel pairs across their interface, per slice and direction class, with the Crofton area, the throat and the
// shortest way across.  The definition is in include/tomo_hip.h.  This is the project's first KEYED accumulation: a row is named
// by a pair of arbitrary int32 labels, and nobody knows in advance which pairs exist or how many.
//
// Three walks over the volume come from ONE templated device function (ct_walk), so that count, insert and hist cannot disagree
// about what a contact pair is:
//   count   N = the contact pairs, one integer atomic per wave at most; the host sizes the hash table from it
//   insert  an open-addressed table of 64-bit keys (a << 32 | b, never 0), claimed by one compare-and-swap per probe; per slot the
//           pairs, the slice range, the first index, the largest value and the shortest way, all by relaxed integer atomics
//   hist    lookup only; counts per (row, slice, class) into the segments the host laid out, and the index of the largest value
// and tomo_contact_finish sums every row's segment in ascending slice and class in sequential float64, one thread per row.
//
// The walk.  A wave is one 64-voxel word column of one slice, a lane one x; the wave walks CT_ROWS rows in ascending y.  It loads
// the bit words of its rows in both slices once, up front (lane j holds row j), so that no label load waits for a bit load.  Per
// row it loads ONE row of the slice and ONE of the slice above (two coalesced 256-byte loads of the map, plus the two voxels
// beside the word), requested CT_AHEAD rows before they are used: the walk is bound by latency, not by bytes (0.64 -> 0.43 ms for
// the count pass at 512^3, profiles/r33_contacts.md).  The other neighbour rows are the registers of the previous step, and
// x - 1 / x + 1 come from the neighbouring lanes
// (DPP).  A value in those registers is the label where the voxel takes part (set, entry > 0) and 0 elsewhere, so a voxel outside
// the stack, beyond the row's end or in another row's end is simply 0.  Nearly every wave sees no unlike neighbour and leaves a
// row after thirteen compares and one ballot.  Where a wave has contacts they share one or two keys: equal keys are combined in
// the wave (the first active lane's key, a ballot of the lanes that hold it, a popcount), and the wave keeps ONE open accumulator
// -- key, slot and sums -- across directions and rows, flushed when the key changes and at the end.  Nothing waits on another
// thread: a probe is bounded by the capacity, a lane that finds no slot counts itself into an overflow counter.
// Every sum is an integer sum, every extreme an integer min / max: the bytes do not depend on the schedule.
#include "tomo_common.h"

#define CT_THREADS 256
#define CT_ROWS 16                                  // rows of one word column a wave walks
#define CT_CLASSES 7
#define CT_FCOLS 11                                 // columns of surface_factors' table; class c reads column c
#define CT_OUT 17                                   // int64 words per row of tomo_contact_finish
#define CT_NONE 0xFFFFFFFFFFFFFFFFull

struct CtGrid {
    int64_t wx, words, chunks, items;
};

static int ct_grid(int nz, int ny, int nx, CtGrid *g)
{
    if (nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    g->wx = tomo_words_per_row(nx);
    g->words = (int64_t)nz * ny * g->wx;
    if (g->words >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    g->chunks = ((int64_t)ny + CT_ROWS - 1) / CT_ROWS;
    g->items = (int64_t)nz * g->chunks * g->wx;      // <= words
    return TOMO_OK;
}

static bool ct_distinct(const void *const *p, int n)
{
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (p[i] && p[i] == p[j]) return false;
    return true;
}

static bool ct_capacity(int64_t cap, int *r)
{
    if (cap <= 0 || (cap & (cap - 1))) { *r = TOMO_E_ARG; return false; }
    if (cap > ((int64_t)1 << 30)) { *r = TOMO_E_SIZE; return false; }
    return true;
}

// the thirteen forward directions in the order of the registers below: (dz, dy, dx) and the class x, y, xy, z, xz, yz, xyz
__device__ static constexpr int CT_DZ[13] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1};
__device__ static constexpr int CT_DY[13] = {0, 1, 1, 1, -1, -1, -1, 0, 0, 0, 1, 1, 1};
__device__ static constexpr int CT_DX[13] = {1, -1, 0, 1, -1, 0, 1, -1, 0, 1, -1, 0, 1};
__device__ static constexpr int CT_CLASS[13] = {0, 2, 1, 2, 6, 5, 6, 4, 3, 4, 6, 5, 6};

struct CtRow {
    int l, m, r;                                     // the labels at x - 1, x, x + 1; 0 where the voxel takes no part
};

// What a wave knows of the bits before it loads a label: lane j holds row y0 - 1 + j of its word column, for the slice (a) and the
// slice above (b): the word itself and, in e, bit 0 = the voxel left of the word is set, bit 1 = the voxel right of it is set.
// Six loads per lane, all in flight together; rows and words outside the stack read as clear.
struct CtBits {
    u64 wa, wb;
    u32 ea, eb;
};

// the labels of one row pair as loaded: at x (m) and, in lanes 0 and 63, beside the word (e)
struct CtRaw {
    int ma, ea, mb, eb;
};

__device__ static inline void ct_bits_row(const u64 *__restrict__ row, int w, int wx, u64 &word, u32 &e)
{
    word = row[w];
    if (w > 0) e |= (u32)(row[w - 1] >> 63);
    if (w + 1 < wx) e |= (u32)(row[w + 1] & 1) << 1;                     // 64 (w + 1) < nx: no tail bit is read
}

__device__ static inline u64 ct_lane64(u64 v, int j)                       // j is the same in every lane
{
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, j), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), j);
    return ((u64)hi << 32) | lo;
}

__device__ static inline void ct_fetch_row(const int *__restrict__ zone, u64 word, u32 e, int x, int b, int nx, int &m, int &edge)
{
    m = 0, edge = 0;
    if (x < nx && ((word >> b) & 1)) m = zone[x];                        // x < nx: no tail bit decides
    if (b == 0 && (e & 1)) edge = zone[x - 1];                            // lane 0 fetches the voxel left of the word,
    if (b == 63 && (e & 2)) edge = zone[x + 1];                           // lane 63 the one right of it
    m = m > 0 ? m : 0;
    edge = edge > 0 ? edge : 0;
}

// rows y of the slice and of the slice above; `wanted` is the same for the whole wave
__device__ static inline CtRaw ct_fetch(const int *__restrict__ zone, const CtBits &k, bool wanted, int y, int y0, int64_t r0, int64_t r1,
                                        int x, int b, int nx)
{
    CtRaw q = {0, 0, 0, 0};
    if (wanted) {
        const int j = __builtin_amdgcn_readfirstlane(y - y0 + 1);
        ct_fetch_row(zone + (r0 + y) * nx, ct_lane64(k.wa, j), (u32)__builtin_amdgcn_readlane((int)k.ea, j), x, b, nx, q.ma, q.ea);
        ct_fetch_row(zone + (r1 + y) * nx, ct_lane64(k.wb, j), (u32)__builtin_amdgcn_readlane((int)k.eb, j), x, b, nx, q.mb, q.eb);
    }
    return q;
}

// the lane exchange runs with every lane active
__device__ static inline CtRow ct_spread(int m, int edge)
{
    CtRow r;
    r.m = m;
    r.l = dpp_from_prev(m, edge);
    r.r = dpp_from_next(m, edge);
    return r;
}

// One work item: slice z, rows [y0, y1), word w.  op.at(z, y, x, own, nb, hit) is called with every lane active whenever some
// lane of the wave has a contact pair; hit has bit d set where (own, nb[d]) is one.  The labels of a row pair are requested
// CT_AHEAD rows before they are used, so that a wave has several rows in flight instead of waiting for each in turn.
#define CT_AHEAD 3
template <class Op>
__device__ static inline void ct_walk(const u64 *__restrict__ bits, const int *__restrict__ zone, int nz, int ny, int nx, int wx,
                                      int chunks, int64_t item, Op &op)
{
    const int b = threadIdx.x & 63;
    const int w = (int)(item % wx);
    const int64_t t = item / wx;
    const int z = (int)(t / chunks);
    const int y0 = (int)(t % chunks) * CT_ROWS;
    const int y1 = y0 + CT_ROWS < ny ? y0 + CT_ROWS : ny;
    const int x = 64 * w + b;
    const bool up = z + 1 < nz;
    const int64_t r0 = (int64_t)z * ny, r1 = r0 + ny;
    CtBits k = {0, 0, 0, 0};
    {
        const int ry = y0 - 1 + b;                                         // lanes 0 .. CT_ROWS + 1: rows y0 - 1 .. y0 + CT_ROWS
        if (b < CT_ROWS + 2 && ry >= 0 && ry < ny) {
            ct_bits_row(bits + (r0 + ry) * wx, w, wx, k.wa, k.ea);
            if (up) ct_bits_row(bits + (r1 + ry) * wx, w, wx, k.wb, k.eb);
        }
    }
    // a row past y1 is never used, a row outside the slice has clear bits: both read as 0 without a load
    const int last = y1 < ny ? y1 : ny - 1;
    CtRaw first = ct_fetch(zone, k, true, y0, y0, r0, r1, x, b, nx);
    CtRaw below = ct_fetch(zone, k, y0 > 0, y0 - 1, y0, r0, r1, x, b, nx);
    CtRaw q[CT_AHEAD];
#pragma unroll
    for (int i = 0; i < CT_AHEAD; i++) q[i] = ct_fetch(zone, k, y0 + 1 + i <= last, y0 + 1 + i, y0, r0, r1, x, b, nx);
    CtRow a0 = ct_spread(first.ma, first.ea), b0 = ct_spread(first.mb, first.eb), bm = ct_spread(below.mb, below.eb);
    for (int y = y0; y < y1; y++) {
        const CtRaw ahead = ct_fetch(zone, k, y + 1 + CT_AHEAD <= last, y + 1 + CT_AHEAD, y0, r0, r1, x, b, nx);
        const CtRow a1 = ct_spread(q[0].ma, q[0].ea), b1 = ct_spread(q[0].mb, q[0].eb);
        const int own = a0.m;
        const int nb[13] = {a0.r, a1.l, a1.m, a1.r, bm.l, bm.m, bm.r, b0.l, b0.m, b0.r, b1.l, b1.m, b1.r};
        u32 hit = 0;
#pragma unroll
        for (int d = 0; d < 13; d++) hit |= (u32)(own > 0 && nb[d] > 0 && nb[d] != own) << d;
        if (__ballot(hit != 0)) op.at(z, y, x, own, nb, hit);
        a0 = a1;
        bm = b0;
        b0 = b1;
#pragma unroll
        for (int i = 0; i + 1 < CT_AHEAD; i++) q[i] = q[i + 1];
        q[CT_AHEAD - 1] = ahead;
    }
}

__device__ static inline u64 ct_key(int p, int q)
{
    const u32 a = (u32)(p < q ? p : q), c = (u32)(p < q ? q : p);
    return ((u64)a << 32) | c;
}

__device__ static inline u64 ct_hash(u64 h)
{
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

// float32 -> a u32 that orders as the floats do (NaN-free input); -0.0 is taken as +0.0
__device__ static inline u32 ct_value_key(float v)
{
    const u32 u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ static inline u32 ct_value_bits(u32 k)
{
    return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
}

// the slot of `key`, claimed when absent; -1 when the table has no room.  At most `cap` probes, no waiting.
__device__ static inline int64_t ct_claim(u64 *keys, int64_t cap, u64 key)
{
    u64 h = ct_hash(key) & (u64)(cap - 1);
    for (int64_t i = 0; i < cap; i++) {
        u64 cur = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS((unsigned long long *)(keys + h), 0ull, (unsigned long long)key);
            if (cur == 0) return (int64_t)h;
        }
        if (cur == key) return (int64_t)h;
        h = (h + 1) & (u64)(cap - 1);
    }
    return -1;
}

// the slot of `key` in the finished table; -1 when it is not there
__device__ static inline int64_t ct_find(const u64 *__restrict__ keys, int64_t cap, u64 key)
{
    u64 h = ct_hash(key) & (u64)(cap - 1);
    for (int64_t i = 0; i < cap; i++) {
        const u64 cur = keys[h];
        if (cur == key) return (int64_t)h;
        if (cur == 0) return -1;
        h = (h + 1) & (u64)(cap - 1);
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------- count
struct CtCount {
    u64 n;
    __device__ inline void at(int, int, int, int, const int *, u32 hit) { n += (u64)__popc(hit); }
};

__global__ __launch_bounds__(CT_THREADS) void contact_count_kernel(const u64 *__restrict__ bits, const int *__restrict__ zone, int nz, int ny,
                                                                   int nx, int wx, int chunks, int64_t items, unsigned long long *counter)
{
    const int64_t item = ((int64_t)blockIdx.x * CT_THREADS + threadIdx.x) >> 6;      // the same for the 64 lanes of a wave
    if (item >= items) return;
    CtCount op = {0};
    ct_walk(bits, zone, nz, ny, nx, wx, chunks, item, op);
    const u64 n = wave_sum64(op.n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (unsigned long long)n);
}

// ---------------------------------------------------------------------------------------------- insert
struct CtInsert {
    const float *__restrict__ values, *__restrict__ dist, *__restrict__ wxy, *__restrict__ wz;
    u64 *keys;
    int64_t cap;
    unsigned long long *pairs, *first, *counters;
    u32 *z_lo, *value_max, *path;
    int *z_hi;
    int ny, nx, lane, z;
    // the open accumulator, the same in every lane
    u64 key, n, lowest;
    int64_t slot;
    u32 vmax, pmin;

    __device__ inline void flush()
    {
        if (key && lane == 0) {
            if (slot < 0)
                atomicAdd(counters, (unsigned long long)n);                        // no room: the contribution is dropped and counted
            else {
                atomicAdd(pairs + slot, (unsigned long long)n);
                atomicMin(z_lo + slot, (u32)z);
                atomicMax(z_hi + slot, z);
                atomicMin(first + slot, (unsigned long long)lowest);
                if (values) atomicMax(value_max + slot, vmax);
                if (dist) atomicMin(path + slot, pmin);
            }
        }
        key = 0;
    }

    __device__ inline void at(int zz, int y, int x, int own, const int *nb, u32 hit)
    {
        z = zz;
        const int64_t p = ((int64_t)zz * ny + y) * nx + x;
#pragma unroll
        for (int d = 0; d < 13; d++) {
            const bool act = (hit >> d) & 1;
            u64 rem = __ballot(act);
            if (!rem) continue;
            const u64 k = act ? ct_key(own, nb[d]) : 0;
            const int64_t q = p + ((int64_t)CT_DZ[d] * ny + CT_DY[d]) * nx + CT_DX[d];
            u32 vk = 0, pb = 0xFFFFFFFFu;
            if (act && values) {
                const u32 kp = ct_value_key(values[p]), kq = ct_value_key(values[q]);
                vk = kp > kq ? kp : kq;
            }
            if (act && dist) {
                const float w = CT_DZ[d] ? wz[4 * (int64_t)zz + (CT_DX[d] ? 1 : 0) + (CT_DY[d] ? 2 : 0)] : wxy[CT_CLASS[d]];
                const float s = dist[p] + w;                                         // two rounded float32 additions
                pb = __float_as_uint(s + dist[q]);
            }
            while (rem) {
                const int leader = __ffsll((unsigned long long)rem) - 1;
                const u64 kl = __shfl(k, leader, 64);
                const bool mine = act && k == kl;
                const u64 same = __ballot(mine);
                rem &= ~same;
                const u64 pl = (u64)__shfl(p, leader, 64);                           // the lowest lane of the group: its lowest index
                const u32 gv = wave_max32(mine ? vk : 0u), gp = wave_min32(mine ? pb : 0xFFFFFFFFu);
                if (kl != key) {
                    flush();
                    int64_t s = 0;
                    // a table that has overflowed once is discarded by the caller: nobody probes a full table again and again
                    if (lane == leader)
                        s = __hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? -1 : ct_claim(keys, cap, kl);
                    slot = __shfl(s, leader, 64);
                    key = kl;
                    n = 0;
                    lowest = CT_NONE;
                    vmax = 0;
                    pmin = 0xFFFFFFFFu;
                }
                n += (u64)__popcll(same);
                lowest = pl < lowest ? pl : lowest;
                vmax = gv > vmax ? gv : vmax;
                pmin = gp < pmin ? gp : pmin;
            }
        }
    }
};

__global__ __launch_bounds__(CT_THREADS) void contact_insert_kernel(const u64 *__restrict__ bits, const int *__restrict__ zone, int nz, int ny,
                                                                    int nx, int wx, int chunks, int64_t items,
                                                                    const float *__restrict__ values, const float *__restrict__ dist,
                                                                    const float *__restrict__ wxy, const float *__restrict__ wz, int64_t cap,
                                                                    u64 *keys, unsigned long long *pairs, u32 *z_lo, int *z_hi,
                                                                    unsigned long long *first, u32 *value_max, u32 *path,
                                                                    unsigned long long *counters)
{
    const int64_t item = ((int64_t)blockIdx.x * CT_THREADS + threadIdx.x) >> 6;
    if (item >= items) return;
    CtInsert op;
    op.values = values, op.dist = dist, op.wxy = wxy, op.wz = wz;
    op.keys = keys, op.cap = cap, op.pairs = pairs, op.first = first, op.counters = counters;
    op.z_lo = z_lo, op.value_max = value_max, op.path = path, op.z_hi = z_hi;
    op.ny = ny, op.nx = nx, op.lane = threadIdx.x & 63, op.z = 0;
    op.key = 0, op.n = 0, op.lowest = CT_NONE, op.slot = -1, op.vmax = 0, op.pmin = 0xFFFFFFFFu;
    ct_walk(bits, zone, nz, ny, nx, wx, chunks, item, op);
    op.flush();
}

// ---------------------------------------------------------------------------------------------- hist
struct CtHist {
    const float *__restrict__ values;
    const u64 *__restrict__ keys;
    int64_t cap, rows, entries;
    const int *__restrict__ row_of_slot;
    const u32 *__restrict__ z_lo, *__restrict__ value_max;
    const int64_t *__restrict__ offset;
    unsigned long long *hist, *value_index, *counters;
    int ny, nx, lane;
    // the open accumulator
    u64 key, lowest;
    int64_t entry, row;
    u32 want;
    u32 n[CT_CLASSES];

    __device__ inline void flush()
    {
        if (key && lane == 0) {
            if (entry < 0) {
                u64 all = 0;
#pragma unroll
                for (int c = 0; c < CT_CLASSES; c++) all += n[c];
                atomicAdd(counters + 1, (unsigned long long)all);                   // a key the table does not hold: an internal error
            } else {
#pragma unroll
                for (int c = 0; c < CT_CLASSES; c++)
                    if (n[c]) atomicAdd(hist + CT_CLASSES * entry + c, (unsigned long long)n[c]);
                if (values && lowest != CT_NONE) atomicMin(value_index + row, (unsigned long long)lowest);
            }
        }
        key = 0;
    }

    __device__ inline void open(u64 kl, int z, int leader)
    {
        int64_t e = -1, r = -1;
        u32 v = 0;
        if (lane == leader) {
            const int64_t s = ct_find(keys, cap, kl);
            if (s >= 0) {
                r = row_of_slot[s];
                const int64_t lo = (int64_t)z_lo[s];
                if (r >= 0 && r < rows && z >= lo) {
                    e = offset[r] + (z - lo);
                    if (e < 0 || e >= entries) e = -1;                              // never outside the segments the host laid out
                    if (values) v = value_max[s];
                }
            }
        }
        entry = __shfl(e, leader, 64);
        row = __shfl(r, leader, 64);
        want = __shfl(v, leader, 64);
        key = kl;
        lowest = CT_NONE;
#pragma unroll
        for (int c = 0; c < CT_CLASSES; c++) n[c] = 0;
    }

    __device__ inline void at(int z, int y, int x, int own, const int *nb, u32 hit)
    {
        const int64_t p = ((int64_t)z * ny + y) * nx + x;
#pragma unroll
        for (int d = 0; d < 13; d++) {
            const bool act = (hit >> d) & 1;
            u64 rem = __ballot(act);
            if (!rem) continue;
            const u64 k = act ? ct_key(own, nb[d]) : 0;
            const int64_t q = p + ((int64_t)CT_DZ[d] * ny + CT_DY[d]) * nx + CT_DX[d];
            u32 kp = 0, kq = 0;
            if (act && values) kp = ct_value_key(values[p]), kq = ct_value_key(values[q]);
            while (rem) {
                const int leader = __ffsll((unsigned long long)rem) - 1;
                const u64 kl = __shfl(k, leader, 64);
                const bool mine = act && k == kl;
                const u64 same = __ballot(mine);
                rem &= ~same;
                if (kl != key) {
                    flush();
                    open(kl, z, leader);
                }
                n[CT_CLASS[d]] += (u32)__popcll(same);
                if (values) {                                                        // the lowest index that attains the row's maximum
                    u64 c = CT_NONE;
                    if (mine && kq == want) c = (u64)q;
                    if (mine && kp == want) c = (u64)p;                              // p < q
                    c = wave_min64(c);
                    lowest = c < lowest ? c : lowest;
                }
            }
        }
    }
};

__global__ __launch_bounds__(CT_THREADS) void contact_hist_kernel(const u64 *__restrict__ bits, const int *__restrict__ zone, int nz, int ny,
                                                                  int nx, int wx, int chunks, int64_t items, const float *__restrict__ values,
                                                                  int64_t cap, const u64 *__restrict__ keys, const int *__restrict__ row_of_slot,
                                                                  const u32 *__restrict__ z_lo, const u32 *__restrict__ value_max,
                                                                  const int64_t *__restrict__ offset, int64_t rows, unsigned long long *hist,
                                                                  int64_t entries, unsigned long long *value_index, unsigned long long *counters)
{
    const int64_t item = ((int64_t)blockIdx.x * CT_THREADS + threadIdx.x) >> 6;
    if (item >= items) return;
    CtHist op;
    op.values = values, op.keys = keys, op.cap = cap, op.rows = rows, op.entries = entries, op.row_of_slot = row_of_slot;
    op.z_lo = z_lo, op.value_max = value_max, op.offset = offset, op.hist = hist, op.value_index = value_index, op.counters = counters;
    op.ny = ny, op.nx = nx, op.lane = threadIdx.x & 63;
    op.key = 0, op.lowest = CT_NONE, op.entry = -1, op.row = -1, op.want = 0;
#pragma unroll
    for (int c = 0; c < CT_CLASSES; c++) op.n[c] = 0;
    ct_walk(bits, zone, nz, ny, nx, wx, chunks, item, op);
    op.flush();
}

// ---------------------------------------------------------------------------------------------- finish
// One thread per row, as cc_surface_kernel: the slices of the row's segment in ascending k, the classes in ascending order,
// area += (double)count * F[k][class] in plain sequential float64.  directions == 3: only x, y and z enter the sum.
__global__ __launch_bounds__(CT_THREADS) void contact_finish_kernel(int64_t rows, const int *__restrict__ slot_of_row, int64_t cap,
                                                                    const u64 *__restrict__ keys, const u64 *__restrict__ pairs,
                                                                    const u32 *__restrict__ z_lo, const int *__restrict__ z_hi,
                                                                    const u64 *__restrict__ first, const u32 *__restrict__ value_max,
                                                                    const u32 *__restrict__ path, const u64 *__restrict__ value_index,
                                                                    const int64_t *__restrict__ offset, const u64 *__restrict__ hist,
                                                                    int64_t entries, const double *__restrict__ F, int nz, int directions,
                                                                    int64_t *__restrict__ out, unsigned long long *counters)
{
    const int64_t r = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x;
    if (r >= rows) return;
    int64_t *o = out + CT_OUT * r;
    const int64_t s = slot_of_row[r];
    const int64_t lo = s >= 0 && s < cap ? (int64_t)z_lo[s] : 0, hi = s >= 0 && s < cap ? (int64_t)z_hi[s] : -1;
    const int64_t off = offset[r];
    if (s < 0 || s >= cap || lo > hi || hi >= nz || off < 0 || off + (hi - lo) >= entries) {       // a layout that does not fit: an internal error
        atomicAdd(counters + 1, 1ull);
        for (int c = 0; c < CT_OUT; c++) o[c] = 0;
        return;
    }
    double area = 0.0;
    u64 n[CT_CLASSES] = {};
    for (int64_t k = lo; k <= hi; k++) {
#pragma unroll
        for (int c = 0; c < CT_CLASSES; c++) {
            const u64 v = hist[CT_CLASSES * (off + k - lo) + c];
            if (directions == 13 || c == 0 || c == 1 || c == 3) area += (double)v * F[CT_FCOLS * k + c];
            n[c] += v;
        }
    }
    const u64 key = keys[s];
    o[0] = (int64_t)(key >> 32);
    o[1] = (int64_t)(key & 0xFFFFFFFFull);
    o[2] = (int64_t)pairs[s];
#pragma unroll
    for (int c = 0; c < CT_CLASSES; c++) o[3 + c] = (int64_t)n[c];
    o[10] = (int64_t)__double_as_longlong(area);
    o[11] = lo;
    o[12] = hi;
    o[13] = (int64_t)first[s];
    o[14] = value_max ? (int64_t)ct_value_bits(value_max[s]) : 0;
    o[15] = value_index ? (int64_t)value_index[r] : 0;
    o[16] = path ? (int64_t)path[s] : 0;
}

// ---------------------------------------------------------------------------------------------- entry points
TOMO_API int tomo_contact_count(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, unsigned long long *counter, void *stream)
{
    CtGrid g;
    const void *const ptrs[] = {bits, zones, counter};
    if (!bits || !zones || !counter || !ct_distinct(ptrs, 3)) return TOMO_E_ARG;
    const int r = ct_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counter, 0, sizeof(unsigned long long), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(contact_count_kernel, dim3((unsigned)ceil_div64(g.items * 64, CT_THREADS)), dim3(CT_THREADS), 0, st,
                       (const u64 *)bits, (const int *)zones, nz, ny, nx, (int)g.wx, (int)g.chunks, g.items, counter);
    return tomo_status();
}

TOMO_API int tomo_contact_insert(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, const float *values, const float *dist,
                                 const float *wxy, const float *wz, int64_t cap, uint64_t *keys, uint64_t *pairs, int32_t *z_lo,
                                 int32_t *z_hi, uint64_t *first_index, uint32_t *value_max, uint32_t *path, unsigned long long *counters,
                                 void *stream)
{
    CtGrid g;
    const void *const ptrs[] = {bits, zones, values, dist, wxy, wz, keys, pairs, z_lo, z_hi, first_index, value_max, path, counters};
    if (!bits || !zones || !keys || !pairs || !z_lo || !z_hi || !first_index || !counters || (values && !value_max) ||
        (dist && (!path || !wxy || !wz)) || !ct_distinct(ptrs, 14))
        return TOMO_E_ARG;
    int r = ct_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    if (!ct_capacity(cap, &r)) return r;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)cap;
    // an empty slot: key 0, no pairs, z_lo and first_index at their largest, z_hi and value_max at their smallest, path above +inf
    if (hipMemsetAsync(keys, 0, n * 8, st) != hipSuccess || hipMemsetAsync(pairs, 0, n * 8, st) != hipSuccess ||
        hipMemsetAsync(z_lo, 0xFF, n * 4, st) != hipSuccess || hipMemsetAsync(z_hi, 0, n * 4, st) != hipSuccess ||
        hipMemsetAsync(first_index, 0xFF, n * 8, st) != hipSuccess ||
        (values && hipMemsetAsync(value_max, 0, n * 4, st) != hipSuccess) || (dist && hipMemsetAsync(path, 0xFF, n * 4, st) != hipSuccess))
        return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(contact_insert_kernel, dim3((unsigned)ceil_div64(g.items * 64, CT_THREADS)), dim3(CT_THREADS), 0, st,
                       (const u64 *)bits, (const int *)zones, nz, ny, nx, (int)g.wx, (int)g.chunks, g.items, values, dist, wxy, wz, cap,
                       (u64 *)keys, (unsigned long long *)pairs, (u32 *)z_lo, (int *)z_hi, (unsigned long long *)first_index,
                       (u32 *)value_max, (u32 *)path, counters);
    return tomo_status();
}

TOMO_API int tomo_contact_hist(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, const float *values, int64_t cap,
                               const uint64_t *keys, const int32_t *row_of_slot, const int32_t *z_lo, const uint32_t *value_max,
                               const int64_t *offset, int64_t rows, uint64_t *hist, int64_t entries, uint64_t *value_index,
                               unsigned long long *counters, void *stream)
{
    CtGrid g;
    const void *const ptrs[] = {bits, zones, values, keys, row_of_slot, z_lo, value_max, offset, hist, value_index, counters};
    if (!bits || !zones || !keys || !row_of_slot || !z_lo || !offset || !hist || !counters || rows <= 0 || entries <= 0 ||
        (values && (!value_max || !value_index)) || !ct_distinct(ptrs, 11))
        return TOMO_E_ARG;
    int r = ct_grid(nz, ny, nx, &g);
    if (r != TOMO_OK) return r;
    if (!ct_capacity(cap, &r)) return r;
    if (rows > cap) return TOMO_E_ARG;
    if (entries >= ((int64_t)1 << 60) / CT_CLASSES) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)entries * CT_CLASSES * 8, st) != hipSuccess ||
        (values && hipMemsetAsync(value_index, 0xFF, (size_t)rows * 8, st) != hipSuccess))
        return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(contact_hist_kernel, dim3((unsigned)ceil_div64(g.items * 64, CT_THREADS)), dim3(CT_THREADS), 0, st,
                       (const u64 *)bits, (const int *)zones, nz, ny, nx, (int)g.wx, (int)g.chunks, g.items, values, cap, (const u64 *)keys,
                       (const int *)row_of_slot, (const u32 *)z_lo, (const u32 *)value_max, offset, rows, (unsigned long long *)hist, entries,
                       (unsigned long long *)value_index, counters);
    return tomo_status();
}

TOMO_API int tomo_contact_finish(int64_t rows, const int32_t *slot_of_row, int64_t cap, const uint64_t *keys, const uint64_t *pairs,
                                 const int32_t *z_lo, const int32_t *z_hi, const uint64_t *first_index, const uint32_t *value_max,
                                 const uint32_t *path, const uint64_t *value_index, const int64_t *offset, const uint64_t *hist,
                                 int64_t entries, const double *F, int nz, int directions, int64_t *out, unsigned long long *counters,
                                 void *stream)
{
    const void *const ptrs[] = {slot_of_row, keys, pairs, z_lo, z_hi, first_index, value_max, path, value_index, offset, hist, F, out, counters};
    if (!slot_of_row || !keys || !pairs || !z_lo || !z_hi || !first_index || !offset || !hist || !F || !out || !counters || rows <= 0 ||
        entries <= 0 || nz <= 0 || (directions != 3 && directions != 13) || (value_max && !value_index) || !ct_distinct(ptrs, 14))
        return TOMO_E_ARG;
    int r = TOMO_OK;
    if (!ct_capacity(cap, &r)) return r;
    if (rows > cap) return TOMO_E_ARG;
    if (entries >= ((int64_t)1 << 60) / CT_CLASSES) return TOMO_E_SIZE;
    hipLaunchKernelGGL(contact_finish_kernel, dim3((unsigned)ceil_div64(rows, CT_THREADS)), dim3(CT_THREADS), 0, (hipStream_t)stream, rows,
                       (const int *)slot_of_row, cap, (const u64 *)keys, (const u64 *)pairs, (const u32 *)z_lo, (const int *)z_hi,
                       (const u64 *)first_index, (const u32 *)value_max, (const u32 *)path, (const u64 *)value_index, offset,
                       (const u64 *)hist, entries, F, nz, directions, out, counters);
    return tomo_status();
}
