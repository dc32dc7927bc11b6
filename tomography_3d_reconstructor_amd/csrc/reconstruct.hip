// reconstruct.hip -- greyscale morphological reconstruction by dilation inside the set voxels of the resident bit volume (no
// counterpart in the reference): a map g that rises under a ceiling f.  Contract, order and the fixed-point argument:
// include/tomo_hip.h.
//
// g(p) = max(m'(p), min(f(p), max over the set neighbours q of g(q))), m' = min(marker, f).  Minima and maxima only, of values
// that are already present: the operator is monotone, values only rise through the finite set of the inputs, so there is ONE
// least fixed point above m' and every order of updates ends there.  It is tomo_geo_sweep's argument turned round, and so is
// the kernel: the same tiles, flags, rounds and marks, on the skeleton of geo_tiles.h.
//
// Order.  Values are compared through recon_key(), an order-preserving uint32 image of the float: sign and magnitude folded
// onto one ascending axis around 0x80000000.  -0.0 and +0.0 share a key, the keys of the finite values and the two infinities
// are consecutive integers -- the float just below v is key - 1 -- and no float mode or denormal setting takes part in a
// comparison.  Key 0 is below -inf: it stands for "no voxel" in the halo box and never raises anything.
//
// One sweep (tomo_recon_sweep).  A workgroup whose flag is clear leaves at once.  Otherwise a thread loads the ceiling and g of
// its 16 voxels into REGISTERS (lane = x, rows wave + 4 k, as in tomo_geo_sweep): the ceiling of a voxel is read by its owner
// alone, so it needs no place in LDS -- only g has a halo box there, 26 400 bytes.  A tile whose voxels all sit at their ceiling
// is finished for good and leaves before it loads the box.  The interior is then raised against the FIXED halo in race-free
// rounds (candidates from the published box, barrier, publish, __syncthreads_or), bounded by GEO_ROUNDS; a voxel that reached
// its ceiling drops out of the rounds.  Changed voxels are stored by their owner alone, the neighbouring tiles next to a changed
// face, edge or corner voxel are marked in dirty_next.  A stale neighbour value is a valid LOWER bound of the fixed point,
// aligned 32-bit accesses do not tear, and the writer marks the reader: nothing waits on another workgroup.
#include "geo_tiles.h"
#include <float.h>

#define RECON_F_NAN 8ull                           // counters[1]: NaN in the mask or the marker of a set voxel
#define RECON_F_WORK 16ull                         // counters[1]: some set voxel starts below its ceiling
#define RECON_KEY_ZERO 0x80000000u                 // the key of +-0.0
#define RECON_KEY_NEG_INF 0x00800000u              // the key of -inf: the lowest key of a value

__device__ static inline u32 recon_key(float v)
{
    const u32 b = __float_as_uint(v), mag = b & 0x7fffffffu;
    return (b >> 31) ? RECON_KEY_ZERO - mag : RECON_KEY_ZERO + mag;
}

__device__ static inline float recon_value(u32 k)
{
    return __uint_as_float(k >= RECON_KEY_ZERO ? k - RECON_KEY_ZERO : (0x80000000u | (RECON_KEY_ZERO - k)));
}

__device__ static inline bool recon_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// ---------------------------------------------------------------------------------------------- seeding
// a wave is one word of a row, a lane one voxel: g = min(marker, mask) on a set voxel, 0.0 elsewhere.  The flags of a wave go
// out with one atomic, and only while counters[1] lacks them: a volume full of work does not queue its waves on one address.
__global__ __launch_bounds__(GEO_THREADS) void recon_seed_kernel(const u64 *__restrict__ bits, const float *__restrict__ mask,
                                                                 const float *__restrict__ marker, int mode, float h, int64_t nwords,
                                                                 int nx, int wx, float *__restrict__ g, unsigned long long *counters)
{
    GeoLane p;
    if (!geo_lane(nwords, wx, &p)) return;
    float out = 0.0f;
    bool nan = false, work = false;
    if (p.x < nx && ((bits[p.word] >> p.b) & 1)) {           // below nx: no tail bit is read
        const float f = mask[p.row * nx + p.x];
        const float m = mode == 0 ? marker[p.row * nx + p.x] : mode == 1 ? f - h : f;
        nan = recon_nan(f) || recon_nan(m);
        const u32 kf = recon_key(f);
        u32 km = recon_key(m);
        if (mode == 2 && kf > RECON_KEY_NEG_INF) km = kf - 1;             // nothing lies below -inf
        const u32 k = min(km, kf);
        out = recon_value(k);
        work = k < kf;
    }
    if (p.x < nx) g[p.row * nx + p.x] = out;
    const u64 nans = __ballot(nan), works = __ballot(work);
    if (p.b == 0) {
        const unsigned long long flags = (nans ? RECON_F_NAN : 0ull) | (works ? RECON_F_WORK : 0ull);
        if (flags & ~__atomic_load_n(counters + 1, __ATOMIC_RELAXED)) atomicOr(counters + 1, flags);
    }
}

// ---------------------------------------------------------------------------------------------- one sweep
// the largest key among the neighbours of a voxel of the halo box; strides: x 1, y GEO_HX, z GEO_HY * GEO_HX
template <int CONN>
__device__ static inline u32 recon_reach(const u32 *__restrict__ p)
{
    const int sy = GEO_HX, sz = GEO_HY * GEO_HX;
    u32 c = max(max(p[-1], p[1]), max(max(p[-sy], p[sy]), max(p[-sz], p[sz])));
    if (CONN == 26) {
        c = max(c, max(max(p[-sy - 1], p[-sy + 1]), max(p[sy - 1], p[sy + 1])));
#pragma unroll
        for (int s = -1; s <= 1; s += 2) {
            const u32 *q = p + s * sz;
            c = max(c, max(max(q[-1], q[1]), max(q[-sy], q[sy])));
            c = max(c, max(max(q[-sy - 1], q[-sy + 1]), max(q[sy - 1], q[sy + 1])));
        }
    }
    return c;
}

// interior row r = wave + 4 k of a thread -> its place in the halo box, without the lane.  geo_box_at() is the same place; with
// it the rounds of the 26-neighbour instance ran 3 to 5 % longer (profiles/r37_sweep_skeleton.md), so the rounds keep this form.
__device__ static inline int recon_box_row(int r) { return ((r / GEO_TY + 1) * GEO_HY + (r % GEO_TY + 1)) * GEO_HX + 1; }

// Two workgroups per CU, the bound of its siblings: the compiler fills it (244 VGPRs, nothing spilled).  Bounds of 3 and 4
// workgroups were compiled as well and spill about 500 and 700 bytes a lane into scratch, so they were not taken.
template <int CONN>
__global__ __launch_bounds__(GEO_THREADS, 2) void recon_sweep_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx, int ty,
                                                                  const float *__restrict__ mask, float *g, u32 *dirty_cur,
                                                                  u32 *dirty_next, unsigned long long *counters)
{
    __shared__ u32 box[GEO_BOX];                             // keys of g; 0 at unset voxels and outside the stack
    __shared__ u64 smid[GEO_HROWS];                          // the word of a halo row; 0 outside the stack
    __shared__ u32 sside[GEO_HROWS];                         // bit 0: the voxel left of the word is set, bit 1: right
    __shared__ u32 snb;                                      // the neighbouring tiles to mark, one bit per (dz, dy, dx)

    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (!geo_enter(dirty_cur, tile, &snb)) return;
    const GeoTile t = geo_tile(tile, wx, ty);
    geo_halo_masks(bits, nz, ny, nx, wx, t, smid, sside);
    __syncthreads();

    // the thread's 16 voxels: ceiling and value in registers.  A set voxel lies inside the stack and below nx.
    const int lane = tid & 63, wave = tid >> 6;
    u32 f[GEO_PER], v[GEO_PER];
    u32 live = 0, moved = 0;                                 // bit k: voxel k is set and below its ceiling / has changed since the load
#pragma unroll
    for (int k = 0; k < GEO_PER; k++) {
        const int r = wave + 4 * k, lz = r / GEO_TY, ly = r % GEO_TY;
        f[k] = v[k] = 0u;
        if ((smid[geo_halo_row(lz, ly)] >> lane) & 1) {
            const int64_t at = geo_voxel(t, lz, ly, lane, ny, nx);
            f[k] = recon_key(mask[at]);
            v[k] = recon_key(g[at]);
            if (v[k] < f[k]) live |= 1u << k;
        }
    }
    if (!__syncthreads_or((int)live)) return;                // every voxel sits at its ceiling: nothing can rise, now or later

    for (int i = tid; i < GEO_BOX; i += GEO_THREADS) {
        const int hr = i / GEO_HX, xx = i - hr * GEO_HX;
        box[i] = geo_halo_set(smid, sside, hr, xx) ? recon_key(g[geo_halo_voxel(t, hr, xx, ny, nx)]) : 0u;
    }
    __syncthreads();

    int more = 1, round = 0;
    for (; round < GEO_ROUNDS && more; round++) {            // bounded: a tile that needs more marks itself in geo_leave
        u32 now = 0;
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            if (!((live >> k) & 1)) continue;
            const u32 c = min(f[k], recon_reach<CONN>(box + recon_box_row(wave + 4 * k) + lane));
            if (c > v[k]) {
                v[k] = c;
                now |= 1u << k;
            }
        }
        __syncthreads();                                     // every candidate of the round is formed: publish
#pragma unroll
        for (int k = 0; k < GEO_PER; k++) {
            if ((now >> k) & 1) {
                box[recon_box_row(wave + 4 * k) + lane] = v[k];
                if (v[k] == f[k]) live &= ~(1u << k);        // at its ceiling: out of the rounds
            }
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
        g[geo_voxel(t, lz, ly, lane, ny, nx)] = recon_value(v[k]);
        nb |= geo_marks(geo_steps(lz, GEO_TZ), geo_steps(ly, GEO_TY), geo_steps(lane, 64));
    }
    geo_leave<CONN>(nb, more, &snb, tile, t, nz, ty, wx, dirty_next, counters);
}

// ---------------------------------------------------------------------------------------------- below the ceiling
// out word = the set voxels with g < mask in the order of the keys; a wave is one word, tail bits zero
__global__ __launch_bounds__(GEO_THREADS) void recon_below_kernel(const u64 *__restrict__ bits, const float *__restrict__ mask,
                                                                  const float *__restrict__ g, int64_t nwords, int nx, int wx,
                                                                  u64 *__restrict__ out)
{
    GeoLane p;
    if (!geo_lane(nwords, wx, &p)) return;
    bool bit = false;
    if (p.x < nx && ((bits[p.word] >> p.b) & 1)) bit = recon_key(g[p.row * nx + p.x]) < recon_key(mask[p.row * nx + p.x]);
    const u64 m = __ballot(bit);
    if (p.b == 0) out[p.word] = m;
}

// ---------------------------------------------------------------------------------------------- entry points
TOMO_API int tomo_recon_seed(const uint64_t *bits, const float *mask, const float *marker, int mode, float h, int nz, int ny, int nx,
                             float *g, unsigned long long *counters, void *stream)
{
    GeoGrid grid;
    if (!bits || !mask || !g || !counters || mode < 0 || mode > 2 || (mode == 0 && !marker) || g == mask || g == marker ||
        (const void *)g == (const void *)bits || (mode == 1 && !(h > 0.0f && h <= FLT_MAX)))
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(recon_seed_kernel, dim3((unsigned)ceil_div64(grid.words * 64, GEO_THREADS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, mask, marker, mode, h, grid.words, nx, (int)grid.wx, g, counters);
    return tomo_status();
}

TOMO_API int tomo_recon_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *mask, float *g,
                              uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters, void *stream)
{
    GeoGrid grid;
    if (!bits || !mask || !g || !dirty_cur || !dirty_next || !counters || dirty_cur == dirty_next || g == mask ||
        (const void *)g == (const void *)bits || (connectivity != 6 && connectivity != 26))
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    geo_launch<recon_sweep_kernel<6>, recon_sweep_kernel<26>>(connectivity, dim3((unsigned)grid.tiles), stream, (const u64 *)bits, nz, ny,
                                                              nx, (int)grid.wx, (int)grid.ty, mask, g, dirty_cur, dirty_next, counters);
    return tomo_status();
}

TOMO_API int tomo_recon_below(const uint64_t *bits, const float *mask, const float *g, int nz, int ny, int nx, uint64_t *out, void *stream)
{
    GeoGrid grid;
    if (!bits || !mask || !g || !out || g == mask || out == bits || (const void *)out == (const void *)mask ||
        (const void *)out == (const void *)g)
        return TOMO_E_ARG;
    const int r = geo_grid(nz, ny, nx, &grid);
    if (r != TOMO_OK) return r;
    hipLaunchKernelGGL(recon_below_kernel, dim3((unsigned)ceil_div64(grid.words * 64, GEO_THREADS)), dim3(GEO_THREADS), 0,
                       (hipStream_t)stream, (const u64 *)bits, mask, g, grid.words, nx, (int)grid.wx, (u64 *)out);
    return tomo_status();
}
