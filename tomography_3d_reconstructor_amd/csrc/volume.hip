// volume.hip -- the callers either side of the hot path that work on the resident bit volume:
//   * per-slice voxel counts and the bounding box (volume_calculator.py:23-35, 37-57, 59-94): the reference does
//     np.sum(voxel_data[z]) per slice and np.where(voxel_data) (three int64 index arrays, 24 B per set voxel);
//     here both are one streaming pass over 1 bit/voxel;
//   * `img >= threshold` of the mask loader (image_loader.py:108) fused with the bit packing, so the grey
//     stack that was uploaded is never written back as 1 B/voxel booleans.
#include "tomo_common.h"

// ------------------------------------------------------------------------------------------ per-slice counts
// grid (chunks, nz): every block sums its part of slice z and adds it to counts[z] (zeroed by the call)
__global__ __launch_bounds__(256) void slice_popcount_kernel(const u64 *__restrict__ bits, int64_t words_per_slice,
                                                             unsigned long long *__restrict__ counts)
{
    const u64 *sl = bits + (int64_t)blockIdx.y * words_per_slice;
    u64 acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words_per_slice; i += (int64_t)gridDim.x * blockDim.x)
        acc += (u64)__popcll(sl[i]);
    acc = wave_sum64(acc);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&counts[blockIdx.y], (unsigned long long)acc);
}

TOMO_API int tomo_slice_popcounts(const uint64_t *bits, int nz, int ny, int nx, unsigned long long *counts, void *stream)
{
    if (!bits || !counts || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    if (nz > 65535) return TOMO_E_SIZE;
    int64_t wps = (int64_t)ny * tomo_words_per_row(nx);
    if (hipMemsetAsync(counts, 0, (size_t)nz * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
        return TOMO_E_LAUNCH;
    int64_t chunks = ceil_div64(wps, 256 * 16);
    if (chunks > 64) chunks = 64;
    hipLaunchKernelGGL(slice_popcount_kernel, dim3((unsigned)chunks, (unsigned)nz), dim3(256), 0, (hipStream_t)stream,
                       (const u64 *)bits, wps, counts);
    return tomo_status();
}

// ------------------------------------------------------------------------------------------ bounding box
// box = {zmin, zmax, ymin, ymax, xmin, xmax} as int32; an empty volume leaves {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1}
__global__ void bbox_init_kernel(int *box)
{
    if (threadIdx.x < 6) box[threadIdx.x] = (threadIdx.x & 1) ? -1 : 0x7fffffff;
}

__device__ static inline int wave_min_i(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { int o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ static inline int wave_max_i(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(256) void bbox_kernel(const u64 *__restrict__ bits, int64_t nwords, int ny, int wx,
                                                   int *__restrict__ box)
{
    int zmin = 0x7fffffff, zmax = -1, ymin = 0x7fffffff, ymax = -1, xmin = 0x7fffffff, xmax = -1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 w = bits[i];
        if (!w) continue;
        const int64_t row = i / wx;
        const int wi = (int)(i - row * wx);
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const int xl = wi * 64 + (__ffsll((long long)w) - 1), xh = wi * 64 + 63 - __clzll((long long)w);
        zmin = z < zmin ? z : zmin; zmax = z > zmax ? z : zmax;
        ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
        xmin = xl < xmin ? xl : xmin; xmax = xh > xmax ? xh : xmax;
    }
    zmin = wave_min_i(zmin); ymin = wave_min_i(ymin); xmin = wave_min_i(xmin);
    zmax = wave_max_i(zmax); ymax = wave_max_i(ymax); xmax = wave_max_i(xmax);
    if ((threadIdx.x & 63) == 0 && zmax >= 0) {
        atomicMin(&box[0], zmin); atomicMax(&box[1], zmax);
        atomicMin(&box[2], ymin); atomicMax(&box[3], ymax);
        atomicMin(&box[4], xmin); atomicMax(&box[5], xmax);
    }
}

TOMO_API int tomo_bbox(const uint64_t *bits, int nz, int ny, int nx, int32_t *box, void *stream)
{
    if (!bits || !box || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    const int wx = (int)tomo_words_per_row(nx);
    const int64_t nwords = (int64_t)nz * ny * wx;
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, box);
    int64_t blocks = ceil_div64(nwords, 256 * 8);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const u64 *)bits, nwords, ny,
                       wx, box);
    return tomo_status();
}

// ------------------------------------------------------------------------------------------ threshold + pack
// bits = (grey >= threshold): same lane layout as pack16_kernel / pack_kernel of bits.hip.
__device__ static inline u32 ge_nibble(u32 w, u32 k2)
{   // bit i of the result = (byte i of w >= t), k2 = (256 - t) * 0x00010001: the compare is the carry out of byte + (256 - t)
    const u32 ce = (((w & 0x00ff00ffu) + k2) >> 8) & 0x00010001u;          // bytes 0, 2
    const u32 co = ((((w >> 8) & 0x00ff00ffu) + k2) >> 8) & 0x00010001u;   // bytes 1, 3
    return (ce & 1u) | ((co & 1u) << 1) | ((ce >> 16) << 2) | ((co >> 16) << 3);
}

__global__ __launch_bounds__(256) void pack16_threshold_kernel(const uint8_t *__restrict__ grey, u64 *__restrict__ bits,
                                                               int64_t rows, int nx, int wx, int groups, u32 k2)
{
    const int lane = threadIdx.x & 63;
    int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wid >= rows * groups) return;
    int64_t row = wid / groups;
    int g = (int)(wid - row * groups);
    int x = g * 1024 + lane * 16;
    u32 piece = 0;
    if (x < nx) {
        typedef unsigned int u4 __attribute__((ext_vector_type(4)));
        const u4 v = __builtin_nontemporal_load((const u4 *)(grey + row * (int64_t)nx + x));   // read once, keep it out of L2
        piece = ge_nibble(v.x, k2) | (ge_nibble(v.y, k2) << 4) | (ge_nibble(v.z, k2) << 8) | (ge_nibble(v.w, k2) << 12);
    }
    u64 w = (u64)piece << (16 * (lane & 3));
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    int word = g * 16 + (lane >> 2);
    if ((lane & 3) == 0 && word < wx) bits[row * (int64_t)wx + word] = w;
}

__global__ __launch_bounds__(256) void pack_threshold_kernel(const uint8_t *__restrict__ grey, u64 *__restrict__ bits,
                                                             int64_t rows, int nx, int wx, int groups, int threshold)
{
    const int lane = threadIdx.x & 63;
    int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wid >= rows * groups) return;
    int64_t row = wid / groups;
    int g = (int)(wid - row * groups);
    const uint8_t *src = grey + row * (int64_t)nx;
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int x = (g * 16 + k) * 64 + lane;
        int b = x < nx ? (int)src[x] : -1;
        u64 m = __ballot(x < nx && b >= threshold);
        if (lane == k) mine = m;
    }
    int w = g * 16 + lane;
    if (lane < 16 && w < wx) bits[row * (int64_t)wx + w] = mine;
}

TOMO_API int tomo_pack_threshold(const uint8_t *grey, uint64_t *bits, int nz, int ny, int nx, int threshold, void *stream)
{
    if (!grey || !bits || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    int wx = (int)tomo_words_per_row(nx);
    int groups = (wx + 15) / 16;
    int64_t rows = (int64_t)nz * ny;
    int64_t blocks = ceil_div64(rows * groups, 4);
    if (blocks > 0x7fffffff) return TOMO_E_SIZE;
    if (threshold > 255) {                                   // uint8 >= t is never true
        if (hipMemsetAsync(bits, 0, (size_t)rows * wx * sizeof(u64), (hipStream_t)stream) != hipSuccess) return TOMO_E_LAUNCH;
        return TOMO_OK;
    }
    if (threshold < 0) threshold = 0;
    if (nx % 16 == 0 && (((uintptr_t)grey) & 15) == 0)
        hipLaunchKernelGGL(pack16_threshold_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grey,
                           (u64 *)bits, rows, nx, wx, groups, (u32)(256 - threshold) * 0x00010001u);
    else
        hipLaunchKernelGGL(pack_threshold_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grey,
                           (u64 *)bits, rows, nx, wx, groups, threshold);
    return tomo_status();
}

// ------------------------------------------------------------------------------------------ point cloud (rank / select)
// voxel_processor.py:99-127: np.where(voxel_data) -- three int64 index arrays, 24 B per set voxel -- then every k-th entry and
// one float64 row (z_mm[z], y * mm_y, x * mm_x) per kept entry.  Here the rank of a set voxel (np.where's C order = word
// order, then ascending bit) comes from popcounts: a count per TILE of PC_TILE words, one 64-bit scan of the tile counts,
// and a second pass in which every tile ranks its own words and writes the rows whose rank is a multiple of k.
#define PC_THREADS 256
#define PC_ROUNDS 8
#define PC_TILE (PC_THREADS * PC_ROUNDS)        // words per tile; word r * PC_THREADS + t of a tile belongs to thread t, round r
#define PC_CHUNK 4096                            // selected voxels compacted in LDS at a time

TOMO_API int64_t tomo_point_cloud_blocks(int nz, int ny, int nx)
{
    if (nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    return ceil_div64((int64_t)nz * ny * tomo_words_per_row(nx), PC_TILE);
}

__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(const u64 *__restrict__ bits, u32 nwords, u64 *__restrict__ blk_off)
{
    __shared__ u32 wsum[PC_THREADS / 64];
    const u32 base = blockIdx.x * (u32)PC_TILE;
    u32 acc = 0;
#pragma unroll
    for (int r = 0; r < PC_ROUNDS; r++) {
        const u32 i = base + r * PC_THREADS + threadIdx.x;
        acc += i < nwords ? (u32)__popcll(bits[i]) : 0u;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) blk_off[blockIdx.x] = (u64)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: off[i] = base + sum of off[0 .. i) for i <= n, in place, 1024 entries per step with a running carry
__global__ __launch_bounds__(1024) void pc_scan_kernel(u64 *__restrict__ off, int64_t n, u64 base)
{
    __shared__ u64 wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = base;
    for (int64_t i0 = 0; i0 < n; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const u64 v = i < n ? off[i] : 0;
        u64 inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const u64 x = wsum[w];
            before += w < wave ? x : 0;
            total += x;
        }
        if (i < n) off[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = carry;
}

TOMO_API int tomo_point_cloud_count(const uint64_t *bits, int nz, int ny, int nx, uint64_t rank_base, uint64_t *blk_off,
                                    void *stream)
{
    if (!bits || !blk_off || nz <= 0 || ny <= 0 || nx <= 0) return TOMO_E_ARG;
    const int64_t nwords = (int64_t)nz * ny * tomo_words_per_row(nx);
    if (nwords >= ((int64_t)1 << 31)) return TOMO_E_SIZE;            // word indices are 32-bit in the kernels
    const int64_t blocks = ceil_div64(nwords, PC_TILE);
    hipLaunchKernelGGL(pc_count_kernel, dim3((unsigned)blocks), dim3(PC_THREADS), 0, (hipStream_t)stream, (const u64 *)bits,
                       (u32)nwords, (u64 *)blk_off);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (u64 *)blk_off, blocks, (u64)rank_base);
    return tomo_status();
}

// t = q k + r for t < 2^32 or t < 2 k (the only cases the rows kernel forms): one 32-bit division or one subtraction
__device__ static inline void pc_divmod(u64 t, u64 k, u64 *q, u64 *r)
{
    if (((t | k) >> 32) == 0) {
        const u32 qq = (u32)t / (u32)k;
        *q = qq;
        *r = (u32)t - qq * (u32)k;
    } else {
        u64 qq = 0;
        while (t >= k) { t -= k; qq++; }
        *q = qq;
        *r = t;
    }
}
__device__ static inline u64 pc_ceil_div(u64 a, u64 k) { const u64 q = a / k; return q + (a != q * k ? 1 : 0); }

// position of the j-th (0-based) set bit of w; j < popcount(w)
__device__ static inline u32 pc_select(u64 w, u32 j)
{
    u32 pos = 0;
#pragma unroll
    for (int width = 32; width > 0; width >>= 1) {
        const u32 c = (u32)__popcll(w & ((1ull << width) - 1));
        if (j >= c) { j -= c; w >>= width; pos += width; }
    }
    return pos;
}

__global__ __launch_bounds__(PC_THREADS) void pc_rows_kernel(const u64 *__restrict__ bits, u32 nwords, int ny, int wx,
                                                             const u64 *__restrict__ blk_off, u64 k,
                                                             const double *__restrict__ z_mm, double mm_y, double mm_x,
                                                             int64_t row_first, int64_t cap_rows, double *__restrict__ out)
{
    __shared__ double zt[PC_TILE];            // per word of the tile: z_mm[z], y, 64 * (word in row)
    __shared__ u32 yt[PC_TILE];
    __shared__ u32 xt[PC_TILE];
    __shared__ u32 sel[PC_CHUNK];             // (word in tile) << 6 | bit of the selected voxels of the chunk, in row order
    __shared__ u32 wtot[PC_ROUNDS][PC_THREADS / 64];

    const u64 lo = blk_off[blockIdx.x], hi = blk_off[blockIdx.x + 1];
    // rows of this tile: [R0, R1) of the whole run; of those, local rows [ls, le) fall into the caller's window
    const u64 R0 = pc_ceil_div(lo, k), R1 = pc_ceil_div(hi, k);
    const u64 W0 = (u64)row_first, W1 = (u64)row_first + (u64)cap_rows;
    const u64 a = R0 > W0 ? R0 : W0, b = R1 < W1 ? R1 : W1;
    if (a >= b) return;
    const u32 ls = (u32)(a - R0), le = (u32)(b - R0);
    const u64 m = lo % k;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 base = blockIdx.x * (u32)PC_TILE;
    u64 w[PC_ROUNDS];
    u32 pre[PC_ROUNDS];                       // inclusive wave prefix of the popcounts, then the word's exclusive rank in the tile
#pragma unroll
    for (int r = 0; r < PC_ROUNDS; r++) {
        const u32 wi = r * PC_THREADS + threadIdx.x, i = base + wi;
        w[r] = i < nwords ? bits[i] : 0ull;
        pre[r] = wave_inclusive_scan((u32)__popcll(w[r]));
        if (lane == 63) wtot[r][wave] = pre[r];
        if (i < nwords) {
            const u32 row = i / (u32)wx, z = row / (u32)ny;
            zt[wi] = z_mm[z];
            yt[wi] = row - z * (u32)ny;
            xt[wi] = (i - row * (u32)wx) * 64u;
        }
    }
    __syncthreads();
    u32 first[PC_ROUNDS], skip[PC_ROUNDS], nsel[PC_ROUNDS];   // local row of the word's first selected bit, set bits in front of it
    {
        u32 run = 0;
#pragma unroll
        for (int r = 0; r < PC_ROUNDS; r++) {
            u32 before = run;
#pragma unroll
            for (int v = 0; v < PC_THREADS / 64; v++) {
                const u32 x = wtot[r][v];
                before += v < wave ? x : 0u;
                run += x;
            }
            const u32 c = (u32)__popcll(w[r]);
            const u32 p = before + pre[r] - c;                 // set voxels of the tile in front of this word
            u64 q, rem;
            pc_divmod(m + p, k, &q, &rem);
            first[r] = (u32)q + (rem ? 1u : 0u) - (m ? 1u : 0u);   // multiples of k among the ranks [lo, lo + p)
            const u64 j0 = rem ? k - rem : 0;                  // set bits of the word in front of its first selected one
            if (j0 < c) {
                skip[r] = (u32)j0;
                nsel[r] = (c - (u32)j0 - 1) / (u32)(k < 64 ? k : 64) + 1;
            } else {
                skip[r] = 0;
                nsel[r] = 0;
            }
        }
    }

    for (u32 cb = ls - ls % PC_CHUNK; cb < le; cb += PC_CHUNK) {
        const u32 ce = cb + PC_CHUNK;
#pragma unroll
        for (int r = 0; r < PC_ROUNDS; r++) {
            if (!nsel[r] || first[r] >= ce || first[r] + nsel[r] <= cb) continue;
            const u32 tag = (u32)(r * PC_THREADS + threadIdx.x) << 6;
            if (k >= 64) {                                     // one selected bit at most: jump to it
                sel[first[r] - cb] = tag | pc_select(w[r], skip[r]);
            } else {
                u64 ww = w[r];
                u32 j = 0, next = skip[r], row = first[r];
                while (ww) {
                    const u32 bit = (u32)__ffsll((long long)ww) - 1;
                    ww &= ww - 1;
                    if (j == next) {
                        if (row >= cb && row < ce) sel[row - cb] = tag | bit;
                        row++;
                        next += (u32)k;
                    }
                    j++;
                }
            }
        }
        __syncthreads();
        // the rows of the chunk are one run of doubles: lane j stores double j (row j / 3, column j % 3)
        const u32 r_lo = cb > ls ? cb : ls, r_hi = ce < le ? ce : le;
        double *dst = out + 3 * ((int64_t)(R0 - W0) + (int64_t)r_lo);   // >= out: R0 + r_lo >= W0 by the choice of ls
        const u32 nd = 3 * (r_hi - r_lo);
        for (u32 j = threadIdx.x; j < nd; j += PC_THREADS) {
            const u32 row = j / 3, col = j - 3 * row;
            const u32 v = sel[r_lo - cb + row], wi = v >> 6;
            double val;
            if (col == 0) val = zt[wi];
            else if (col == 1) val = (double)yt[wi] * mm_y;
            else val = (double)(xt[wi] + (v & 63u)) * mm_x;
            dst[j] = val;
        }
        __syncthreads();
    }
}

TOMO_API int tomo_point_cloud_rows(const uint64_t *bits, int nz, int ny, int nx, const uint64_t *blk_off, int64_t k,
                                   const double *z_mm, double mm_y, double mm_x, int64_t row_first, int64_t cap_rows,
                                   double *out, void *stream)
{
    if (!bits || !blk_off || !z_mm || nz <= 0 || ny <= 0 || nx <= 0 || k < 1 || row_first < 0 || cap_rows < 0) return TOMO_E_ARG;
    if (cap_rows == 0) return TOMO_OK;
    if (!out) return TOMO_E_ARG;
    const int wx = (int)tomo_words_per_row(nx);
    const int64_t nwords = (int64_t)nz * ny * wx;
    if (nwords >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int64_t blocks = ceil_div64(nwords, PC_TILE);
    hipLaunchKernelGGL(pc_rows_kernel, dim3((unsigned)blocks), dim3(PC_THREADS), 0, (hipStream_t)stream, (const u64 *)bits,
                       (u32)nwords, ny, wx, (const u64 *)blk_off, (u64)k, z_mm, mm_y, mm_x, row_first, cap_rows, out);
    return tomo_status();
}
