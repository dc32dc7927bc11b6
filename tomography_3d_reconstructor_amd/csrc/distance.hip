// distance.hip -- exact Euclidean distance transform of the resident bit volume in millimetres, with per-slice depths
// (scipy.ndimage.distance_transform_edt cannot express those; no counterpart in the reference, whose "SDF" is a smoothed
// occupancy).  Contract: include/tomo_hip.h.
//
// Sites and coordinates.  Axis a has the coordinate table ta[0 .. na + 1]: ta[i + 1] is the centre of index i and ta[0] /
// ta[na + 1] are the two VIRTUAL sites just outside the volume.  inside != 0: the sites are the unset voxels and every virtual
// position (one layer of background round the volume); the result at a set voxel is the distance to the nearest site, at an
// unset voxel 0.  inside == 0: the sites are the set voxels, virtual positions are never sites, no site at all gives +inf.
//
// Three separable passes, every one an exact minimum over its line, d2 = ((dx^2 + dy^2) + dz^2) in float64 without contraction
// (the Makefile passes -ffp-contract=off): rounding is monotone, so the minimum per line of the rounded partial sums is the
// rounded 3-D minimum.
//   x  from the 64-bit words: a wave is one word of a row, the nearest site left and right of a lane comes from bit scans of
//      the word and, past its ends, of the neighbouring words (a wave-uniform walk); g = min(dxl^2, dxr^2).
//   y, z  the lower envelope of the parabolas f(s) + (t - p[s])^2 (Felzenszwalb & Huttenlocher) over the sites with finite f,
//      one thread per line, 64 lanes adjacent in x so that every load and store of a step is one 512-byte row.  The envelope
//      stack (site index, left end of its interval) lives in the workspace, [slot][lane] like the lines: nothing per line sits
//      in registers or scratch.  The VALUE written is always f(s) + (t - p[s])^2 of the chosen site, formed as above; only the
//      choice between two sites whose parabolas cross within rounding of t can differ from the exhaustive minimum.
// The volume is processed in chunks of cw columns of x (a multiple of 64): the workspace holds two float64 planes of
// nz * ny * cw and the stack, never a per-voxel array of the whole volume.  The last pass ends in one of three tails: float32
// sqrt, a comparison of d2 with r^2 that is balloted into bit words, or a (maximum, first index) reduction -- per thread, then
// one workgroup folds the partials in a fixed order: no float atomics, the same answer on every run.
//
// Local thickness (Hildebrand & Ruegsegger) by levels, contract in include/tomo_hip.h: one inside transform whose tail keeps
// d2 itself (float64, the only per-voxel float64 array), then per squared radius r2 the eroded set {set && d2 >= r2} balloted
// into bits, one OUTSIDE transform of those bits whose tail stores the level where d2 < r2 at a set voxel of the original
// volume (levels ascend, later ones overwrite: the maximum), and one finishing pass that turns the level map into float32
// through a host-made table and counts the voxels per (slice, level) with integer atomics only.
#include "tomo_common.h"
#include <math.h>

#define EDT_THREADS 256
#define EDT_TAIL_PLANE 0             // y pass: float64 plane for the z pass
#define EDT_TAIL_FLOAT 1
#define EDT_TAIL_GT 2                // bit = d2 > r2
#define EDT_TAIL_LE 3                // bit = d2 <= r2
#define EDT_TAIL_ARGMAX 4
#define EDT_TAIL_SQUARED 5           // float64 d2 (nz, ny, nx)
#define EDT_TAIL_GE_AND 6            // bit = d2 >= r2 && mask bit
#define EDT_TAIL_LT_AND 7            // bit = d2 < r2 && mask bit
#define EDT_TAIL_COVER 8             // map = level where d2 < r2 && mask bit
#define EDT_FINISH_LDS 4096          // levels (K + 1) the finishing pass counts in LDS; beyond: straight global atomics

struct EdtPlan {
    int64_t cw;                      // columns per chunk
    int64_t plane;                   // doubles of one float64 plane
    int64_t stack;                   // entries of the stack
    int64_t parts;                   // argmax partials
    int64_t bytes;
};

static int edt_plan(int nz, int ny, int nx, int64_t cw, EdtPlan *p)
{
    const int64_t a = (int64_t)(ny + 2) * nz, b = (int64_t)(nz + 2) * ny;
    p->cw = cw;
    p->plane = (int64_t)nz * ny * cw;
    p->stack = (a > b ? a : b) * cw;
    p->parts = (int64_t)ny * cw;
    p->bytes = 2 * p->plane * 8 + p->stack * 8 + p->parts * 8 + p->stack * 4 + p->parts * 4;
    return TOMO_OK;
}

static inline int64_t edt_column_bytes(int nz, int ny)
{
    EdtPlan p;
    edt_plan(nz, ny, 64, 64, &p);
    return p.bytes / 64;
}

TOMO_API int64_t tomo_edt_chunk_columns(int nz, int ny, int nx, int64_t workspace_bytes)
{
    if (nz <= 0 || ny <= 0 || nx <= 0 || workspace_bytes <= 0) return TOMO_E_ARG;
    const int64_t all = 64 * tomo_words_per_row(nx);
    int64_t cw = workspace_bytes / edt_column_bytes(nz, ny) / 64 * 64;
    if (cw < 64) return TOMO_E_WORKSPACE;
    return cw < all ? cw : all;
}

TOMO_API int64_t tomo_edt_workspace_bytes(int nz, int ny, int nx, int64_t budget_bytes)
{
    if (nz <= 0 || ny <= 0 || nx <= 0 || budget_bytes < 0) return TOMO_E_ARG;
    const int64_t col = edt_column_bytes(nz, ny);
    int64_t cw = tomo_edt_chunk_columns(nz, ny, nx, budget_bytes > 64 * col ? budget_bytes : 64 * col);
    return cw * col;
}

// ---------------------------------------------------------------------------------------------- x pass
// site word w of a row: bit b = position 64 w + b is a site.  inside: the unset voxels and every position from nx on (the
// virtual site nx is the first of them); else the set voxels below nx, whatever the buffer holds in the tail bits
__device__ static inline u64 edt_sites(const u64 *__restrict__ row, int nx, int wx, int w, int inside)
{
    const int r = nx - 64 * (wx - 1);
    const u64 tail = (w == wx - 1 && r < 64) ? ((1ull << r) - 1) : ~0ull;
    const u64 v = row[w] & tail;
    return inside ? ~v : v;
}

#define EDT_NONE (-2)

// G[(row * cw) + c] = min over the sites s of the row of (xt[x + 1] - xt[s + 1])^2, x = x0 + c; +inf without a site
__global__ __launch_bounds__(EDT_THREADS) void edt_x_kernel(const u64 *__restrict__ bits, int64_t nrows, int nx, int wx, int x0, int cw,
                                                            const double *__restrict__ xt, int inside, double *__restrict__ G)
{
    const int64_t t = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
    const int64_t row = t / cw;
    const int c = (int)(t - row * cw);
    const int x = x0 + c;
    if (row >= nrows || x >= nx) return;
    const u64 *r = bits + row * wx;
    const int w0 = x >> 6, b = x & 63;
    int l, rr;
    {
        int w = w0;
        u64 m = edt_sites(r, nx, wx, w, inside) & (~0ull >> (63 - b));
        while (m == 0 && --w >= 0) m = edt_sites(r, nx, wx, w, inside);        // w only falls: at most wx turns
        l = m ? 64 * w + 63 - __clzll((long long)m) : (inside ? -1 : EDT_NONE);
    }
    {
        int w = w0;
        u64 m = edt_sites(r, nx, wx, w, inside) & (~0ull << b);
        while (m == 0 && ++w < wx) m = edt_sites(r, nx, wx, w, inside);        // w only grows
        rr = m ? 64 * w + __ffsll((long long)m) - 1 : (inside ? nx : EDT_NONE);
        if (rr > nx) rr = nx;                                                  // cannot be: the first tail position IS nx
    }
    const double px = xt[x + 1];
    double g = INFINITY;
    if (l != EDT_NONE) {
        const double d = px - xt[l + 1];
        g = d * d;
    }
    if (rr != EDT_NONE) {
        const double d = xt[rr + 1] - px;
        const double g2 = d * d;
        g = g2 < g ? g2 : g;
    }
    G[row * cw + c] = g;
}

// ---------------------------------------------------------------------------------------------- line passes
// One line: slots s = 0 .. n + 1 at positions p[s]; f(0) = f(n + 1) = vval (the virtual sites), f(s) = in[(s - 1) * es].
struct EdtLine {
    const double *in;
    int64_t es;
    double vval;
    int n;
};

__device__ static inline double edt_f(const EdtLine &L, int s)
{
    return (s == 0 || s == L.n + 1) ? L.vval : L.in[(int64_t)(s - 1) * L.es];
}

// geometry of a pass, in elements: thread (o, c) works on the line at in + o * in_ls + c with stride in_es, its stack at
// o * st_ls + c with stride st_es.  y pass: o = z;  z pass: o = y.
struct EdtPass {
    const double *in;
    const double *p;                 // n + 2 positions
    int32_t *sv;
    double *sz;
    int64_t in_ls, in_es, st_ls, st_es;
    int64_t outer;                   // lines per column
    int n, cw, x0, nx, ny, wx;
    int inside;
    double r2;
    double *plane;                   // EDT_TAIL_PLANE: same geometry as `in`
    float *out;                      // EDT_TAIL_FLOAT: (nz, ny, nx)
    u64 *obits;                      // EDT_TAIL_GT / LE: (nz, ny, wx)
    float *pval;                     // EDT_TAIL_ARGMAX: one partial per thread
    int64_t *pidx;
    double *out2;                    // EDT_TAIL_SQUARED: (nz, ny, nx)
    const u64 *mask;                 // EDT_TAIL_GE_AND / LT_AND / COVER: (nz, ny, wx), the volume the answer is confined to
    int32_t *map;                    // EDT_TAIL_COVER: (nz, ny, nx)
    int level;
};

template <int TAIL>
__global__ __launch_bounds__(EDT_THREADS) void edt_line_kernel(const EdtPass P)
{
    const int64_t t = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
    const int64_t o = t / P.cw;                              // the same for the 64 lanes of a wave: cw is a multiple of 64
    if (o >= P.outer) return;                                // whole waves leave
    const int c = (int)(t - o * P.cw);
    const int x = P.x0 + c;
    const bool live = x < P.nx;
    const int n = P.n;
    EdtLine L = {P.in + o * P.in_ls + c, P.in_es, P.inside ? 0.0 : (double)INFINITY, n};
    int32_t *sv = P.sv + o * P.st_ls + c;
    double *sz = P.sz + o * P.st_ls + c;
    const double *__restrict__ p = P.p;

    // the envelope: slots of the stack 0 .. top, the parabola of slot k rules from sz[k] to sz[k + 1]
    int top = -1;
    int tv = 0;
    double tf = 0, tp = 0, tz = 0;                           // the top entry, in registers
    if (live) {
        for (int s = 0; s <= n + 1; s++) {
            const double fs = edt_f(L, s);
            if (!(fs < INFINITY)) continue;                  // not a site
            const double ps = p[s];
            double sx = -INFINITY;
            while (top >= 0) {                               // every turn but the last pops: at most top turns
                sx = ((fs + ps * ps) - (tf + tp * tp)) / (2.0 * (ps - tp));
                if (top == 0 || sx > tz) break;              // slot 0 (tz = -inf) is never popped, whatever the tables hold
                top--;
                tv = sv[(int64_t)top * P.st_es];
                tz = sz[(int64_t)top * P.st_es];
                tf = edt_f(L, tv);
                tp = p[tv];
            }
            top++;                                           // <= the sites seen so far - 1 <= n + 1
            tv = s;
            tf = fs;
            tp = ps;
            tz = sx;
            sv[(int64_t)top * P.st_es] = tv;
            sz[(int64_t)top * P.st_es] = tz;
        }
    }

    // the fill, ascending: k only grows
    int k = 0;
    double cf = INFINITY, cp = 0, nextz = INFINITY;
    if (live && top >= 0) {
        const int v0 = sv[0];
        cf = edt_f(L, v0);
        cp = p[v0];
        nextz = top > 0 ? sz[P.st_es] : (double)INFINITY;
    }
    float best = -1.0f;
    int64_t best_i = -1;
    for (int q = 0; q < n; q++) {                            // wave-uniform trip count: the ballot below needs every lane
        double d2 = INFINITY;
        if (live && top >= 0) {
            const double pq = p[q + 1];
            while (nextz < pq) {                             // at most top turns over the whole line
                k++;
                const int v = sv[(int64_t)k * P.st_es];
                cf = edt_f(L, v);
                cp = p[v];
                nextz = k < top ? sz[(int64_t)(k + 1) * P.st_es] : (double)INFINITY;
            }
            const double d = pq - cp;
            d2 = cf + d * d;
        }
        if (TAIL == EDT_TAIL_PLANE) {
            if (live) P.plane[o * P.in_ls + c + (int64_t)q * P.in_es] = d2;
        } else {
            const int64_t row = (int64_t)q * P.ny + o;       // z pass: q = z, o = y
            if (TAIL == EDT_TAIL_FLOAT) {
                if (live) P.out[row * P.nx + x] = (float)sqrt(d2);
            } else if (TAIL == EDT_TAIL_SQUARED) {
                if (live) P.out2[row * P.nx + x] = d2;
            } else if (TAIL == EDT_TAIL_COVER) {             // an unset voxel keeps its 0 even where d2 is an ulp off
                if (live && d2 < P.r2 && ((P.mask[row * P.wx + (x >> 6)] >> (x & 63)) & 1)) P.map[row * P.nx + x] = P.level;
            } else if (TAIL == EDT_TAIL_GE_AND || TAIL == EDT_TAIL_LT_AND) {
                const bool bit = live && (TAIL == EDT_TAIL_GE_AND ? d2 >= P.r2 : d2 < P.r2);
                const u64 word = __ballot(bit);              // bits past nx are not live: the tail stays zero
                if ((threadIdx.x & 63) == 0) P.obits[row * P.wx + (x >> 6)] = word & P.mask[row * P.wx + (x >> 6)];
            } else if (TAIL == EDT_TAIL_ARGMAX) {
                const float v = (float)sqrt(d2);
                if (live && v > best) {                      // q ascends = the flat index ascends: the first maximum stays
                    best = v;
                    best_i = row * P.nx + x;
                }
            } else {
                const bool bit = live && (TAIL == EDT_TAIL_GT ? d2 > P.r2 : d2 <= P.r2);
                const u64 word = __ballot(bit);              // the wave is word x0 / 64 + c / 64 of the row
                if ((threadIdx.x & 63) == 0) P.obits[row * P.wx + (x >> 6)] = word;
            }
        }
    }
    if (TAIL == EDT_TAIL_ARGMAX) {
        P.pval[t] = best;
        P.pidx[t] = best_i;
    }
}

// larger value first, then the smaller index; an index < 0 is "nothing"
__device__ static inline void edt_better(float &v, int64_t &i, float ov, int64_t oi)
{
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

// one workgroup: res = the best of res and the n partials.  res int64[2]: [0] the float32 bits of the value, [1] the index
__global__ __launch_bounds__(1024) void edt_argmax_kernel(const float *__restrict__ pval, const int64_t *__restrict__ pidx, int64_t n,
                                                          int64_t *res)
{
    __shared__ float bv[16];
    __shared__ int64_t bi[16];
    float v = -1.0f;
    int64_t i = -1;
    for (int64_t j = threadIdx.x; j < n; j += 1024) edt_better(v, i, pval[j], pidx[j]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int64_t oi = __shfl_xor(i, d, 64);
        edt_better(v, i, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) {
        bv[threadIdx.x >> 6] = v;
        bi[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) edt_better(v, i, bv[w], bi[w]);
        edt_better(v, i, __int_as_float((int)res[0]), res[1]);
        res[0] = (int64_t)(u32)__float_as_int(v);
        res[1] = i;
    }
}

__global__ void edt_argmax_init_kernel(int64_t *res)
{
    res[0] = (int64_t)(u32)__float_as_int(-1.0f);
    res[1] = -1;
}

// ---------------------------------------------------------------------------------------------- local thickness
// out word (row, w) = the set voxels of `bits` with d2 >= r2; a wave is one word, tail bits zero
__global__ __launch_bounds__(EDT_THREADS) void edt_at_least_kernel(const double *__restrict__ d2, const u64 *__restrict__ bits,
                                                                   int64_t nwords, int nx, int wx, double r2, u64 *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
    const int64_t word = t >> 6;                             // the same for the 64 lanes of a wave
    if (word >= nwords) return;
    const int64_t row = word / wx;
    const int b = (int)(t & 63);
    const int x = (int)(word - row * wx) * 64 + b;
    const bool bit = x < nx && ((bits[word] >> b) & 1) && d2[row * nx + x] >= r2;
    const u64 w = __ballot(bit);
    if (b == 0) out[word] = w;
}

// map int32 (nz, ny, nx) -> float32 in place: values[level - 1] at a set voxel of level >= 1, 0.0f elsewhere; counts[z][l] +=
// the set voxels of slice z at level l.  A workgroup stays inside one slice: its counters are private in LDS (K + 1 <=
// EDT_FINISH_LDS) and are added to the table once.  Integer atomics only: the same bytes on every run.
__global__ __launch_bounds__(EDT_THREADS) void edt_finish_kernel(int32_t *map, const u64 *__restrict__ bits, int64_t slice, int nx, int wx,
                                                                 const float *__restrict__ values, int K, unsigned long long *counts,
                                                                 int blocks_per_slice, int lds)
{
    extern __shared__ unsigned int edt_hist[];
    const int z = blockIdx.x / blocks_per_slice;
    const int64_t per = (slice + blocks_per_slice - 1) / blocks_per_slice;
    const int64_t a = (int64_t)(blockIdx.x - z * blocks_per_slice) * per;
    const int64_t e = a + per < slice ? a + per : slice;
    unsigned long long *cz = counts + (int64_t)z * (K + 1);
    if (lds) {
        for (int l = threadIdx.x; l <= K; l += EDT_THREADS) edt_hist[l] = 0;
        __syncthreads();
    }
    for (int64_t i = a + threadIdx.x; i < e; i += EDT_THREADS) {
        const int64_t y = i / nx;
        const int x = (int)(i - y * nx);
        const int64_t at = (int64_t)z * slice + i;
        int l = map[at];
        if ((unsigned)l > (unsigned)K) l = 0;                // nothing writes such a level; never index past the tables
        const bool set = (bits[((int64_t)z * (slice / nx) + y) * wx + (x >> 6)] >> (x & 63)) & 1;
        float v = 0.0f;
        if (set) {
            if (l > 0) v = values[l - 1];
            if (lds) atomicAdd(&edt_hist[l], 1u);
            else atomicAdd(&cz[l], 1ull);
        }
        ((float *)map)[at] = v;
    }
    if (lds) {
        __syncthreads();
        for (int l = threadIdx.x; l <= K; l += EDT_THREADS)
            if (edt_hist[l]) atomicAdd(&cz[l], (unsigned long long)edt_hist[l]);
    }
}

static int edt_run(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt, int inside,
                   int tail, double r2, void *result, void *workspace, int64_t workspace_bytes, void *stream,
                   const uint64_t *mask = nullptr, int level = 0)
{
    if (!bits || !zt || !yt || !xt || !result || !workspace || nz <= 0 || ny <= 0 || nx <= 0 || workspace_bytes <= 0 ||
        result == (const void *)bits)
        return TOMO_E_ARG;
    if (tail >= EDT_TAIL_GE_AND && (!mask || result == (const void *)mask)) return TOMO_E_ARG;
    if (!(r2 >= 0.0)) return TOMO_E_ARG;
    const int64_t cw = tomo_edt_chunk_columns(nz, ny, nx, workspace_bytes);
    if (cw < 0) return (int)cw;
    const int wx = (int)tomo_words_per_row(nx);
    const int64_t nrows = (int64_t)nz * ny;
    EdtPlan pl;
    edt_plan(nz, ny, nx, cw, &pl);
    if (pl.bytes > workspace_bytes) return TOMO_E_WORKSPACE;
    if (ceil_div64(pl.plane, EDT_THREADS) >= ((int64_t)1 << 31) || ceil_div64(pl.stack, EDT_THREADS) >= ((int64_t)1 << 31))
        return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    double *G = (double *)workspace, *H = G + pl.plane, *sz = H + pl.plane;
    int64_t *pidx = (int64_t *)(sz + pl.stack);
    int32_t *sv = (int32_t *)(pidx + pl.parts);
    float *pval = (float *)(sv + pl.stack);
    if (tail == EDT_TAIL_ARGMAX) hipLaunchKernelGGL(edt_argmax_init_kernel, dim3(1), dim3(1), 0, st, (int64_t *)result);
    for (int64_t x0 = 0; x0 < 64 * (int64_t)wx; x0 += cw) {
        const int64_t w = 64 * (int64_t)wx - x0 < cw ? 64 * (int64_t)wx - x0 : cw;        // this chunk's columns, a multiple of 64
        hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)ceil_div64(nrows * w, EDT_THREADS)), dim3(EDT_THREADS), 0, st,
                           (const u64 *)bits, nrows, nx, wx, (int)x0, (int)w, xt, inside, G);
        EdtPass P;
        P.in = G;
        P.p = yt;
        P.sv = sv;
        P.sz = sz;
        P.in_ls = (int64_t)ny * w;
        P.in_es = w;
        P.st_ls = (int64_t)(ny + 2) * w;
        P.st_es = w;
        P.outer = nz;
        P.n = ny;
        P.cw = (int)w;
        P.x0 = (int)x0;
        P.nx = nx;
        P.ny = ny;
        P.wx = wx;
        P.inside = inside;
        P.r2 = r2;
        P.plane = H;
        P.out = nullptr;
        P.obits = nullptr;
        P.pval = nullptr;
        P.pidx = nullptr;
        P.out2 = nullptr;
        P.mask = (const u64 *)mask;
        P.map = nullptr;
        P.level = level;
        hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_PLANE>, dim3((unsigned)ceil_div64((int64_t)nz * w, EDT_THREADS)), dim3(EDT_THREADS),
                           0, st, P);
        P.in = H;
        P.p = zt;
        P.in_ls = w;
        P.in_es = (int64_t)ny * w;
        P.st_ls = w;
        P.st_es = (int64_t)ny * w;
        P.outer = ny;
        P.n = nz;
        P.plane = nullptr;
        const dim3 grid((unsigned)ceil_div64((int64_t)ny * w, EDT_THREADS));
        if (tail == EDT_TAIL_FLOAT) {
            P.out = (float *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_FLOAT>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_GT) {
            P.obits = (u64 *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_GT>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_LE) {
            P.obits = (u64 *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_LE>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_SQUARED) {
            P.out2 = (double *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_SQUARED>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_GE_AND) {
            P.obits = (u64 *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_GE_AND>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_LT_AND) {
            P.obits = (u64 *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_LT_AND>, grid, dim3(EDT_THREADS), 0, st, P);
        } else if (tail == EDT_TAIL_COVER) {
            P.map = (int32_t *)result;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_COVER>, grid, dim3(EDT_THREADS), 0, st, P);
        } else {
            P.pval = pval;
            P.pidx = pidx;
            hipLaunchKernelGGL(edt_line_kernel<EDT_TAIL_ARGMAX>, grid, dim3(EDT_THREADS), 0, st, P);
            hipLaunchKernelGGL(edt_argmax_kernel, dim3(1), dim3(1024), 0, st, (const float *)pval, (const int64_t *)pidx,
                               (int64_t)ny * w, (int64_t *)result);
        }
    }
    return tomo_status();
}

TOMO_API int tomo_edt_distance(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt,
                               int inside, float *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    return edt_run(bits, nz, ny, nx, zt, yt, xt, inside ? 1 : 0, EDT_TAIL_FLOAT, 0.0, out, workspace, workspace_bytes, stream);
}

TOMO_API int tomo_edt_threshold(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt,
                                int inside, double r2, int keep_greater, uint64_t *out, void *workspace, int64_t workspace_bytes,
                                void *stream)
{
    return edt_run(bits, nz, ny, nx, zt, yt, xt, inside ? 1 : 0, keep_greater ? EDT_TAIL_GT : EDT_TAIL_LE, r2, out, workspace,
                   workspace_bytes, stream);
}

TOMO_API int tomo_edt_argmax(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt,
                             int inside, int64_t *result, void *workspace, int64_t workspace_bytes, void *stream)
{
    return edt_run(bits, nz, ny, nx, zt, yt, xt, inside ? 1 : 0, EDT_TAIL_ARGMAX, 0.0, result, workspace, workspace_bytes, stream);
}

TOMO_API int tomo_edt_squared(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt,
                              int inside, double *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    return edt_run(bits, nz, ny, nx, zt, yt, xt, inside ? 1 : 0, EDT_TAIL_SQUARED, 0.0, out, workspace, workspace_bytes, stream);
}

TOMO_API int tomo_edt_threshold_masked(const uint64_t *sites, int nz, int ny, int nx, const double *zt, const double *yt,
                                       const double *xt, int inside, double r2, int keep_less, const uint64_t *mask, uint64_t *out,
                                       void *workspace, int64_t workspace_bytes, void *stream)
{
    return edt_run(sites, nz, ny, nx, zt, yt, xt, inside ? 1 : 0, keep_less ? EDT_TAIL_LT_AND : EDT_TAIL_GE_AND, r2, out, workspace,
                   workspace_bytes, stream, mask);
}

TOMO_API int tomo_edt_at_least(const double *d2, const uint64_t *bits, int nz, int ny, int nx, double r2, uint64_t *out, void *stream)
{
    if (!d2 || !bits || !out || nz <= 0 || ny <= 0 || nx <= 0 || out == bits || (const void *)out == (const void *)d2) return TOMO_E_ARG;
    if (!(r2 >= 0.0)) return TOMO_E_ARG;
    const int wx = (int)tomo_words_per_row(nx);
    const int64_t nwords = (int64_t)nz * ny * wx;
    if (ceil_div64(nwords * 64, EDT_THREADS) >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipLaunchKernelGGL(edt_at_least_kernel, dim3((unsigned)ceil_div64(nwords * 64, EDT_THREADS)), dim3(EDT_THREADS), 0,
                       (hipStream_t)stream, d2, (const u64 *)bits, nwords, nx, wx, r2, (u64 *)out);
    return tomo_status();
}

TOMO_API int tomo_edt_cover(const uint64_t *sites, const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt,
                            const double *xt, double r2, int level, int32_t *map, void *workspace, int64_t workspace_bytes,
                            void *stream)
{
    if (level < 1) return TOMO_E_ARG;
    return edt_run(sites, nz, ny, nx, zt, yt, xt, 0, EDT_TAIL_COVER, r2, map, workspace, workspace_bytes, stream, bits, level);
}

TOMO_API int tomo_edt_thickness_finish(int32_t *map, const uint64_t *bits, int nz, int ny, int nx, const float *values, int levels,
                                       int64_t *counts, void *stream)
{
    if (!map || !bits || !counts || nz <= 0 || ny <= 0 || nx <= 0 || levels < 0 || (levels > 0 && !values) ||
        (const void *)map == (const void *)bits || (const void *)counts == (const void *)map || (const void *)counts == (const void *)bits)
        return TOMO_E_ARG;
    const int64_t slice = (int64_t)ny * nx;
    int64_t bps = ceil_div64(slice, 16 * EDT_THREADS);           // 16 voxels a thread: the LDS counters are worth their flush
    if (bps * nz >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    const int lds = levels + 1 <= EDT_FINISH_LDS;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)nz * (levels + 1) * 8, st) != hipSuccess) return tomo_status();
    hipLaunchKernelGGL(edt_finish_kernel, dim3((unsigned)(bps * nz)), dim3(EDT_THREADS), lds ? (size_t)(levels + 1) * 4 : 0, st, map,
                       (const u64 *)bits, slice, nx, (int)tomo_words_per_row(nx), values, levels, (unsigned long long *)counts, (int)bps,
                       lds);
    return tomo_status();
}
