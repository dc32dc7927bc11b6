// chords.hip -- chord lengths of the bit volume along the 13 lattice directions (tomo_chord_hist): the one pass of the library
// that follows a lattice line through the whole volume instead of looking one step ahead.  A direction s = (dz, dy, dx) is
// led by its first non-zero axis.  The nine directions led by z give one lane to every position (j0, i0) of the slice plane:
// at step k the lane looks at voxel (k, (j0 + k dy) mod ny, (i0 + k dx) mod nx), so every voxel of slice k is seen by exactly one
// lane and the 64 lanes of a wave read one or two words of one row.  Where the index wraps, the voxel before the wrap had its
// successor outside the stack: the open chord ends there as a border chord, and a chord that starts right after the wrap is a
// border chord as well.  The three directions led by y do the same per slice with one lane per i0; (0, 0, 1) is a row pass
// over the runs of cc_runs.h.  A lane carries the length, the sum of the fixed-point steps and the border bit of its open chord
// in registers.  Finished chords of fewer than CHORD_BINS voxels go to bins in LDS -- interior chords of one and two voxels,
// three in four on noise, are first counted in registers and combined per wave -- and a workgroup adds its non-zero bins to the
// tables once at its end.  A longer chord goes to slot n mod CHORD_FAR of a second, direct-mapped set of bins in LDS, which the
// first length to come claims for the workgroup; only a length that finds its slot taken by another goes straight to the
// tables: the lines of a solid body or of its background are long and alike, and thousands of adds to one address of global
// memory are what a workgroup must not do (a full 512^3 took 12 ms that way, 1.4 ms is the walk).  Integer atomics only: the
// same bytes on every run.
#include "cc_runs.h"

#define CHORD_THREADS 256
#define CHORD_BINS 256               // bins a workgroup keeps in LDS: chords of 1 .. CHORD_BINS - 1 voxels (6 KiB)
#define CHORD_FAR 256                // direct-mapped bins for the longer ones: slot n mod CHORD_FAR, one length a slot (7 KiB)
#define CHORD_LDS_WORDS (3 * CHORD_BINS + 3 * CHORD_FAR + CHORD_FAR / 2)
#define CHORD_DIRECTIONS 13

// where the finished chords of a thread go
struct ChordSink {
    u64 *lds;                        // [3][CHORD_BINS]: counts, border, sum_q of the workgroup; then [3][CHORD_FAR] and the tags
    u64 *counts, *border, *sum_q;    // the rows of the direction in the tables
    int64_t lmax;
    u32 c1, c2;                      // interior chords of one and of two voxels met by this thread ...
    u64 s1, s2;                      // ... and the sums of their steps

    __device__ void put(u32 n, u64 sq, bool edge)
    {
        if (!edge && n == 1) {
            c1++;
            s1 += sq;
        } else if (!edge && n == 2) {
            c2++;
            s2 += sq;
        } else if (n < CHORD_BINS) {
            atomicAdd(lds + n, 1ull);
            if (edge) atomicAdd(lds + CHORD_BINS + n, 1ull);
            atomicAdd(lds + 2 * CHORD_BINS + n, sq);
        } else if ((int64_t)n <= lmax) {                    // n <= max(nz, ny, nx) <= lmax: the check keeps a wrong lmax harmless
            const u32 slot = n & (CHORD_FAR - 1);
            const u32 owner = atomicCAS(tags() + slot, 0u, n);  // the first length claims the slot; a tag is written once
            if (owner == 0 || owner == n) {
                u64 *far = lds + 3 * CHORD_BINS + slot;
                atomicAdd(far, 1ull);
                if (edge) atomicAdd(far + CHORD_FAR, 1ull);
                atomicAdd(far + 2 * CHORD_FAR, sq);
            } else {
                atomicAdd(counts + n, 1ull);
                if (edge) atomicAdd(border + n, 1ull);
                atomicAdd(sum_q + n, sq);
            }
        }
    }

    __device__ u32 *tags() const { return (u32 *)(lds + 3 * CHORD_BINS + 3 * CHORD_FAR); }

    // every thread of the workgroup comes here: the registers per wave into LDS, then the non-zero bins into the tables
    __device__ void finish()
    {
        const u32 a1 = wave_sum(c1), a2 = wave_sum(c2);
        const u64 b1 = wave_sum64(s1), b2 = wave_sum64(s2);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            if (a1) {
                atomicAdd(lds + 1, (u64)a1);
                atomicAdd(lds + 2 * CHORD_BINS + 1, b1);
            }
            if (a2) {
                atomicAdd(lds + 2, (u64)a2);
                atomicAdd(lds + 2 * CHORD_BINS + 2, b2);
            }
        }
        __syncthreads();
        for (int n = threadIdx.x; n < CHORD_BINS; n += CHORD_THREADS) {
            const u64 c = lds[n];
            if (c == 0 || (int64_t)n > lmax) continue;
            atomicAdd(counts + n, c);
            const u64 e = lds[CHORD_BINS + n];
            if (e) atomicAdd(border + n, e);
            atomicAdd(sum_q + n, lds[2 * CHORD_BINS + n]);
        }
        for (int slot = threadIdx.x; slot < CHORD_FAR; slot += CHORD_THREADS) {
            const u32 n = tags()[slot];
            if (n == 0 || (int64_t)n > lmax) continue;
            const u64 *far = lds + 3 * CHORD_BINS + slot;
            atomicAdd(counts + n, far[0]);
            if (far[CHORD_FAR]) atomicAdd(border + n, far[CHORD_FAR]);
            atomicAdd(sum_q + n, far[2 * CHORD_FAR]);
        }
    }
};

__device__ static inline ChordSink chord_sink_begin(u64 *lds, int m, int64_t lmax, u64 *counts, u64 *border, u64 *sum_q)
{
    for (int t = threadIdx.x; t < CHORD_LDS_WORDS; t += CHORD_THREADS) lds[t] = 0;
    __syncthreads();
    const int64_t row = (int64_t)m * (lmax + 1);
    return {lds, counts + row, border + row, sum_q + row, lmax, 0u, 0u, 0ull, 0ull};
}

// The directions led by z (ZLED: blockIdx.y = 0 .. 8 are the directions 4 .. 12, (1, -1, -1) .. (1, 1, 1); a thread is a position
// (j0, i0) of the slice plane and walks the slices) and those led by y (blockIdx.y = 0 .. 2 are the directions 1 .. 3, (0, 1, -1) ..
// (0, 1, 1); a thread is a slice and a column i0 and walks the rows).  edge: the predecessor of the open chord, or of the next
// chord to open, lies outside the stack.
template <bool ZLED>
__global__ __launch_bounds__(CHORD_THREADS) void chord_walk_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx,
                                                                   const int64_t *__restrict__ steps_q, int64_t lmax,
                                                                   u64 *__restrict__ counts, u64 *__restrict__ border,
                                                                   u64 *__restrict__ sum_q)
{
    __shared__ u64 lds[CHORD_LDS_WORDS];
    const int m = (ZLED ? 4 : 1) + (int)blockIdx.y;
    const int dy = ZLED ? (int)blockIdx.y / 3 - 1 : 0, dx = (int)blockIdx.y % 3 - 1;
    ChordSink sink = chord_sink_begin(lds, m, lmax, counts, border, sum_q);
    const int64_t p = (int64_t)blockIdx.x * CHORD_THREADS + threadIdx.x;
    if (p < (int64_t)(ZLED ? ny : nz) * nx) {
        const int a = (int)(p / nx);
        int i = (int)(p % nx), j = ZLED ? a : 0;
        const int steps = ZLED ? nz : ny;
        u32 n = 0;
        u64 sq = 0;
        bool edge = true;
        for (int t = 0; t < steps; t++) {
            const int k = ZLED ? t : a;
            const u64 word = bits[((int64_t)k * ny + j) * wx + (i >> 6)];
            if ((word >> (i & 63)) & 1ull) {
                n++;
                sq += (u64)steps_q[(int64_t)k * CHORD_DIRECTIONS + m];
            } else {
                if (n) sink.put(n, sq, edge);
                n = 0;
                sq = 0;
                edge = false;
            }
            bool wrap = false;
            j += ZLED ? dy : 1;
            if (ZLED) {
                if (j < 0) {
                    j = ny - 1;
                    wrap = true;
                } else if (j >= ny) {
                    j = 0;
                    wrap = true;
                }
            }
            i += dx;
            if (i < 0) {
                i = nx - 1;
                wrap = true;
            } else if (i >= nx) {
                i = 0;
                wrap = true;
            }
            if (wrap) {                                     // the successor of the voxel just seen lies outside the stack
                if (n) sink.put(n, sq, true);
                n = 0;
                sq = 0;
                edge = true;
            }
        }
        if (n) sink.put(n, sq, true);                       // the line leaves the stack through its last slice / row
    }
    sink.finish();
}

// (0, 0, 1): one thread per row, the chords are its runs; a run that crosses a word boundary is one chord
__global__ __launch_bounds__(CHORD_THREADS) void chord_row_kernel(const u64 *__restrict__ bits, int64_t nrows, int ny, int nx, int wx,
                                                                  const int64_t *__restrict__ steps_q, int64_t lmax,
                                                                  u64 *__restrict__ counts, u64 *__restrict__ border,
                                                                  u64 *__restrict__ sum_q)
{
    __shared__ u64 lds[CHORD_LDS_WORDS];
    ChordSink sink = chord_sink_begin(lds, 0, lmax, counts, border, sum_q);
    const int64_t row = (int64_t)blockIdx.x * CHORD_THREADS + threadIdx.x;
    if (row < nrows) {
        const u64 q = (u64)steps_q[(row / ny) * CHORD_DIRECTIONS];
        for (CcRuns it = cc_runs_begin(bits, row, nx, wx); it.valid; cc_runs_next(it)) {
            const u32 n = (u32)(it.e - it.s);
            sink.put(n, (u64)n * q, it.s == 0 || it.e == nx);
        }
    }
    sink.finish();
}

TOMO_API int tomo_chord_hist(const uint64_t *bits, int nz, int ny, int nx, const int64_t *steps_q, int64_t lmax, int64_t *counts,
                             int64_t *border, int64_t *sum_q, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!steps_q || !counts || !border || !sum_q) return TOMO_E_ARG;
    if (lmax < nz || lmax < ny || lmax < nx) return TOMO_E_ARG;
    if (lmax >= ((int64_t)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)CHORD_DIRECTIONS * (size_t)(lmax + 1) * sizeof(u64);
    if (hipMemsetAsync(counts, 0, bytes, st) != hipSuccess || hipMemsetAsync(border, 0, bytes, st) != hipSuccess ||
        hipMemsetAsync(sum_q, 0, bytes, st) != hipSuccess)
        return TOMO_E_LAUNCH;
    const u64 *b = (const u64 *)bits;
    u64 *c = (u64 *)counts, *e = (u64 *)border, *s = (u64 *)sum_q;
    const dim3 block(CHORD_THREADS);
    hipLaunchKernelGGL((chord_walk_kernel<true>), dim3((unsigned)ceil_div64((int64_t)ny * nx, CHORD_THREADS), 9), block, 0, st, b, nz, ny,
                       nx, wx, steps_q, lmax, c, e, s);
    hipLaunchKernelGGL((chord_walk_kernel<false>), dim3((unsigned)ceil_div64((int64_t)nz * nx, CHORD_THREADS), 3), block, 0, st, b, nz, ny,
                       nx, wx, steps_q, lmax, c, e, s);
    hipLaunchKernelGGL(chord_row_kernel, dim3((unsigned)ceil_div64(nrows, CHORD_THREADS)), block, 0, st, b, nrows, ny, nx, wx, steps_q,
                       lmax, c, e, s);
    return tomo_status();
}
