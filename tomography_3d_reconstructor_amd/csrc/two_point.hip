// two_point.hip -- the two-point covariance of the bit volume over a box of integer lags (tomo_two_point): pairs[hz][hy + ry]
// [hx + rx] = N(h) = #{p : p set, p + h set, both inside the stack}, the non-periodic estimator.  The one pass of the library that
// is compute bound: a workgroup serves ONE plane (hz, hy) of lags for its chunk of the word space, a thread takes a word A of row
// (k, j) and the three words Bm, B0, Bp round the same place in the partner row (k + hz, j + hy), and for every hx of the plane
// adds popcount(A & shift(B, hx)) to an accumulator of its own -- 2 RX + 1 of them per lane, all in registers: the loop over hx
// is unrolled when compiled (a fold over an index sequence), so every shift is an immediate and every accumulator has a static
// index.  The volume streams past the accumulators; nothing is written until the end, where each accumulator is summed over
// the wave, the four wave sums are combined in LDS and the workgroup sends ONE 64-bit add per lag.  Integer adds only: the same
// bytes on every run and under every grid.  Nobody waits on anybody: no persistent grid, no spin.
#include "cc_runs.h"

#define TWO_POINT_THREADS 256
#define TWO_POINT_WAVES (TWO_POINT_THREADS / WAVE)
#define TWO_POINT_MAX_RX 63          // a shifted word comes from a word and ONE neighbour
// Words of one chunk at the most.  A lane visits at most CHUNK_MAX / 256 = 2^16 words of it and adds at most 64 per visit: a lane's
// accumulator stays below 2^22, a wave's sum below 2^28, the workgroup's below 2^30 -- every sum on the way to the one 64-bit add
// fits 32 bits (the 32-bit popcount adds for free; 2^25 visits a lane would be the bound for the lane's accumulator alone).
#define TWO_POINT_CHUNK_MAX ((int64_t)1 << 24)
#define TWO_POINT_GRID 8192          // workgroups wanted: 32 for each of the 256 compute units, so that the last round is short

// A row's words as 32-bit halves, in ascending x: m0 m1 | c0 c1 | p0 p1 (the word before, the word itself, the word after).  The
// half whose bit x is bit x + S of the 64 bits hi:lo -- one v_alignbit_b32 -- and S = 0 and 32, which are moves.
struct TwoPointRow {
    u32 m0, m1, c0, c1, p0, p1;
};

template <int S>
__device__ static inline u32 two_point_half(u32 lo, u32 hi)
{
    static_assert(S >= 0 && S < 32, "the shift stays inside the pair of halves");
    if constexpr (S == 0)
        return lo;
    else
        return __builtin_amdgcn_alignbit(hi, lo, S);
}

// acc + popcount(x) in ONE instruction: the 32-bit popcount takes an addend.  Written out because the compiler, given two
// popcounts and an accumulator, counts both into zero and joins the three with v_add3_u32: three instructions for two.
__device__ static inline u32 two_point_count(u32 x, u32 acc)
{
    u32 out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(x), "v"(acc));
    return out;
}

// acc += popcount(A & row shifted by HX), HX in [-63, 63]: bit x of the shifted row is bit x + HX of the row.  The 64 bits wanted
// start HX bits into c0 (HX >= 0) or 64 + HX bits into m0 (HX < 0): two funnel shifts over three neighbouring halves, two ANDs,
// and two 32-bit popcounts that add as they count -- six vector instructions a lag, fewer where a shift is a move.
template <int HX>
__device__ static inline u32 two_point_lag(u32 acc, u32 a0, u32 a1, const TwoPointRow &r)
{
    constexpr int T = HX >= 0 ? HX : 64 + HX;               // bits into the pair of words (c, p) or (m, c)
    const u32 w0 = HX >= 0 ? r.c0 : r.m0, w1 = HX >= 0 ? r.c1 : r.m1, w2 = HX >= 0 ? r.p0 : r.c0, w3 = HX >= 0 ? r.p1 : r.c1;
    u32 s0, s1;
    if constexpr (T < 32) {
        s0 = two_point_half<T>(w0, w1);
        s1 = two_point_half<T>(w1, w2);
    } else {
        s0 = two_point_half<T - 32>(w1, w2);
        s1 = two_point_half<T - 32>(w2, w3);
    }
    return two_point_count(a1 & s1, two_point_count(a0 & s0, acc));
}

template <int RX, int... I>
__device__ static inline void two_point_word(u32 (&acc)[2 * RX + 1], u64 A, u64 Bm, u64 B0, u64 Bp, std::integer_sequence<int, I...>)
{
    const TwoPointRow r = {(u32)Bm, (u32)(Bm >> 32), (u32)B0, (u32)(B0 >> 32), (u32)Bp, (u32)(Bp >> 32)};
    const u32 a0 = (u32)A, a1 = (u32)(A >> 32);
    ((acc[I] = two_point_lag<I - RX>(acc[I], a0, a1, r)), ...);
}

// blockIdx.x: the plane (hz, hy) among the planes that can hold a pair at all (hz < nz, |hy| < ny; the others stay zero);
// blockIdx.y: the chunk of the word space.  pairs is the whole table, (rz + 1, 2 ry + 1, 2 rx + 1).
template <int RX>
__global__ __launch_bounds__(TWO_POINT_THREADS) void two_point_kernel(const u64 *__restrict__ bits, int nz, int ny, int nx, int wx,
                                                                      int64_t nwords, int64_t chunk, int ryc, int ry, int rx,
                                                                      u64 *__restrict__ pairs)
{
    constexpr int NL = 2 * RX + 1;
    __shared__ u32 part[TWO_POINT_WAVES][NL];
    const int hz = (int)(blockIdx.x / (unsigned)(2 * ryc + 1)), hy = (int)(blockIdx.x % (unsigned)(2 * ryc + 1)) - ryc;
    u32 acc[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) acc[l] = 0;
    const int64_t begin = (int64_t)blockIdx.y * chunk;
    const int64_t end = begin + chunk < nwords ? begin + chunk : nwords;
    // word i = base + threadIdx.x is word w of row (k, j): one division here, carries from then on
    int64_t i = begin + threadIdx.x;
    const int dw = TWO_POINT_THREADS % wx, drow = TWO_POINT_THREADS / wx, dj = drow % ny, dk = drow / ny;
    const int64_t row = i / wx;
    int w = (int)(i - row * wx), k = (int)(row / ny), j = (int)(row - (int64_t)k * ny);
    for (int64_t base = begin; base < end; base += TWO_POINT_THREADS, i += TWO_POINT_THREADS) {      // the same turns for every thread
        const int kp = k + hz, jp = j + hy;
        const bool inside = i < end && kp < nz && jp >= 0 && jp < ny;
        const u64 A = inside ? cc_word(bits + ((int64_t)k * ny + j) * wx, nx, wx, w) : 0ull;
        if (__any(A != 0ull)) {                             // a wave without a set bit that has a partner row skips the word
            const u64 *prow = inside ? bits + ((int64_t)kp * ny + jp) * wx : nullptr;
            const u64 Bm = (prow && w > 0) ? cc_word(prow, nx, wx, w - 1) : 0ull;
            const u64 B0 = cc_word_or0(prow, nx, wx, w);
            const u64 Bp = cc_word_or0(prow, nx, wx, w + 1);
            two_point_word<RX>(acc, A, Bm, B0, Bp, std::make_integer_sequence<int, NL>{});
        }
        w += dw;
        j += dj;
        k += dk;
        if (w >= wx) {
            w -= wx;
            j++;
        }
        if (j >= ny) {
            j -= ny;
            k++;
        }
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const u32 s = wave_sum(acc[l]);
        if (lane == 0) part[wave][l] = s;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < NL; l += TWO_POINT_THREADS) {
        const int hx = l - RX;
        if (hx < -rx || hx > rx) continue;                  // the variant is wider than the box: those columns are not in the table
        u32 s = 0;
#pragma unroll
        for (int v = 0; v < TWO_POINT_WAVES; v++) s += part[v][l];
        if (s) atomicAdd(pairs + ((int64_t)hz * (2 * ry + 1) + (hy + ry)) * (2 * rx + 1) + (hx + rx), (u64)s);
    }
}

template <int RX>
static void two_point_go(const u64 *bits, int nz, int ny, int nx, int wx, int64_t nwords, int64_t chunk, dim3 grid, int ryc, int ry,
                         int rx, u64 *pairs, hipStream_t st)
{
    hipLaunchKernelGGL(two_point_kernel<RX>, grid, dim3(TWO_POINT_THREADS), 0, st, bits, nz, ny, nx, wx, nwords, chunk, ryc, ry, rx,
                       pairs);
}

TOMO_API int tomo_two_point(const uint64_t *bits, int nz, int ny, int nx, int rz, int ry, int rx, int64_t *pairs, void *stream)
{
    int64_t nrows;
    int wx;
    const int g = cc_geometry(bits, nz, ny, nx, &nrows, &wx);
    if (g != TOMO_OK) return g;
    if (!pairs || rz < 0 || ry < 0 || rx < 0 || rx > TWO_POINT_MAX_RX) return TOMO_E_ARG;
    const unsigned __int128 cells = (unsigned __int128)((int64_t)rz + 1) * (unsigned __int128)(2 * (int64_t)ry + 1) *
                                    (unsigned __int128)(2 * rx + 1);
    if (cells >= ((unsigned __int128)1 << 31)) return TOMO_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(pairs, 0, (size_t)cells * sizeof(u64), st) != hipSuccess) return TOMO_E_LAUNCH;
    // the planes that can hold a pair: a lag that reaches the size of its axis reads 0, which the table already does
    const int rzc = rz < nz - 1 ? rz : nz - 1, ryc = ry < ny - 1 ? ry : ny - 1;
    const int64_t planes = ((int64_t)rzc + 1) * (2 * (int64_t)ryc + 1);      // <= cells < 2^31: they fit the grid's x
    const int64_t nwords = nrows * wx;
    // chunks per plane: enough for TWO_POINT_GRID workgroups in all, never fewer than TWO_POINT_CHUNK_MAX asks for, never more
    // than there are rounds of 256 words; an address takes one add per chunk
    int64_t chunks = ceil_div64(TWO_POINT_GRID, planes);
    const int64_t least = ceil_div64(nwords, TWO_POINT_CHUNK_MAX), most = ceil_div64(nwords, TWO_POINT_THREADS);
    if (chunks < least) chunks = least;
    if (chunks > most) chunks = most;
    if (chunks > 65535) chunks = 65535;                     // the grid's y; least <= 2^31 / 2^24 = 128
    const int64_t chunk = ceil_div64(ceil_div64(nwords, chunks), TWO_POINT_THREADS) * TWO_POINT_THREADS;
    const dim3 grid((unsigned)planes, (unsigned)ceil_div64(nwords, chunk));
    const u64 *b = (const u64 *)bits;
    u64 *p = (u64 *)pairs;
    if (rx <= 8)                                            // the smallest variant that holds the box: 17, 33, 65 or 127 lags a plane
        two_point_go<8>(b, nz, ny, nx, wx, nwords, chunk, grid, ryc, ry, rx, p, st);
    else if (rx <= 16)
        two_point_go<16>(b, nz, ny, nx, wx, nwords, chunk, grid, ryc, ry, rx, p, st);
    else if (rx <= 32)
        two_point_go<32>(b, nz, ny, nx, wx, nwords, chunk, grid, ryc, ry, rx, p, st);
    else
        two_point_go<63>(b, nz, ny, nx, wx, nwords, chunk, grid, ryc, ry, rx, p, st);
    return tomo_status();
}
