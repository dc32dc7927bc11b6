// glb.hip -- the device half of the GLB export (glb_exporter.py of the reference, 52-91 and the trimesh calls of 26-49):
// layer colours, the undirected edge table of a triangle mesh, face orientation (consistency check, then a union-find with
// parity when the winding is not consistent), the signed volume after the per-face flips, and the packing of positions and
// indices straight into the GLB binary chunk.  The orientation contract is written out in include/tomo_hip.h.
#include "tomo_common.h"

namespace {

constexpr u64 EMPTY_KEY = ~0ULL;
constexpr int BLOCK = 256;

static inline unsigned grid_for(int64_t n, int64_t cap = 4096)
{
    int64_t b = ceil_div64(n > 0 ? n : 1, BLOCK);
    return (unsigned)(b > cap ? cap : b);
}

// Table layout inside the caller's buffer: keys u64[cap] | count u32[cap] | entries u32[2 cap] (face << 1 | direction).
// cap = the power of two >= max(1024, 2 * 3 nf): at most a quarter of the slots are ever taken on a closed mesh (every
// undirected edge of a closed mesh is inserted twice).
static inline int64_t table_cap(int64_t nf)
{
    int64_t want = 6 * nf, cap = 1024;
    while (cap < want) cap <<= 1;
    return cap;
}
static inline int64_t table_bytes(int64_t nf) { return table_cap(nf) * (8 + 4 + 8); }

struct Table {
    u64 *keys;
    u32 *cnt;
    u32 *ent;
    int64_t cap;
};

static inline Table table_view(void *base, int64_t cap)
{
    char *p = (char *)base;
    return Table{(u64 *)p, (u32 *)(p + 8 * cap), (u32 *)(p + 12 * cap), cap};
}

__device__ static inline u64 mix64(u64 k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// one atomicAdd per wave of a per-lane count
__device__ static inline void wave_add(unsigned long long *dst, u32 v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// ---- layer colours (glb_exporter.py:52-91) ------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void layer_colors_kernel(const T *__restrict__ v, int64_t nv, int64_t stride, double s1,
                                                              double e1, int en1, double s2, double e2, int en2,
                                                              u32 *__restrict__ rgba)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < nv; i += (int64_t)gridDim.x * BLOCK) {
        const double z = (double)v[i * stride];
        u32 c = 0xffc8c8c8u;                                       // 200, 200, 200, 255 (little endian RGBA)
        if (en1 && z >= s1 && z <= e1) c = 0xff0000ffu;           // 255, 0, 0, 255
        if (en2 && z >= s2 && z <= e2) c = 0xffff0000u;           // 0, 0, 255, 255: blue is applied after red
        rgba[i] = c;
    }
}

// ---- edge table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void edge_insert_kernel(const int64_t *__restrict__ faces, int64_t nf, int64_t nv, Table t,
                                                             unsigned long long *__restrict__ counters)
{
    u32 bad = 0, degenerate = 0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) { bad++; continue; }
        if (a == b || b == c || a == c) { degenerate++; continue; }
        const int64_t from[3] = {a, b, c}, to[3] = {b, c, a};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const u64 lo = (u64)(from[e] < to[e] ? from[e] : to[e]), hi = (u64)(from[e] < to[e] ? to[e] : from[e]);
            const u64 key = (lo << 32) | hi;
            const u32 dir = from[e] < to[e] ? 0u : 1u;
            u64 s = mix64(key) & (u64)(t.cap - 1);
            for (int64_t probe = 0; probe < t.cap; probe++) {
                const u64 old = atomicCAS(&t.keys[s], EMPTY_KEY, key);
                if (old == EMPTY_KEY || old == key) {
                    const u32 k = atomicAdd(&t.cnt[s], 1u);
                    if (k < 2) t.ent[2 * s + k] = ((u32)f << 1) | dir;
                    break;
                }
                s = (s + 1) & (u64)(t.cap - 1);
            }
        }
    }
    wave_add(&counters[4], bad);
    wave_add(&counters[5], degenerate);
}

__global__ __launch_bounds__(BLOCK) void edge_classify_kernel(Table t, unsigned long long *__restrict__ counters)
{
    u32 boundary = 0, manifold = 0, nonmanifold = 0, inconsistent = 0;
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.cap; s += (int64_t)gridDim.x * BLOCK) {
        if (t.keys[s] == EMPTY_KEY) continue;
        const u32 n = t.cnt[s];
        if (n == 1) boundary++;
        else if (n == 2) {
            manifold++;
            if (((t.ent[2 * s] ^ t.ent[2 * s + 1]) & 1u) == 0) inconsistent++;    // both faces run the edge the same way
        } else nonmanifold++;
    }
    wave_add(&counters[0], boundary);
    wave_add(&counters[1], manifold);
    wave_add(&counters[2], nonmanifold);
    wave_add(&counters[3], inconsistent);
}

// ---- seam edges of a mesh that is cut into ranks (the multi-rank paragraph of the orientation contract) --------------------
// one atomicAdd per wave of a per-lane SIGNED count (two's complement: the counters are read as int64)
__device__ static inline void wave_add_signed(unsigned long long *dst, int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)(long long)v);
}

// Every table entry whose two endpoints are ghost rows (local index >= first_ghost: lo < hi, so lo decides) becomes one
// record {key in the UPPER rank's local indices, direction bits << 32 | face count}.  *count ends as the number of such
// entries whatever cap is; records beyond cap are not written.  The loop bound is wave-uniform (cap and the stride are
// multiples of 64), so the ballot sees whole waves.
__global__ __launch_bounds__(BLOCK) void seam_collect_kernel(Table t, u64 first_ghost, int64_t cap, u64 *__restrict__ msg,
                                                              unsigned long long *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.cap; s += (int64_t)gridDim.x * BLOCK) {
        const u64 key = t.keys[s];
        const bool hit = key != EMPTY_KEY && (key >> 32) >= first_ghost;
        const u64 mask = __ballot(hit);
        if (!mask) continue;
        unsigned long long base = 0;
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (!hit) continue;
        const int64_t at = (int64_t)base + __popcll(mask & ((1ULL << lane) - 1ULL));
        if (at >= cap) continue;
        const u32 n = t.cnt[s];
        const u32 bits = (t.ent[2 * s] & 1u) | (n >= 2 ? (t.ent[2 * s + 1] & 1u) << 1 : 0u);
        msg[2 * at] = (((key >> 32) - first_ghost) << 32) | ((key & 0xffffffffULL) - first_ghost);
        msg[2 * at + 1] = ((u64)bits << 32) | (u64)n;
    }
}

__device__ static inline void seam_class(u32 n, int sign, int &boundary, int &manifold, int &nonmanifold)
{
    if (n == 1) boundary += sign;
    else if (n == 2) manifold += sign;
    else if (n >= 3) nonmanifold += sign;
}

// The upper rank's half: each record is looked up in this rank's table (read only).  corr[0..3] receive what has to be
// ADDED to (the lower rank's counters + this rank's counters) so that the edge counts once, in the class of c_lo + c_hi.
__global__ __launch_bounds__(BLOCK) void seam_merge_kernel(Table t, const u64 *__restrict__ msg, int64_t n,
                                                            unsigned long long *__restrict__ corr)
{
    int boundary = 0, manifold = 0, nonmanifold = 0, inconsistent = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const u64 key = msg[2 * i], w = msg[2 * i + 1];
        const u32 c_lo = (u32)w, bits = (u32)(w >> 32);
        if (c_lo == 0) continue;
        u32 c_hi = 0, e0 = 0, e1 = 0;
        u64 s = mix64(key) & (u64)(t.cap - 1);
        for (int64_t probe = 0; probe < t.cap; probe++) {
            const u64 k = t.keys[s];
            if (k == key) {
                c_hi = t.cnt[s];
                e0 = t.ent[2 * s];
                e1 = c_hi >= 2 ? t.ent[2 * s + 1] : 0u;
                break;
            }
            if (k == EMPTY_KEY) break;
            s = (s + 1) & (u64)(t.cap - 1);
        }
        if (c_hi == 0) continue;                       // the lower rank's own count stands
        const u32 sum = c_lo + c_hi;
        seam_class(sum, 1, boundary, manifold, nonmanifold);
        seam_class(c_lo, -1, boundary, manifold, nonmanifold);
        seam_class(c_hi, -1, boundary, manifold, nonmanifold);
        if (sum == 2) {                                // one face on either side: they run the edge the same way or not
            if (((bits ^ e0) & 1u) == 0) inconsistent++;
        } else {                                       // three or more faces: no pair; take back what either side counted
            if (c_lo == 2 && ((bits ^ (bits >> 1)) & 1u) == 0) inconsistent--;
            if (c_hi == 2 && ((e0 ^ e1) & 1u) == 0) inconsistent--;
        }
    }
    wave_add_signed(&corr[0], boundary);
    wave_add_signed(&corr[1], manifold);
    wave_add_signed(&corr[2], nonmanifold);
    wave_add_signed(&corr[3], inconsistent);
}

// ---- union-find with parity ---------------------------------------------------------------------------------------------
// uf[f] = parent << 1 | parity of f relative to its parent.  A root holds (f << 1 | 0).  Every link points from a larger
// face index to a smaller one (hooking puts the larger root under the smaller; compression only moves a link further up
// the same chain), so there are no cycles and each component's root is its lowest-index face.
__device__ static inline u64 uf_load(const u64 *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (root << 1 | parity of x relative to root); links x straight to the root it found (one 64-bit store: root and parity)
__device__ static inline u64 uf_find(u64 *uf, u32 x)
{
    const u64 w = uf_load(uf + x);
    const u32 p = (u32)(w >> 1);
    if (p == x) return w;
    u32 cur = p, par = (u32)(w & 1);
    for (;;) {
        const u64 wc = uf_load(uf + cur);
        const u32 pc = (u32)(wc >> 1);
        if (pc == cur) break;
        par ^= (u32)(wc & 1);
        cur = pc;
    }
    const u64 res = ((u64)cur << 1) | par;
    if (cur != p) __hip_atomic_store(uf + x, res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // x is not a root: nobody hooks it
    return res;
}

__global__ __launch_bounds__(BLOCK) void uf_init_kernel(u64 *__restrict__ uf, u32 *__restrict__ conflict, int64_t nf)
{
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        uf[f] = (u64)f << 1;
        conflict[f] = 0;
    }
}

__global__ __launch_bounds__(BLOCK) void uf_union_kernel(Table t, u64 *uf)
{
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.cap; s += (int64_t)gridDim.x * BLOCK) {
        if (t.keys[s] == EMPTY_KEY || t.cnt[s] != 2) continue;
        const u32 e0 = t.ent[2 * s], e1 = t.ent[2 * s + 1];
        const u32 f = e0 >> 1, g = e1 >> 1;
        if (f == g) continue;
        const u32 r = ((e0 ^ e1) & 1u) ^ 1u;          // 1: the two faces must end up with opposite flips
        for (;;) {
            const u64 a = uf_find(uf, f), b = uf_find(uf, g);
            const u32 ra = (u32)(a >> 1), rb = (u32)(b >> 1);
            if (ra == rb) break;                       // same component: the verification pass judges this edge
            const u32 p = (u32)((a ^ b) & 1) ^ r;
            const u32 hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
            const u64 expect = (u64)hi << 1;
            if (atomicCAS((unsigned long long *)&uf[hi], (unsigned long long)expect, (unsigned long long)(((u64)lo << 1) | p)) == expect)
                break;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void uf_resolve_kernel(u64 *uf, int64_t nf, u32 *__restrict__ root, uint8_t *__restrict__ flip,
                                                            unsigned long long *__restrict__ counts)
{
    u32 comps = 0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        const u64 w = uf_find(uf, (u32)f);
        root[f] = (u32)(w >> 1);
        flip[f] = (uint8_t)(w & 1);
        comps += (u32)(w >> 1) == (u32)f;
    }
    wave_add(&counts[0], comps);
}

// every manifold edge whose two faces do not end up opposite marks its component (the pass that decides conflicts)
__global__ __launch_bounds__(BLOCK) void uf_verify_kernel(Table t, const u32 *__restrict__ root, const uint8_t *__restrict__ flip,
                                                           u32 *__restrict__ conflict)
{
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.cap; s += (int64_t)gridDim.x * BLOCK) {
        if (t.keys[s] == EMPTY_KEY || t.cnt[s] != 2) continue;
        const u32 e0 = t.ent[2 * s], e1 = t.ent[2 * s + 1];
        const u32 f = e0 >> 1, g = e1 >> 1;
        const u32 r = ((e0 ^ e1) & 1u) ^ 1u;
        if (((u32)(flip[f] ^ flip[g])) != r) conflict[root[f]] = 1;
    }
}

__global__ __launch_bounds__(BLOCK) void uf_conflict_kernel(int64_t nf, const u32 *__restrict__ root, const u32 *__restrict__ conflict,
                                                             uint8_t *__restrict__ flip, unsigned long long *__restrict__ counts)
{
    u32 bad = 0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        const u32 r = root[f];
        if (conflict[r]) {
            flip[f] = 0;                               // a conflicting component is left as given
            bad += r == (u32)f;
        }
    }
    wave_add(&counts[1], bad);
}

// ---- signed volume after the flips, packing -----------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void signed_volume_kernel(const float *__restrict__ v, const int64_t *__restrict__ faces, int64_t nf,
                                                               const uint8_t *__restrict__ flip, double *__restrict__ out)
{
    double vol = 0.0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        const float *a = v + 3 * faces[3 * f], *b = v + 3 * faces[3 * f + 1], *c = v + 3 * faces[3 * f + 2];
        // the arithmetic of tomo_mesh_volume_area; a reversed face contributes the negated term
        float cx = b[1] * c[2] - b[2] * c[1], cy = b[2] * c[0] - b[0] * c[2], cz = b[0] * c[1] - b[1] * c[0];
        float d = a[0] * cx + a[1] * cy + a[2] * cz;
        const double t = (double)d / 6.0;
        vol += (flip && flip[f]) ? -t : t;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) vol += __shfl_xor(vol, d, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, vol);
}

template <typename O>
__global__ __launch_bounds__(BLOCK) void pack_faces_kernel(const int64_t *__restrict__ faces, int64_t nf, const uint8_t *__restrict__ flip,
                                                            const double *__restrict__ volume, O *__restrict__ out)
{
    const u32 all = (volume && *volume < 0.0) ? 1u : 0u;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const bool rev = ((flip ? (u32)flip[f] : 0u) ^ all) != 0;
        out[3 * f] = (O)(rev ? c : a);
        out[3 * f + 1] = (O)b;
        out[3 * f + 2] = (O)(rev ? a : c);
    }
}

// float -> u32 whose unsigned order is the float order (for atomicMin / atomicMax)
__device__ static inline u32 f2key(float x)
{
    const u32 u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ static inline float key2f(u32 k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void minmax_init_kernel(u32 *keys)
{
    if (threadIdx.x < 6) keys[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

__global__ void minmax_decode_kernel(u32 *keys)
{
    if (threadIdx.x < 6) {
        const float f = key2f(keys[threadIdx.x]);
        ((float *)keys)[threadIdx.x] = f;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void pack_positions_kernel(const T *__restrict__ v, int64_t nv, float *__restrict__ pos, u32 *keys)
{
    u32 mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < nv; i += (int64_t)gridDim.x * BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float x = (float)v[3 * i + c];
            pos[3 * i + c] = x;
            const u32 k = f2key(x);
            mn[c] = k < mn[c] ? k : mn[c];
            mx[c] = k > mx[c] ? k : mx[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u32 a = __shfl_xor(mn[c], d, 64), b = __shfl_xor(mx[c], d, 64);
            mn[c] = a < mn[c] ? a : mn[c];
            mx[c] = b > mx[c] ? b : mx[c];
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&keys[c], mn[c]);
            atomicMax(&keys[3 + c], mx[c]);
        }
    }
}

// ---- vertex normals (the normals contract in include/tomo_hip.h) ----------------------------------------------------------
// An inverted index instead of float atomics: per vertex the list of the faces that name it (one entry per corner), built
// with integer atomics in whatever order the corners arrive, then put into ascending order by the kernel that sums -- so
// the float64 sums do not depend on the schedule.  A face with an index outside [0, nv) enters no list and is counted.
// Multi-rank form: the kernel that sums takes a vertex range [vb, nv), starts the first n_seed vertices from given sums
// instead of +0.0 and leaves the vertices from raw_base on as raw float64 sums (not normalised, not counted).
constexpr int NRM_REG = 16;            // lists up to this length are sorted in registers (a marching-cubes vertex has 4-9 faces)

template <typename I>
__device__ static inline bool face_corners(const I *__restrict__ idx, int64_t f, int64_t nv, u64 c[3])
{
    c[0] = (u64)idx[3 * f];
    c[1] = (u64)idx[3 * f + 1];
    c[2] = (u64)idx[3 * f + 2];
    return c[0] < (u64)nv && c[1] < (u64)nv && c[2] < (u64)nv;          // a negative int64 is a huge u64
}

template <typename I>
__global__ __launch_bounds__(BLOCK) void normals_count_kernel(const I *__restrict__ idx, int64_t nf, int64_t nv, u32 *__restrict__ deg,
                                                               unsigned long long *__restrict__ counters)
{
    u32 bad = 0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        u64 c[3];
        if (!face_corners(idx, f, nv, c)) { bad++; continue; }
#pragma unroll
        for (int k = 0; k < 3; k++) atomicAdd(&deg[c[k]], 1u);
    }
    wave_add(&counters[1], bad);
}

// deg counts down to zero: the slot of a corner is off[v] + (what is left of deg[v]) - 1
template <typename I>
__global__ __launch_bounds__(BLOCK) void normals_fill_kernel(const I *__restrict__ idx, int64_t nf, int64_t nv, u32 *__restrict__ deg,
                                                              const u32 *__restrict__ off, u32 *__restrict__ list)
{
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < nf; f += (int64_t)gridDim.x * BLOCK) {
        u64 c[3];
        if (!face_corners(idx, f, nv, c)) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) list[off[c[k]] + (atomicSub(&deg[c[k]], 1u) - 1u)] = (u32)f;
    }
}

// rule 1 of the contract: float64 from the float32 positions, no fused multiply-add (the build passes -ffp-contract=off)
template <typename I>
__device__ static inline void face_vector(const float *__restrict__ pos, const I *__restrict__ idx, u32 f, double g[3])
{
    const float *p0 = pos + 3 * (int64_t)idx[3 * (int64_t)f], *p1 = pos + 3 * (int64_t)idx[3 * (int64_t)f + 1],
                *p2 = pos + 3 * (int64_t)idx[3 * (int64_t)f + 2];
    const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
    const double wx = (double)p2[0] - (double)p0[0], wy = (double)p2[1] - (double)p0[1], wz = (double)p2[2] - (double)p0[2];
    g[0] = uy * wz - uz * wy;
    g[1] = uz * wx - ux * wz;
    g[2] = ux * wy - uy * wx;
}

// One lane per vertex.  A list of at most NRM_REG entries is sorted in registers (odd-even transposition, padded with
// 0xffffffff: a face number is below 2^32 / 3) and summed by its lane.  Longer lists are taken one at a time by the whole
// wave: each step finds the smallest face number above the last one summed and how often it occurs (a face that names the
// vertex twice has two entries), so the order is exact for any length without memory for a sorted copy.
template <typename I>
__global__ __launch_bounds__(BLOCK) void vertex_normals_kernel(const float *__restrict__ pos, int64_t vb, int64_t nv,
                                                                const I *__restrict__ idx, const u32 *__restrict__ off,
                                                                const u32 *__restrict__ list, float *__restrict__ normals,
                                                                unsigned long long *__restrict__ counters,
                                                                const double *__restrict__ seed, int64_t n_seed,
                                                                double *__restrict__ raw, int64_t raw_base)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * (BLOCK / 64);
    u32 defaulted = 0;
    for (int64_t base = vb + wave * 64; base < nv; base += nwaves * 64) {
        const int64_t v = base + lane;
        u32 o = 0, d = 0;
        double s[3] = {0.0, 0.0, 0.0};
        if (v < nv) {
            o = off[v];
            d = off[v + 1] - o;
            if (v < n_seed) {                                           // the sums of the faces a lower rank holds come first
                s[0] = seed[3 * v];
                s[1] = seed[3 * v + 1];
                s[2] = seed[3 * v + 2];
            }
        }
        if (d <= NRM_REG) {
            u32 key[NRM_REG];
#pragma unroll
            for (int k = 0; k < NRM_REG; k++) key[k] = (u32)k < d ? list[o + k] : 0xffffffffu;
#pragma unroll
            for (int r = 0; r < NRM_REG; r++) {
#pragma unroll
                for (int i = r & 1; i + 1 < NRM_REG; i += 2) {
                    const u32 a = key[i], b = key[i + 1];
                    key[i] = a < b ? a : b;
                    key[i + 1] = a < b ? b : a;
                }
            }
#pragma unroll
            for (int k = 0; k < NRM_REG; k++) {
                if ((u32)k < d) {
                    double g[3];
                    face_vector(pos, idx, key[k], g);
                    s[0] += g[0];
                    s[1] += g[1];
                    s[2] += g[2];
                }
            }
        }
        u64 longer = __ballot(d > NRM_REG);
        while (longer) {
            const int src = __ffsll((long long)longer) - 1;
            longer &= longer - 1;
            const u32 lo = __shfl(o, src, 64), ld = __shfl(d, src, 64);
            double t[3] = {__shfl(s[0], src, 64), __shfl(s[1], src, 64), __shfl(s[2], src, 64)};     // +0.0 or the seed
            int64_t last = -1;
            for (u32 done = 0; done < ld;) {
                u32 m = 0xffffffffu, c = 0;
                for (u32 k = lane; k < ld; k += 64) {
                    const u32 f = list[lo + k];
                    if ((int64_t)f <= last) continue;
                    if (f < m) { m = f; c = 1; }
                    else if (f == m) c++;
                }
                u32 best = m;
#pragma unroll
                for (int w = 32; w > 0; w >>= 1) {
                    const u32 x = __shfl_xor(best, w, 64);
                    best = x < best ? x : best;
                }
                const u32 times = wave_sum(m == best ? c : 0u);
                if (best == 0xffffffffu || times == 0) break;          // cannot happen with the lists the fill kernel wrote
                double g[3];
                face_vector(pos, idx, best, g);
                for (u32 j = 0; j < times; j++) {
                    t[0] += g[0];
                    t[1] += g[1];
                    t[2] += g[2];
                }
                last = (int64_t)best;
                done += times;
            }
            if (lane == src) {
                s[0] = t[0];
                s[1] = t[1];
                s[2] = t[2];
            }
        }
        if (v < nv && v >= raw_base) {                                  // a ghost row: its owner continues the sum
            raw[3 * (v - raw_base)] = s[0];
            raw[3 * (v - raw_base) + 1] = s[1];
            raw[3 * (v - raw_base) + 2] = s[2];
        } else if (v < nv) {
            const double q = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
            float n[3] = {0.0f, 0.0f, 1.0f};
            if (q > 0.0 && q < (double)INFINITY) {                      // finite and positive (a NaN fails both)
                const double r = sqrt(q);
                n[0] = (float)(s[0] / r);
                n[1] = (float)(s[1] / r);
                n[2] = (float)(s[2] / r);
            } else {
                defaulted++;
            }
            normals[3 * v] = n[0];
            normals[3 * v + 1] = n[1];
            normals[3 * v + 2] = n[2];
        }
    }
    wave_add(&counters[0], defaulted);
}

// Workspace of the normals: deg u32[nv] | off u32[nv + 1] | list u32[3 nf] | totals u64[4] | scan workspace, each part on
// a 256-byte boundary.
struct NormalsWs {
    int64_t off, list, totals, scan, scan_bytes, total;
};
static inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }
static inline NormalsWs normals_ws(int64_t nv, int64_t nf)
{
    NormalsWs w;
    w.off = up256(4 * nv);
    w.list = w.off + up256(4 * (nv + 1));
    w.totals = w.list + up256(12 * nf);
    w.scan = w.totals + 256;
    w.scan_bytes = tomo_mc_scan_workspace_bytes(nv);
    w.total = w.scan + up256(w.scan_bytes);
    return w;
}
static inline bool normals_sizes_ok(int64_t nv, int64_t nf) { return nv < (int64_t)0xffffffffLL && 3 * nf < ((int64_t)1 << 32); }

}  // namespace

TOMO_API int64_t tomo_mesh_vertex_normals_workspace_bytes(int64_t nv, int64_t nf)
{
    if (nv <= 0 || nf <= 0) return TOMO_E_ARG;
    if (!normals_sizes_ok(nv, nf)) return TOMO_E_SIZE;
    return normals_ws(nv, nf).total;
}

// phase bit 0: build the lists (and zero the counters), then the raw sums of the last n_raw vertices; bit 1: the normals of
// the first nv - n_raw vertices, the first n_seed of them continued from `seed`.
static int normals_run(const float *pos, int64_t nv, const void *idx, int idx_i64, int64_t nf, void *workspace, float *normals,
                       unsigned long long *counters, const double *seed, int64_t n_seed, double *raw, int64_t n_raw, int phase,
                       hipStream_t st)
{
    const NormalsWs w = normals_ws(nv, nf);
    char *base = (char *)workspace;
    u32 *deg = (u32 *)base, *off = (u32 *)(base + w.off), *list = (u32 *)(base + w.list);
    const unsigned gf = grid_for(nf);
    const int64_t own = nv - n_raw;
    if (phase & 1) {
        if (hipMemsetAsync(deg, 0, 4 * nv, st) != hipSuccess || hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), st) != hipSuccess)
            return TOMO_E_LAUNCH;
        if (nf > 0) {
            if (idx_i64)
                hipLaunchKernelGGL(normals_count_kernel<int64_t>, dim3(gf), dim3(BLOCK), 0, st, (const int64_t *)idx, nf, nv, deg, counters);
            else
                hipLaunchKernelGGL(normals_count_kernel<uint32_t>, dim3(gf), dim3(BLOCK), 0, st, (const uint32_t *)idx, nf, nv, deg, counters);
        }
        const int rc = tomo_mc_scan(deg, nv, off, nullptr, (unsigned long long *)(base + w.totals), base + w.scan, w.scan_bytes, st);
        if (rc != TOMO_OK) return rc;
        if (nf > 0) {
            if (idx_i64)
                hipLaunchKernelGGL(normals_fill_kernel<int64_t>, dim3(gf), dim3(BLOCK), 0, st, (const int64_t *)idx, nf, nv, deg, off, list);
            else
                hipLaunchKernelGGL(normals_fill_kernel<uint32_t>, dim3(gf), dim3(BLOCK), 0, st, (const uint32_t *)idx, nf, nv, deg, off, list);
        }
    }
    for (int part = 0; part < 2; part++) {                 // 0: the raw suffix [own, nv), 1: the normals of [0, own)
        if (!(phase & (1 << part))) continue;
        const int64_t vb = part == 0 ? own : 0, ve = part == 0 ? nv : own;
        if (ve <= vb) continue;
        const unsigned gv = grid_for(ve - vb);
        if (idx_i64)
            hipLaunchKernelGGL(vertex_normals_kernel<int64_t>, dim3(gv), dim3(BLOCK), 0, st, pos, vb, ve, (const int64_t *)idx, off, list,
                               normals, counters, seed, part == 1 ? n_seed : (int64_t)0, raw, part == 0 ? own : ve);
        else
            hipLaunchKernelGGL(vertex_normals_kernel<uint32_t>, dim3(gv), dim3(BLOCK), 0, st, pos, vb, ve, (const uint32_t *)idx, off, list,
                               normals, counters, seed, part == 1 ? n_seed : (int64_t)0, raw, part == 0 ? own : ve);
    }
    return tomo_status();
}

TOMO_API int tomo_mesh_vertex_normals(const float *pos, int64_t nv, const void *idx, int idx_i64, int64_t nf, void *workspace,
                                      int64_t workspace_bytes, float *normals, unsigned long long *counters, void *stream)
{
    if (!pos || !idx || !workspace || !normals || !counters || nv <= 0 || nf <= 0) return TOMO_E_ARG;
    if (((uintptr_t)pos & 3) || ((uintptr_t)normals & 3) || ((uintptr_t)idx & (idx_i64 ? 7 : 3)) || ((uintptr_t)workspace & 255) ||
        ((uintptr_t)counters & 7))
        return TOMO_E_ARG;
    if (!normals_sizes_ok(nv, nf)) return TOMO_E_SIZE;
    if (workspace_bytes < normals_ws(nv, nf).total) return TOMO_E_WORKSPACE;
    return normals_run(pos, nv, idx, idx_i64, nf, workspace, normals, counters, nullptr, 0, nullptr, 0, 3, (hipStream_t)stream);
}

TOMO_API int tomo_mesh_vertex_normals_seeded(const float *pos, int64_t nv, const void *idx, int idx_i64, int64_t nf, void *workspace,
                                             int64_t workspace_bytes, float *normals, unsigned long long *counters, const double *seed,
                                             int64_t n_seed, double *raw, int64_t n_raw, int phase, void *stream)
{
    if (!pos || !workspace || !counters || nv <= 0 || nf < 0 || n_seed < 0 || n_raw < 0 || phase < 1 || phase > 3) return TOMO_E_ARG;
    if (n_raw > nv || n_seed > nv - n_raw || (nf > 0 && !idx) || (n_seed > 0 && !seed) || (n_raw > 0 && !raw)) return TOMO_E_ARG;
    if ((phase & 2) && nv - n_raw > 0 && !normals) return TOMO_E_ARG;
    if (((uintptr_t)pos & 3) || ((uintptr_t)normals & 3) || ((uintptr_t)idx & (idx_i64 ? 7 : 3)) || ((uintptr_t)workspace & 255) ||
        ((uintptr_t)counters & 7) || ((uintptr_t)seed & 7) || ((uintptr_t)raw & 7))
        return TOMO_E_ARG;
    if (!normals_sizes_ok(nv, nf)) return TOMO_E_SIZE;
    if (workspace_bytes < normals_ws(nv, nf).total) return TOMO_E_WORKSPACE;
    return normals_run(pos, nv, idx, idx_i64, nf, workspace, normals, counters, seed, n_seed, raw, n_raw, phase, (hipStream_t)stream);
}

TOMO_API int tomo_layer_colors(const void *verts, int is_f64, int64_t nv, int64_t stride, double start1, double end1, int enable1,
                               double start2, double end2, int enable2, uint8_t *rgba, void *stream)
{
    if (nv < 0 || stride < 1) return TOMO_E_ARG;
    if (nv == 0) return TOMO_OK;
    if (!verts || !rgba || ((uintptr_t)rgba & 3)) return TOMO_E_ARG;
    const unsigned g = grid_for(nv);
    if (is_f64)
        hipLaunchKernelGGL(layer_colors_kernel<double>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, (const double *)verts, nv, stride,
                           start1, end1, enable1, start2, end2, enable2, (u32 *)rgba);
    else
        hipLaunchKernelGGL(layer_colors_kernel<float>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, (const float *)verts, nv, stride,
                           start1, end1, enable1, start2, end2, enable2, (u32 *)rgba);
    return tomo_status();
}

TOMO_API int64_t tomo_mesh_edge_table_bytes(int64_t nf)
{
    if (nf < 0 || nf >= (int64_t)1 << 31) return TOMO_E_SIZE;
    return table_bytes(nf);
}

TOMO_API int tomo_mesh_edges(const int64_t *faces, int64_t nf, int64_t nv, void *table, int64_t bytes, unsigned long long *counters,
                             void *stream)
{
    if (!faces || !table || !counters || nf <= 0 || nv <= 0) return TOMO_E_ARG;
    if (nf >= (int64_t)1 << 31 || nv > (int64_t)0xffffffffLL) return TOMO_E_SIZE;
    const int64_t cap = table_cap(nf);
    if (bytes < table_bytes(nf)) return TOMO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Table t = table_view(table, cap);
    if (hipMemsetAsync(t.keys, 0xff, 8 * cap, st) != hipSuccess || hipMemsetAsync(t.cnt, 0, 4 * cap, st) != hipSuccess ||
        hipMemsetAsync(counters, 0, 6 * sizeof(unsigned long long), st) != hipSuccess)
        return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(edge_insert_kernel, dim3(grid_for(nf)), dim3(BLOCK), 0, st, faces, nf, nv, t, counters);
    hipLaunchKernelGGL(edge_classify_kernel, dim3(grid_for(cap)), dim3(BLOCK), 0, st, t, counters);
    return tomo_status();
}

TOMO_API int tomo_mesh_seam_edges(const void *table, int64_t bytes, int64_t nf, int64_t first_ghost, unsigned long long *msg, int64_t cap,
                                  unsigned long long *count, void *stream)
{
    if (!table || !count || nf <= 0 || first_ghost < 0 || cap < 0 || (cap > 0 && !msg)) return TOMO_E_ARG;
    if (((uintptr_t)msg & 7) || ((uintptr_t)count & 7)) return TOMO_E_ARG;
    if (nf >= (int64_t)1 << 31 || first_ghost > (int64_t)0xffffffffLL) return TOMO_E_SIZE;
    if (bytes < table_bytes(nf)) return TOMO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t cap_t = table_cap(nf);
    if (hipMemsetAsync(count, 0, sizeof(unsigned long long), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(seam_collect_kernel, dim3(grid_for(cap_t)), dim3(BLOCK), 0, st, table_view((void *)table, cap_t), (u64)first_ghost, cap,
                       (u64 *)msg, count);
    return tomo_status();
}

TOMO_API int tomo_mesh_seam_merge(const void *table, int64_t bytes, int64_t nf, const unsigned long long *msg, int64_t n, int64_t *corr,
                                  void *stream)
{
    if (!table || !corr || nf <= 0 || n < 0 || (n > 0 && !msg)) return TOMO_E_ARG;
    if (((uintptr_t)msg & 7) || ((uintptr_t)corr & 7)) return TOMO_E_ARG;
    if (nf >= (int64_t)1 << 31) return TOMO_E_SIZE;
    if (bytes < table_bytes(nf)) return TOMO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(corr, 0, 4 * sizeof(int64_t), st) != hipSuccess) return TOMO_E_LAUNCH;
    if (n == 0) return TOMO_OK;
    hipLaunchKernelGGL(seam_merge_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, st, table_view((void *)table, table_cap(nf)), (const u64 *)msg, n,
                       (unsigned long long *)corr);
    return tomo_status();
}

TOMO_API int64_t tomo_mesh_orient_workspace_bytes(int64_t nf)
{
    if (nf < 0 || nf >= (int64_t)1 << 31) return TOMO_E_SIZE;
    return nf * (8 + 4 + 4);
}

TOMO_API int tomo_mesh_orient(const void *table, int64_t bytes, int64_t nf, void *workspace, int64_t workspace_bytes, uint8_t *flip,
                              unsigned long long *counts, void *stream)
{
    if (!table || !workspace || !flip || !counts || nf <= 0) return TOMO_E_ARG;
    if (nf >= (int64_t)1 << 31) return TOMO_E_SIZE;
    const int64_t cap = table_cap(nf);
    if (bytes < table_bytes(nf) || workspace_bytes < tomo_mesh_orient_workspace_bytes(nf)) return TOMO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Table t = table_view((void *)table, cap);
    u64 *uf = (u64 *)workspace;
    u32 *root = (u32 *)((char *)workspace + 8 * nf);
    u32 *conflict = root + nf;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), st) != hipSuccess) return TOMO_E_LAUNCH;
    hipLaunchKernelGGL(uf_init_kernel, dim3(grid_for(nf)), dim3(BLOCK), 0, st, uf, conflict, nf);
    hipLaunchKernelGGL(uf_union_kernel, dim3(grid_for(cap)), dim3(BLOCK), 0, st, t, uf);
    hipLaunchKernelGGL(uf_resolve_kernel, dim3(grid_for(nf)), dim3(BLOCK), 0, st, uf, nf, root, flip, counts);
    hipLaunchKernelGGL(uf_verify_kernel, dim3(grid_for(cap)), dim3(BLOCK), 0, st, t, root, flip, conflict);
    hipLaunchKernelGGL(uf_conflict_kernel, dim3(grid_for(nf)), dim3(BLOCK), 0, st, nf, root, conflict, flip, counts);
    return tomo_status();
}

TOMO_API int tomo_mesh_signed_volume(const float *verts, const int64_t *faces, int64_t nf, const uint8_t *flip, double *out, void *stream)
{
    if (!verts || !faces || !out || nf < 0) return TOMO_E_ARG;
    if (nf == 0) return TOMO_OK;
    hipLaunchKernelGGL(signed_volume_kernel, dim3(grid_for(nf, 1024)), dim3(BLOCK), 0, (hipStream_t)stream, verts, faces, nf, flip, out);
    return tomo_status();
}

TOMO_API int tomo_glb_pack_faces(const int64_t *faces, int64_t nf, const uint8_t *flip, const double *volume, void *out, int out_i64,
                                 void *stream)
{
    if (!faces || !out || nf < 0) return TOMO_E_ARG;
    if (nf == 0) return TOMO_OK;
    if ((uintptr_t)out & (out_i64 ? 7 : 3)) return TOMO_E_ARG;
    const unsigned g = grid_for(nf);
    if (out_i64)
        hipLaunchKernelGGL(pack_faces_kernel<int64_t>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, faces, nf, flip, volume, (int64_t *)out);
    else
        hipLaunchKernelGGL(pack_faces_kernel<uint32_t>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, faces, nf, flip, volume, (uint32_t *)out);
    return tomo_status();
}

TOMO_API int tomo_glb_pack_positions(const void *verts, int is_f64, int64_t nv, float *pos, float *minmax, void *stream)
{
    if (!verts || !pos || !minmax || nv <= 0 || ((uintptr_t)pos & 3) || ((uintptr_t)minmax & 3)) return TOMO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    u32 *keys = (u32 *)minmax;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(64), 0, st, keys);
    const unsigned g = grid_for(nv, 1024);
    if (is_f64)
        hipLaunchKernelGGL(pack_positions_kernel<double>, dim3(g), dim3(BLOCK), 0, st, (const double *)verts, nv, pos, keys);
    else
        hipLaunchKernelGGL(pack_positions_kernel<float>, dim3(g), dim3(BLOCK), 0, st, (const float *)verts, nv, pos, keys);
    hipLaunchKernelGGL(minmax_decode_kernel, dim3(1), dim3(64), 0, st, keys);
    return tomo_status();
}
