"""Host reference for the greyscale reconstruction by dilation inside a bool volume, the h-maxima, the regional and the
extended maxima, in plain NumPy on top of components_reference, geodesic_reference (offsets) and zones_reference (_shifted),
which it imports and leaves alone.  Nothing here calls the product.

The definitions (include/tomo_hip.h).  m' = min(marker, f); g is the least fixed point above m' of
g(p) = max(m'(p), min(f(p), max over the set neighbours q of g(q))); unset voxels take no part and read 0.0 in the result;
-0.0 is read as +0.0.  Two independent reconstructions: sweeps() applies the operator to the whole volume at once until
nothing changes (float comparisons of NumPy), flood() settles the voxels one by one from the highest value down, a widest-path
search on a heap (integer keys).  HMAX_h(f) = reconstruction of fl32(f - h) under f; RMAX(f) by the rule of the device --
reconstruction of the float just below f stays below f -- and, another way, by the plateau definition: plateau_maxima()."""
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import geodesic_reference as G  # noqa: E402
import zones_reference as Z  # noqa: E402

F32 = np.float32
NEG = F32(-np.inf)
KEY_ZERO = 1 << 31
PLATEAU_LEVELS = 512                  # up to so many distinct values the plateaus are labelled value by value


def canon(a):
    """float32, -0.0 read as +0.0."""
    a = np.asarray(a, dtype=F32)
    return np.where(a == 0, F32(0.0), a).astype(F32)


def keys(a):
    """The order-preserving uint32 key of the header as int64: 2^31 + magnitude, 2^31 - magnitude for a negative value."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    return np.where(b >> 31, KEY_ZERO - mag, KEY_ZERO + mag)


def values(k):
    k = np.asarray(k, dtype=np.int64)
    bits = np.where(k >= KEY_ZERO, k - KEY_ZERO, (1 << 31) | (KEY_ZERO - k))
    return bits.astype(np.uint32).view(F32)


def below(a):
    """The float just below every entry (below +-0.0 lies the smallest negative denormal); -inf stays."""
    return np.nextafter(canon(a), NEG).astype(F32)


def sweeps(v, mask, marker, connectivity=26, limit=100000):
    """-> (g float32, applications of the operator until nothing changed)."""
    v = np.asarray(v) != 0
    f = canon(mask)
    with np.errstate(invalid="ignore"):
        g = np.where(v, np.minimum(canon(marker), f), NEG).astype(F32)
    offs = G.offsets(connectivity)
    for n in range(1, limit + 1):
        reach = np.full(v.shape, NEG, dtype=F32)
        for off in offs:
            np.maximum(reach, Z._shifted(g, off, NEG), out=reach)          # g is -inf at unset voxels: they raise nothing
        new = np.where(v, np.maximum(g, np.minimum(f, reach)), NEG).astype(F32)
        if new.tobytes() == g.tobytes():
            return np.where(v, g, F32(0.0)).astype(F32), n
        g = new
    raise AssertionError("no fixed point within the limit")


def flood(v, mask, marker, connectivity=26):
    """The same fixed point, one voxel at a time: the highest unsettled value is final (nothing higher can still arrive), and
    it offers min(f(q), g(p)) to its set neighbours.  Integer keys, a padded flat volume -> g float32."""
    v = np.asarray(v) != 0
    nz, ny, nx = v.shape
    pv = np.pad(v, 1)
    kf = np.pad(keys(canon(mask)), 1)
    km = np.pad(np.minimum(keys(canon(marker)), keys(canon(mask))), 1)
    sy, sz = nx + 2, (ny + 2) * (nx + 2)
    steps = [(o[0] * sz + o[1] * sy + o[2]) for o in G.offsets(connectivity)]
    on = pv.reshape(-1).tolist()
    f = kf.reshape(-1).tolist()
    g = np.where(pv, km, 0).reshape(-1).tolist()
    heap = [(-g[p], p) for p in np.flatnonzero(pv.reshape(-1)).tolist()]
    heapq.heapify(heap)
    while heap:
        negk, p = heapq.heappop(heap)
        if -negk != g[p]:
            continue                                                       # raised since it was pushed
        gp = g[p]
        for s in steps:
            q = p + s
            if on[q]:
                c = gp if gp < f[q] else f[q]
                if c > g[q]:
                    g[q] = c
                    heapq.heappush(heap, (-c, q))
    out = np.array(g, dtype=np.int64).reshape(pv.shape)[1:-1, 1:-1, 1:-1]
    return np.where(v, values(np.where(v, out, KEY_ZERO)), F32(0.0)).astype(F32)


def reconstruct(v, mask, marker, connectivity=26):
    return sweeps(v, mask, marker, connectivity)[0]


def h_marker(values_, h):
    """fl32(f - fl32(h)): one float32 subtraction per voxel."""
    with np.errstate(invalid="ignore"):
        return (canon(values_) - F32(h)).astype(F32)


def h_maxima(v, values_, h, connectivity=26, how=reconstruct):
    return how(v, values_, h_marker(values_, h), connectivity)


def regional_maxima(v, values_, connectivity=26, how=reconstruct):
    """The device's rule: the set voxels whose reconstruction from the float just below stays below -> bool volume."""
    v = np.asarray(v) != 0
    f = canon(values_)
    g = how(v, f, below(f), connectivity)
    return v & (keys(g) < keys(f))


def extended_maxima(v, values_, h, connectivity=26, how=reconstruct):
    return regional_maxima(v, h_maxima(v, values_, h, connectivity, how), connectivity, how)


def plateaus(v, values_, connectivity=26):
    """-> int64 labels: two set voxels share a label when a path of set voxels of ONE value joins them; 0 at unset voxels.
    Few distinct values: components_reference.label value by value; many: the smallest flat index spreads over equal neighbours."""
    v = np.asarray(v) != 0
    f = canon(values_)
    lab = np.zeros(v.shape, dtype=np.int64)
    levels = np.unique(f[v])
    if len(levels) <= PLATEAU_LEVELS:
        base = 0
        for level in levels:
            part, n = C.label(v & (f == level), connectivity)
            lab = np.where(part > 0, part.astype(np.int64) + base, lab)
            base += n
        return lab
    lab = np.where(v, np.arange(1, v.size + 1, dtype=np.int64).reshape(v.shape), 0)
    k = np.where(v, keys(f), -1)
    while True:
        new = lab
        for off in G.offsets(connectivity):
            same = v & (Z._shifted(k, off, -1) == k)
            new = np.where(same, np.minimum(new, Z._shifted(lab, off, 0)), new)
        if np.array_equal(new, lab):
            return lab
        lab = new


def plateau_maxima(v, values_, connectivity=26):
    """The definition: a plateau is a regional maximum when no member has a higher set neighbour -> bool volume."""
    v = np.asarray(v) != 0
    f = canon(values_)
    lab = plateaus(v, f, connectivity)
    k = np.where(v, keys(f), -1)
    higher = np.zeros(v.shape, dtype=bool)
    for off in G.offsets(connectivity):
        higher |= v & (Z._shifted(k, off, -1) > k)
    bad = np.zeros(int(lab.max()) + 1, dtype=bool)
    bad[lab[higher]] = True
    return v & ~bad[lab]


# ----------------------------------------------------------------------------- the volumes and maps of the tests
SCENE_SHAPE = (20, 40, 70)
SCENE_BALLS = (((10, 10, 10), 8), ((10, 10, 23), 8), ((10, 30, 8), 4), ((10, 30, 14), 4), ((10, 30, 40), 4), ((10, 12, 50), 8))
SCENE_MARKERS = (2, 1, 2, 1)          # extended maxima per component in label order, h = 1
SHAPES = ((9, 17, 70), SCENE_SHAPE, (17, 24, 130))


def scene():
    """Six balls in four components: a large pair, a small pair, a small ball and a large one (centre (z, y, x), radius)."""
    z, y, x = np.indices(SCENE_SHAPE)
    v = np.zeros(SCENE_SHAPE, dtype=bool)
    for (cz, cy, cx), r in SCENE_BALLS:
        v |= (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    return v


def unit_distance(v):
    """The inside Euclidean distance under unit spacing, everything outside the stack background -> float32."""
    from scipy import ndimage
    return ndimage.distance_transform_edt(np.pad(np.asarray(v) != 0, 1))[1:-1, 1:-1, 1:-1].astype(F32)


def noise(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def level_map(shape, levels, seed, lo=0.0, step=1.0):
    """A random quantised map: `levels` values lo + step * i."""
    return (lo + step * np.random.default_rng(seed).integers(0, levels, shape)).astype(F32)


def float_map(shape, seed, signed=False):
    a = np.random.default_rng(seed).random(shape).astype(F32)
    return (a - F32(0.5)).astype(F32) if signed else a


def zero_map(shape, seed):
    """Values among -1, -0.0, +0.0, 1 and a negative denormal: the two zeros are one value, and the float below them exists."""
    pool = np.array([-1.0, -0.0, 0.0, 1.0, -1e-45], dtype=F32)
    return pool[np.random.default_rng(seed).integers(0, len(pool), shape)]


def corridor(shape=(17, 24, 130)):
    """A one-voxel-wide path that snakes through every tile of the volume -> (bool volume, the voxels of the path in order):
    along x in row y = 0 of a slice, two voxels up in y, back along x, ... every second row, then two slices on in z, every
    second slice, so that no two runs touch under the 26-adjacency."""
    nz, ny, nx = shape
    v = np.zeros(shape, dtype=bool)
    path = []
    forward_y = True
    forward_x = True
    for z in range(0, nz, 2):
        rows = list(range(0, ny, 2))
        if not forward_y:
            rows.reverse()
        for n, y in enumerate(rows):
            xs = range(nx) if forward_x else range(nx - 1, -1, -1)
            path.extend((z, y, x) for x in xs)
            forward_x = not forward_x
            if n + 1 < len(rows):                                          # the link to the next row, at the end just reached
                path.append((z, (y + rows[n + 1]) // 2, path[-1][2]))
        forward_y = not forward_y
        if z + 2 < nz:
            path.append((z + 1, path[-1][1], path[-1][2]))
    for p in path:
        v[p] = True
    return v, path


def pitted_capsule(seed, shape=(16, 16, 40), radius=6.3, share=0.03):
    """A capsule along x with random pits: `share` of its voxels cleared."""
    z, y, x = np.indices(shape)
    cz, cy = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    ax = np.clip(x, radius + 1, shape[2] - 2 - radius)
    v = (z - cz) ** 2 + (y - cy) ** 2 + (x - ax) ** 2 <= radius * radius
    return v & ~(np.random.default_rng(seed).random(shape) < share)
