"""Host reference for the geodesic distance and the geodesic length per component, in plain NumPy + heapq on top of
edt_reference, thickness_reference and components_reference (which it imports and leaves alone).

The metric (include/tomo_hip.h).  Voxel (k, j, i) sits at (zc[k], j mm_y, i mm_x), the inner entries of edt_reference.positions.
A step goes between two set voxels that are neighbours under the connectivity (6 or 26, no corner-cutting test); its weight is
float32(sqrt(((dx mm_x)^2 + (dy mm_y)^2) + dzc^2)) with the float64 dzc = zc[k + 1] - zc[k] between slices.  weights() builds the
two tables from the positions on its own; nothing here calls the product.

dijkstra(): multi-source, np.float32 additions left to right along the path, a binary heap.  bellman_ford(): the same fixed
point by raster and anti-raster sweeps in place until a pair of sweeps changes nothing -- another order of the same relaxations
(tests/test_geodesic_cpu.py holds the two to the same bytes: the property the tiled GPU kernel rests on).
reach(): the set voxels within a radius.  search(): the repeated farthest-point search per component, all components at once
(propagation stays inside a component), the lowest flat index among equals."""
import heapq
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import edt_reference as E  # noqa: E402
import thickness_reference as T  # noqa: E402

KINDS = ("unit", "sided", "dyadic")
CONNECTIVITIES = (6, 26)
F32 = np.float32
INF = np.float32(np.inf)


# ----------------------------------------------------------------------------- the weights
def weights_from(zt, mm_y, mm_x):
    """-> (wxy float32 (3,): x, y, xy; wz float32 (max(nz - 1, 1), 4): z, zx, zy, zyx across the boundary k | k + 1)."""
    zc = np.asarray(zt, dtype=np.float64)[1:-1]
    nz = len(zc)

    def w(dx, dy, dzc):
        return np.sqrt(((dx * mm_x) ** 2 + (dy * mm_y) ** 2) + dzc ** 2)

    wxy = np.array([w(1, 0, 0.0), w(0, 1, 0.0), w(1, 1, 0.0)], dtype=np.float64).astype(np.float32)
    wz = np.zeros((max(nz - 1, 1), 4), dtype=np.float32)
    for k in range(nz - 1):
        dzc = zc[k + 1] - zc[k]
        wz[k] = np.array([w(0, 0, dzc), w(1, 0, dzc), w(0, 1, dzc), w(1, 1, dzc)], dtype=np.float64).astype(np.float32)
    return wxy, wz


def weights(shape, kind):
    depths, mm_y, mm_x = T.spacing(kind, shape[0])
    zt, _, _ = E.positions(shape, depths, mm_y, mm_x)
    return weights_from(zt, float(mm_y), float(mm_x))


def offsets(connectivity):
    """All neighbour offsets (dz, dy, dx) of the connectivity."""
    if connectivity == 6:
        return [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]
    if connectivity == 26:
        return [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    raise ValueError("connectivity must be 6 or 26")


def step_weight(wxy, wz, k, off):
    """The float32 weight of the step `off` from a voxel of slice k."""
    dz, dy, dx = off
    if dz == 0:
        return wxy[2 if (dx and dy) else (1 if dy else 0)]
    return wz[min(k, k + dz), (1 if dx else 0) + (2 if dy else 0)]


def seeds_mask(shape, seeds):
    """seeds as a bool volume: a bool volume itself, or integer (n, 3) rows of (z, y, x)."""
    s = np.asarray(seeds)
    if s.dtype == bool and s.shape == tuple(shape):
        return s
    out = np.zeros(shape, dtype=bool)
    s = s.reshape(-1, 3)
    out[s[:, 0], s[:, 1], s[:, 2]] = True
    return out


# ----------------------------------------------------------------------------- the distance
def dijkstra(v, seeds, wxy, wz, connectivity=26):
    """float32 (nz, ny, nx): 0.0 at a set seed, the least float32 path sum at a set voxel a seed reaches, +inf elsewhere."""
    v = np.asarray(v) != 0
    nz, ny, nx = v.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = v
    py, pz = nx + 2, (ny + 2) * (nx + 2)
    mask = pad.reshape(-1).tolist()
    steps = []                                                   # per slice k: (flat offset, float32 weight)
    for k in range(nz):
        row = []
        for off in offsets(connectivity):
            if 0 <= k + off[0] < nz:
                row.append((off[0] * pz + off[1] * py + off[2], F32(step_weight(wxy, wz, k, off))))
        steps.append(row)
    dist = [INF] * len(mask)
    heap = []
    sm = np.zeros_like(pad)
    sm[1:-1, 1:-1, 1:-1] = seeds_mask(v.shape, seeds) & v
    for p in np.flatnonzero(sm.reshape(-1)).tolist():
        dist[p] = F32(0)
        heap.append((F32(0), p))
    heapq.heapify(heap)
    while heap:
        d, p = heapq.heappop(heap)
        if d > dist[p]:
            continue
        for off, w in steps[p // pz - 1]:
            q = p + off
            if mask[q]:
                nd = d + w                                       # np.float32 + np.float32: one rounded addition
                if nd < dist[q]:
                    dist[q] = nd
                    heapq.heappush(heap, (nd, q))
    out = np.array(dist, dtype=np.float32).reshape(pad.shape)[1:-1, 1:-1, 1:-1]
    return np.ascontiguousarray(out)


def bellman_ford(v, seeds, wxy, wz, connectivity=26, limit=100000):
    """The same map by in-place raster and anti-raster sweeps to a fixed point -> (map, sweeps)."""
    v = np.asarray(v) != 0
    nz, ny, nx = v.shape
    dist = np.full(v.shape, INF, dtype=np.float32)
    dist[seeds_mask(v.shape, seeds) & v] = 0
    cells = [tuple(int(a) for a in c) for c in np.argwhere(v)]
    offs = offsets(connectivity)
    for sweep in range(limit):
        changed = False
        for k, j, i in (cells if sweep % 2 == 0 else reversed(cells)):
            best = dist[k, j, i]
            for off in offs:
                a, b, c = k + off[0], j + off[1], i + off[2]
                if 0 <= a < nz and 0 <= b < ny and 0 <= c < nx and v[a, b, c]:
                    nd = dist[a, b, c] + F32(step_weight(wxy, wz, k, off))
                    if nd < best:
                        best = nd
            if best < dist[k, j, i]:
                dist[k, j, i] = best
                changed = True
        if not changed:
            return dist, sweep + 1
    raise AssertionError("no fixed point within the limit")


def reach(v, dist, max_mm=None):
    """The set voxels with a finite distance (max_mm None) or with dist <= max_mm."""
    v = np.asarray(v) != 0
    return v & (np.isfinite(dist) if max_mm is None else dist.astype(np.float64) <= float(max_mm))


# ----------------------------------------------------------------------------- the farthest-point search
def _farthest(labels, n, dist):
    """Per label 1 .. n: (float32 maximum of dist over the component, the lowest flat index that attains it)."""
    flat = np.flatnonzero(labels.reshape(-1))
    lab = labels.reshape(-1)[flat].astype(np.int64)
    bits = dist.reshape(-1)[flat].view(np.uint32).astype(np.int64)       # values >= 0: the bit order is the float order
    order = np.lexsort((flat, -bits, lab))
    first = order[np.searchsorted(lab[order], np.arange(1, n + 1))]
    return dist.reshape(-1)[flat[first]], flat[first]


def search(v, labels, n, selected, kind, connectivity, sweeps=3):
    """The repeated farthest-point search for the labels in `selected` (ascending) -> list of dicts; every other component
    stays at +inf.  a0 = the first voxel of the component in raster order; for s = 1 .. sweeps the map is propagated from
    a(s - 1) and a_s is the farthest voxel, the lowest flat index among equals."""
    v = np.asarray(v) != 0
    shape = v.shape
    wxy, wz = weights(shape, kind)
    depths, mm_y, mm_x = T.spacing(kind, shape[0])
    zt, yt, xt = E.positions(shape, depths, mm_y, mm_x)
    selected = np.asarray(selected, dtype=np.int64)
    if len(selected) == 0:
        return [], np.full(shape, INF, dtype=np.float32)
    _, a = _farthest(labels, n, np.zeros(shape, dtype=np.float32))      # the first voxel of every component
    dist = None
    for _ in range(sweeps):
        prev = a
        seeds = np.stack(np.unravel_index(prev[selected - 1], shape), axis=1)
        dist = dijkstra(v, seeds, wxy, wz, connectivity)
        far, a = _farthest(labels, n, dist)
    sizes = C.sizes(labels, n)
    rows = []
    for c in selected:
        ends = [tuple(int(t) for t in np.unravel_index(int(p[c - 1]), shape)) for p in (prev, a)]
        mm = [(float(zt[k + 1]), float(yt[j + 1]), float(xt[i + 1])) for k, j, i in ends]
        d = [mm[1][t] - mm[0][t] for t in range(3)]
        chord = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        length = float(far[c - 1])
        rows.append({"label": int(c), "voxels": int(sizes[c - 1]), "length_mm": length, "ends_index": ends, "ends_mm": mm,
                     "chord_mm": chord, "tortuosity": length / chord if chord > 0 else 1.0})
    return rows, dist


def select_labels(labels, n, min_voxels=0, largest=False):
    """The keep rule -> the selected labels, ascending."""
    sz = C.sizes(labels, n)
    keep = np.flatnonzero(sz >= min_voxels) + 1
    if largest and len(keep):
        keep = keep[[int(np.argmax(sz[keep - 1]))]]               # the first maximum: the lowest label among equals
    return keep


def per_component(v, connectivity, kind, sweeps=3, min_voxels=0, largest=False):
    labels, n = C.label(v, connectivity)
    return search(v, labels, n, select_labels(labels, n, min_voxels, largest), kind, connectivity, sweeps)


def enclosed(v, connectivity, kind, sweeps=3, min_voxels=0):
    """The rows of the cavities of v: the search on the complement under 32 - connectivity, for its components of at least
    min_voxels voxels whose index box touches no face of the stack."""
    outside = ~(np.asarray(v) != 0)
    conn = 32 - connectivity
    labels, n = C.label(outside, conn)
    sz = C.sizes(labels, n)
    keep = []
    for c in range(1, n + 1):
        idx = np.nonzero(labels == c)
        if sz[c - 1] >= min_voxels and all(a.min() > 0 and a.max() < s - 1 for a, s in zip(idx, outside.shape)):
            keep.append(c)
    return search(outside, labels, n, keep, kind, conn, sweeps)


# ----------------------------------------------------------------------------- the volumes of the tests
def _trace(shape, points):
    """A 6-connected one-voxel path through the integer points, axis by axis (z, then y, then x) between neighbours."""
    v = np.zeros(shape, dtype=bool)
    cur = list(points[0])
    v[tuple(cur)] = True
    for p in points[1:]:
        for axis in range(3):
            while cur[axis] != p[axis]:
                cur[axis] += 1 if p[axis] > cur[axis] else -1
                v[tuple(cur)] = True
    return v


def weave():
    """(2, 20, 130): one thin path that crosses the tile face y = 7 | 8 sixty-five times (a square wave along x in rows 6 .. 9),
    the face x = 63 | 64 five more times (a square wave along y in columns 62 .. 65) and hops between the two slices along
    row 2: every crossing costs the tiled kernel a sweep."""
    pts = [(0, 2, 0), (0, 6, 0)]
    for x in range(0, 130, 2):                                   # bars at even x, joined at y = 9 and y = 6 in turn
        top = (x // 2) % 2 == 0
        pts += [(0, 9 if top else 6, x)]
        if x + 2 < 130:
            pts += [(0, 9 if top else 6, x + 2)]
    v = _trace((2, 20, 130), pts)
    pts = [(0, 9, 64), (0, 11, 64), (0, 11, 62)]
    for k, y in enumerate(range(11, 20, 2)):                     # bars at odd y from x = 62 to 65
        right = k % 2 == 0
        pts += [(0, y, 65 if right else 62)]
        if y + 2 < 20:
            pts += [(0, y + 2, 65 if right else 62)]
    v |= _trace((2, 20, 130), pts)
    for x in range(130):                                         # row 2: slice 0 at x % 4 in (0, 1, 3), slice 1 at (1, 2, 3)
        v[0, 2, x] = x % 4 != 2
        v[1, 2, x] = x % 4 != 0
    return v


def coil():
    """(12, 24, 70): a helix of four turns round the x axis, one voxel thin: far longer than it is wide."""
    t = np.linspace(0.0, 8.0 * np.pi, 2000)
    pts = np.stack([np.rint(5.5 + 4.0 * np.sin(t)), np.rint(12.0 + 9.0 * np.cos(t)), np.rint(2.0 + 66.0 * t / t[-1])], axis=1)
    return _trace((12, 24, 70), [tuple(int(a) for a in p) for p in pts])


def ring():
    """(3, 22, 75): a circle of radius 9 in the middle slice, across the word boundary at x = 64."""
    t = np.linspace(0.0, 2.0 * np.pi, 400)
    pts = np.stack([np.ones_like(t), np.rint(11.0 + 9.0 * np.sin(t)), np.rint(63.0 + 9.0 * np.cos(t))], axis=1)
    return _trace((3, 22, 75), [tuple(int(a) for a in p) for p in pts])


def rod(axis, length=11):
    shape = [3, 3, 3]
    shape[axis] = length + 2
    v = np.zeros(shape, dtype=bool)
    idx = [1, 1, 1]
    idx[axis] = slice(1, length + 1)
    v[tuple(idx)] = True
    return v


COMPONENT_FIXTURES = ("words_130", "one_voxel", "empty", "full", "corner", "serpentine", "snake3d", "comb", "tie", "noise_031")


def fixtures():
    """name -> bool volume, in a fixed order: components_reference's, two noise volumes that cross a tile boundary on every
    axis, and the thin paths."""
    out = dict(C.fixtures())
    rng = np.random.default_rng(31)
    out["noise_tiles"] = rng.random((9, 17, 65)) < 0.6           # tile boundaries at z = 8, y = 8 / 16, x = 64
    out["noise_words"] = rng.random((17, 9, 130)) < 0.6          # three words, ragged last word
    out["weave"] = weave()
    out["coil"] = coil()
    out["ring"] = ring()
    return out


def default_seeds(v, every=97):
    """A deterministic seed set for a fixture: every `every`-th set voxel in raster order, and some unset voxels that must be
    ignored -> int64 (n, 3)."""
    v = np.asarray(v) != 0
    on = np.argwhere(v)[::every]
    off = np.argwhere(~v)[::max(1, every * 3)][:5]
    return np.concatenate([on, off]).astype(np.int64).reshape(-1, 3)
