"""NumPy reference of the chord tables (include/tomo_hip.h, "Chord lengths"): counts, border and sum_q per direction and length
for a bool volume, by running lengths carried from slab to slab along the leading axis of a direction -- no line is followed,
no index wraps: nothing of the kernel's walk is repeated here.  walk_points is the slow second opinion, a walk from every chord
start over a set of points; tests/test_chords_cpu.py holds the two against each other and against hand values."""
import itertools
import math

import numpy as np

FORWARD = tuple(s for s in itertools.product((-1, 0, 1), repeat=3) if s > (0, 0, 0))       # ascending (dz, dy, dx)
ONE = 1 << 16


def steps(slice_depths, nz, mm_y=1.0, mm_x=1.0):
    """float64 (nz, 13): the length of one step of each direction through a voxel of slice k, entry by entry."""
    d = [1.0] * nz if slice_depths is None else [float(x) for x in slice_depths]
    assert len(d) == nz
    return np.array([[math.sqrt(((dz * d[k]) ** 2 + (dy * float(mm_y)) ** 2) + (dx * float(mm_x)) ** 2) for dz, dy, dx in FORWARD]
                     for k in range(nz)], dtype=np.float64).reshape(nz, 13)


def steps_q(st):
    """int64: round(step * 65536), half to even (Python's round)."""
    return np.array([[int(round(float(x) * ONE)) for x in row] for row in st], dtype=np.int64).reshape(len(st), 13)


def _shifted(a, da, db):
    """out[j, i] = a[j - da, i - db] where that lies inside, 0 elsewhere -> (out, inside)."""
    A, B = a.shape
    out = np.zeros_like(a)
    inside = np.zeros(a.shape, dtype=bool)
    j0, j1 = max(0, da), min(A, A + da)
    i0, i1 = max(0, db), min(B, B + db)
    if j0 < j1 and i0 < i1:
        out[j0:j1, i0:i1] = a[j0 - da:j1 - da, i0 - db:i1 - db]
        inside[j0:j1, i0:i1] = True
    return out, inside


def tables(v, q):
    """(counts, border, sum_q), int64 (13, L + 1) each, L = max(v.shape), of the bool volume v under the fixed-point steps q
    int64 (nz, 13)."""
    v = np.asarray(v, dtype=bool)
    nz = v.shape[0]
    q = np.asarray(q, dtype=np.int64).reshape(nz, 13)
    L = max(v.shape)
    counts, border, sum_q = (np.zeros((13, L + 1), dtype=np.int64) for _ in range(3))
    for m, s in enumerate(FORWARD):
        lead = next(ax for ax in range(3) if s[ax])
        da, db = (s[ax] for ax in range(3) if ax != lead)
        w = np.moveaxis(v, lead, 0)
        qv = np.moveaxis(np.broadcast_to(q[:, m].reshape(nz, 1, 1), v.shape), lead, 0)
        T = w.shape[0]
        run = np.zeros(w.shape[1:], dtype=np.int64)          # voxels of the chord that ends here so far
        acc = np.zeros(w.shape[1:], dtype=np.int64)          # ... and their steps
        edge = np.zeros(w.shape[1:], dtype=bool)             # ... and whether its predecessor lies outside the stack
        for t in range(T):
            cur = w[t]
            prun, inside = _shifted(run, da, db)
            pacc, _ = _shifted(acc, da, db)
            pedge, _ = _shifted(edge, da, db)
            if t == 0:
                inside = np.zeros_like(inside)
            run = np.where(cur, prun + 1, 0)
            acc = np.where(cur, pacc + qv[t], 0)
            edge = cur & (~inside | pedge)
            if t + 1 < T:
                nxt, has = _shifted(w[t + 1], -da, -db)
            else:
                nxt, has = np.zeros_like(cur), np.zeros_like(cur)
            end = cur & ~nxt
            cut = edge | ~has
            n = run[end]
            counts[m] += np.bincount(n, minlength=L + 1)
            border[m] += np.bincount(n[cut[end]], minlength=L + 1)
            weights = acc[end]
            assert weights.sum() < 2 ** 52
            sum_q[m] += np.bincount(n, weights=weights.astype(np.float64), minlength=L + 1).astype(np.int64)
    return counts, border, sum_q


def walk_points(points, shape, q):
    """The same tables from a walk: `points` the set voxels (z, y, x), every other voxel of `shape` clear.  For every direction,
    from every set voxel whose predecessor is clear or outside, step until the successor is clear or outside.  q: int64
    (nz, 13), or rows of any exact Python numbers (fractions.Fraction: sum_q is then an object array of their sums)."""
    nz, ny, nx = shape
    exact = not isinstance(q, np.ndarray)
    q = [[x if exact else int(x) for x in row] for row in q]
    assert len(q) == nz and all(len(row) == 13 for row in q)
    pts = set((int(z), int(y), int(x)) for z, y, x in points)
    L = max(shape)
    counts, border = (np.zeros((13, L + 1), dtype=np.int64) for _ in range(2))
    sum_q = np.zeros((13, L + 1), dtype=object if exact else np.int64)

    def outside(p):
        return not (0 <= p[0] < nz and 0 <= p[1] < ny and 0 <= p[2] < nx)

    for m, (dz, dy, dx) in enumerate(FORWARD):
        for p in pts:
            before = (p[0] - dz, p[1] - dy, p[2] - dx)
            if before in pts:
                continue
            n, acc, cur = 0, 0, p
            while cur in pts:
                n += 1
                acc += q[cur[0]][m]
                cur = (cur[0] + dz, cur[1] + dy, cur[2] + dx)
            counts[m, n] += 1
            sum_q[m, n] += acc
            if outside(before) or outside(cur):
                border[m, n] += 1
    return counts, border, sum_q


def walk(v, q):
    """walk_points of a bool volume: the triple loop over every voxel and direction."""
    v = np.asarray(v, dtype=bool)
    return walk_points([(z, y, x) for z in range(v.shape[0]) for y in range(v.shape[1]) for x in range(v.shape[2]) if v[z, y, x]],
                       v.shape, q)


def noise(density, shape, seed):
    return np.random.default_rng(seed).random(shape) < density


def ellipsoid(shape, semi_axes):
    """The voxels whose centres lie in the axis-aligned ellipsoid with the semi-axes (a_z, a_y, a_x) round the centre of the box."""
    z, y, x = np.indices(shape).astype(np.float64)
    c = [(s - 1) / 2.0 for s in shape]
    return ((z - c[0]) / semi_axes[0]) ** 2 + ((y - c[1]) / semi_axes[1]) ** 2 + ((x - c[2]) / semi_axes[2]) ** 2 <= 1.0
