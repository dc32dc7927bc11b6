"""Host reference for the Crofton mean breadth (pipeline.mean_breadth / component_breadth): the definition, literally, in
NumPy / SciPy -- for small dense arrays.

Lattice and background are those of the distance transform: voxel (k, j, i) sits at (zc[k], j mm_y, i mm_x), everything outside
the stack is clear (the volume is padded by one voxel).

NORMALS:    the 13 Miller indices (a_z, a_y, a_x) in {-1, 0, 1}^3, first non-zero entry positive, ascending.
cells(m):   the cells of the section lattice of family m besides the vertex, as tuples of corner offsets from the anchor (the
            raster-first corner): edges (one offset) and faces (three offsets for a rectangle, two for a triangle), derived
            from m alone -- the axis steps and face diagonals perpendicular to m.  Every offset is a 26-neighbour offset and
            lexicographically positive; both are asserted.
chi():      per label c, slice k and column: the signed section Euler numbers of the cells anchored at the voxels of label c in
            slice k -> int64 (n, nz, 26).  Columns 0 .. 12: vertices - edges + faces of the cells whose corners all lie in
            slice k, per family; 13 .. 25: - edges + faces of the cells with a corner in slice k + 1.  The other corners of a
            cell only have to be set in `occupied` (the whole volume).
factors():  B[k][f] = c_m / |n|, n = (a_z / h, a_y / mm_y, a_x / mm_x), h = d[k] in the columns 0 .. 12 and (d[k] + d[k + 1]) / 2
            in 13 .. 25 (0.0 in the last slice and for (1, 0, 0)); c_m twice the share of the sphere in the Voronoi cell of
            n / |n| among the 26 normals: scipy.spatial.SphericalVoronoi.  directions = 3: thirds for the axis normals.
breadth():  the sequential float64 sum over k ascending and the columns 0 .. 25 of (double)chi[k][col] * B[k][col]."""
import itertools
import math

import numpy as np

NORMALS = tuple(m for m in itertools.product((-1, 0, 1), repeat=3) if m > (0, 0, 0))
AXES = tuple(NORMALS.index(m) for m in ((0, 0, 1), (0, 1, 0), (1, 0, 0)))
FORWARD = NORMALS                                                    # the 13 forward 26-neighbour offsets are the same tuples


def _add(a, b):
    return tuple(int(x + y) for x, y in zip(a, b))


def _sub(a, b):
    return tuple(int(x - y) for x, y in zip(a, b))


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def cells(m):
    """-> (edges, faces): lists of tuples of corner offsets besides the anchor (0, 0, 0)."""
    nonzero = [i for i in range(3) if m[i]]
    unit = [tuple(int(i == j) for j in range(3)) for i in range(3)]
    diagonals = [d for d in FORWARD if sum(map(abs, d)) == 2 and _dot(d, m) == 0]      # face diagonals in the plane
    if len(nonzero) == 1:
        u, v = [unit[i] for i in range(3) if not m[i]]
        edges, faces = [(u,), (v,)], [(u, v, _add(u, v))]
    elif len(nonzero) == 2:
        (u,) = [unit[i] for i in range(3) if not m[i]]
        (e,) = diagonals
        edges, faces = [(u,), (e,)], [(u, e, _add(u, e))]
    else:
        assert len(diagonals) == 3
        edges = [(d,) for d in diagonals]
        both = diagonals + [tuple(-x for x in d) for d in diagonals]
        faces = [(a, b) for a, b in itertools.combinations(diagonals, 2) if _sub(b, a) in both]
        assert len(faces) == 2
    for cell in edges + faces:
        for o in cell:
            assert max(map(abs, o)) <= 1 and o > (0, 0, 0), (m, cell)   # a 26-neighbour offset; the anchor is raster-first
            assert _dot(o, m) == 0, (m, cell)                           # ... in the plane
    return edges, faces


CELLS = tuple(cells(m) for m in NORMALS)


def _shifted(padded, o, shape):
    nz, ny, nx = shape
    return padded[1 + o[0]:1 + o[0] + nz, 1 + o[1]:1 + o[1] + ny, 1 + o[2]:1 + o[2] + nx]


def chi(labels, n, occupied=None):
    """int64 (n, nz, 26) of the label image `labels` (0: clear) against the whole volume."""
    labels = np.asarray(labels)
    occupied = labels != 0 if occupied is None else np.asarray(occupied) != 0
    shape = labels.shape
    pad = np.pad(occupied, 1)
    out = np.zeros((n, shape[0], 26), dtype=np.int64)
    own = labels != 0
    lab = labels[own].astype(np.int64) - 1
    z = np.nonzero(own)[0]
    for f in range(13):
        np.add.at(out[:, :, f], (lab, z), 1)                           # every vertex lies in its slice
        edges, faces = CELLS[f]
        for sign, group in ((-1, edges), (1, faces)):
            for cell in group:
                hit = own.copy()
                for o in cell:
                    hit &= _shifted(pad, o, shape)
                col = f + 13 if any(o[0] for o in cell) else f
                np.add.at(out[:, :, col], (labels[hit].astype(np.int64) - 1, np.nonzero(hit)[0]), sign)
    return out


def chi_whole(mask):
    """int64 (nz, 26) of the volume as one component."""
    mask = np.asarray(mask) != 0
    return chi(mask.astype(np.int64), 1)[0]


def section_euler(x):
    """(.., nz, 26) -> (.., 13): in and cross parts added over the slices."""
    x = np.asarray(x, dtype=np.int64)
    return x[..., :13].sum(axis=-2) + x[..., 13:].sum(axis=-2)


_weights = {}


def weights(mm_x, mm_y, h, directions=13):
    """c_m per family of NORMALS for the lattice (h, mm_y, mm_x) -> float64 (13,)."""
    key = (float(mm_x), float(mm_y), float(h), directions)
    if key not in _weights:
        if directions == 3:
            w = np.zeros(13)
            w[list(AXES)] = 1.0 / 3.0
        else:
            from scipy.spatial import SphericalVoronoi
            steps = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]
            units = np.array(steps, dtype=np.float64) / np.array([h, mm_y, mm_x], dtype=np.float64)
            units /= np.linalg.norm(units, axis=1)[:, None]
            areas = SphericalVoronoi(units).calculate_areas()
            w = np.array([areas[steps.index(m)] for m in NORMALS]) / (2.0 * math.pi)
        _weights[key] = w
    return _weights[key].copy()


def spacing(m, mm_x, mm_y, h):
    return 1.0 / math.sqrt((m[0] / h) ** 2 + (m[1] / mm_y) ** 2 + (m[2] / mm_x) ** 2)


def depths_of(slice_depths, nz):
    return np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)


def factors(slice_depths, nz, mm_y=1.0, mm_x=1.0, directions=13):
    d = depths_of(slice_depths, nz)
    assert len(d) == nz
    B = np.zeros((nz, 26))
    for k in range(nz):
        w = weights(mm_x, mm_y, d[k], directions)
        for f, m in enumerate(NORMALS):
            B[k, f] = w[f] * spacing(m, mm_x, mm_y, d[k])
        if k + 1 < nz:
            h = (d[k] + d[k + 1]) / 2
            w = weights(mm_x, mm_y, h, directions)
            for f, m in enumerate(NORMALS):
                if m != (1, 0, 0):
                    B[k, 13 + f] = w[f] * spacing(m, mm_x, mm_y, h)
    return B


def breadth(x, B, directions=13):
    """The sequential sum of one component's (nz, 26) integers; directions = 3: the columns of the axis normals only."""
    s = 0.0
    for k in range(len(x)):
        for col in range(26):
            if directions == 13 or col % 13 in AXES:
                s += float(int(x[k][col])) * float(B[k][col])
    return s


def mean_breadth(mask, slice_depths=None, mm_y=1.0, mm_x=1.0, directions=13):
    mask = np.asarray(mask)
    return breadth(chi_whole(mask), factors(slice_depths, mask.shape[0], mm_y, mm_x, directions), directions)


def one_lattice(mask, h=1.0, mm_y=1.0, mm_x=1.0, directions=13):
    """sum over m of c_m delta_m chi_m on ONE lattice of height h: what the per-slice rule must give for uniform depths."""
    e = section_euler(chi_whole(mask))
    w = weights(mm_x, mm_y, h, directions)
    return sum(w[f] * spacing(m, mm_x, mm_y, h) * int(e[f]) for f, m in enumerate(NORMALS))


def slice_centres(slice_depths, nz):
    d = depths_of(slice_depths, nz)
    return np.cumsum(d) - d / 2.0


def grid(depths, ny, nx, mm_y=1.0, mm_x=1.0):
    """Centred coordinates (z, y, x) in mm, broadcastable."""
    d = np.asarray(depths, dtype=np.float64)
    zc = slice_centres(d, len(d))
    z = zc - (zc[0] + zc[-1]) / 2.0
    y = (np.arange(ny) - (ny - 1) / 2.0) * mm_y
    x = (np.arange(nx) - (nx - 1) / 2.0) * mm_x
    return z[:, None, None], y[None, :, None], x[None, None, :]


def ball(R_mm, depths, ny, nx, mm_y=1.0, mm_x=1.0):
    z, y, x = grid(depths, ny, nx, mm_y, mm_x)
    return z ** 2 + y ** 2 + x ** 2 <= R_mm * R_mm


def torus(R, r, n):
    """A solid torus round the z axis in a unit lattice of (2 r + 3, n, n) voxels."""
    z, y, x = grid(np.ones(2 * int(r) + 3), n, n)
    return (np.sqrt(y ** 2 + x ** 2) - R) ** 2 + z ** 2 <= r * r
