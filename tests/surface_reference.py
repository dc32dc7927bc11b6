"""Host reference for the Crofton surface area (pipeline.surface_area / component_surface): the definition, literally, in
NumPy / SciPy -- for small dense arrays.

Coordinates, spacing and background are those of the distance transform: pixel sizes mm_x, mm_y, slice depths d[k], everything
outside the stack is background (the mask is padded by one voxel), the virtual slices -1 and nz are as deep as the edge slice
next to them.

counts():   for a set voxel p of `mask` in slice k and each of its 26 neighbours q that is clear in `occupied` (the whole
            volume; the mask itself by default) or outside the stack, one count in n[k][c].  The column c follows (|dz|, |dy|,
            |dx|) of q - p and the sign of dz: 0, 1, 2 = x, y, xy in the slice; 3 .. 6 = z, xz, yz, xyz towards slice k + 1;
            7 .. 10 = the same towards slice k - 1 -> int64 (nz, 11).
weights():  per class x, y, xy, z, xz, yz, xyz twice the share of the unit sphere in the Voronoi cell of the class's normalised
            lattice direction among the 26 of the box (h, mm_y, mm_x): scipy.spatial.SphericalVoronoi.calculate_areas() / 2 pi.
            directions = 3: thirds for x, y and z.
factors():  F[k][c] = 2 w_c (mm_x mm_y h) / L, h = d[k] in the slice, (d[k] + d[k + 1]) / 2 upwards, (d[k - 1] + d[k]) / 2
            downwards, L the length of the class's lattice step -> float64 (nz, 11).
area():     the sequential float64 sum over k ascending and c = 0 .. 10 of n[k][c] * F[k][c]."""
import math

import numpy as np

CLASSES = ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))      # (|dz|, |dy|, |dx|): x y xy z xz yz xyz
MULTIPLICITY = (1, 1, 2, 1, 2, 2, 4)                              # directions (pairs of opposite steps) per class: 13 in all
STEPS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dz or dy or dx]
CUBIC = (0.09155578240952, 0.07396125575216, 0.07039127956464)   # Ohser & Muecklich: axes, face diagonals, cube diagonals


def column(dz, dy, dx):
    cls = CLASSES.index((abs(dz), abs(dy), abs(dx)))
    return cls + 4 if dz < 0 else cls


def fold(n):
    """(.., 11) counters -> (.., 7): up and down folded into the class."""
    n = np.asarray(n, dtype=np.int64)
    out = n[..., :7].copy()
    out[..., 3:7] += n[..., 7:11]
    return out


def counts(mask, occupied=None):
    mask = np.asarray(mask) != 0
    occupied = mask if occupied is None else np.asarray(occupied) != 0
    nz, ny, nx = mask.shape
    clear = ~np.pad(occupied, 1)
    out = np.zeros((nz, 11), dtype=np.int64)
    for dz, dy, dx in STEPS:
        q = clear[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        out[:, column(dz, dy, dx)] += np.count_nonzero(mask & q, axis=(1, 2))
    return out


def component_counts(labels, n, occupied=None):
    """counts() of every mask `labels == c` against the whole volume at once -> int64 (n, nz, 11)."""
    labels = np.asarray(labels)
    occupied = labels != 0 if occupied is None else np.asarray(occupied) != 0
    nz, ny, nx = labels.shape
    clear = ~np.pad(occupied, 1)
    out = np.zeros((n, nz, 11), dtype=np.int64)
    for dz, dy, dx in STEPS:
        hit = (labels != 0) & clear[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        z = np.nonzero(hit)[0]
        np.add.at(out[:, :, column(dz, dy, dx)], (labels[hit].astype(np.int64) - 1, z), 1)
    return out


_weights = {}


def weights(mm_x, mm_y, h, directions=13):
    key = (float(mm_x), float(mm_y), float(h), directions)
    if key not in _weights:
        _weights[key] = _weights_of(*key)
    return _weights[key].copy()


def _weights_of(mm_x, mm_y, h, directions):
    if directions == 3:
        return np.array([1, 1, 0, 1, 0, 0, 0], dtype=np.float64) / 3.0
    from scipy.spatial import SphericalVoronoi
    units = np.array(STEPS, dtype=np.float64) * np.array([h, mm_y, mm_x], dtype=np.float64)
    units /= np.linalg.norm(units, axis=1)[:, None]
    areas = SphericalVoronoi(units).calculate_areas()
    return np.array([areas[STEPS.index(c)] for c in CLASSES]) / (2.0 * math.pi)


def depths_of(slice_depths, nz):
    return np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)


def factors(slice_depths, nz, mm_y, mm_x, directions=13):
    d = depths_of(slice_depths, nz)
    assert len(d) == nz
    d = np.concatenate([d[:1], d, d[-1:]])
    F = np.zeros((nz, 11))
    for k in range(nz):
        for c in range(11):
            h = d[k + 1] if c < 3 else (d[k + 1] + d[k + 2]) / 2 if c < 7 else (d[k] + d[k + 1]) / 2
            cls = c if c < 7 else c - 4
            az, ay, ax = CLASSES[cls]
            L = math.sqrt((az * h) ** 2 + (ay * mm_y) ** 2 + (ax * mm_x) ** 2)
            F[k, c] = 2.0 * weights(mm_x, mm_y, h, directions)[cls] * (mm_x * mm_y * h) / L
    return F


def area(n, F):
    s = 0.0
    for k in range(len(n)):
        for c in range(11):
            s += float(n[k][c]) * float(F[k][c])
    return s


def surface_area(mask, slice_depths=None, mm_y=1.0, mm_x=1.0, directions=13, occupied=None):
    mask = np.asarray(mask)
    return area(counts(mask, occupied), factors(slice_depths, mask.shape[0], mm_y, mm_x, directions))


def slice_centres(slice_depths, nz):
    """The slice centres of pipeline.distance_positions: the running sum of the depths, minus half a depth."""
    d = depths_of(slice_depths, nz)
    return np.cumsum(d) - d / 2.0


def ball(R_mm, mm_x, mm_y, depths, ny, nx):
    """The voxels whose centres lie within R_mm of the centre of the stack, in the coordinates of distance_positions."""
    d = np.asarray(depths, dtype=np.float64)
    zc = slice_centres(d, len(d))
    z = zc - (zc[0] + zc[-1]) / 2.0
    y = (np.arange(ny) - (ny - 1) / 2.0) * mm_y
    x = (np.arange(nx) - (nx - 1) / 2.0) * mm_x
    return z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2 <= R_mm * R_mm


VARIABLE_DEPTHS = np.array([0.5] * 4 + [1.0] * 20 + [0.25] * 8)

# (R_mm, mm_x, mm_y, depths, ny, nx): the three balls of the tests, each inside its stack
BALLS = {"r16_unit": (16.0, 1.0, 1.0, np.ones(37), 37, 37),
         "r10_aniso": (10.0, 0.5, 0.75, np.ones(25), 31, 45),
         "r9_variable": (9.0, 1.0, 1.0, VARIABLE_DEPTHS, 23, 23)}
