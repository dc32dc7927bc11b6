"""NumPy reference of the two-point table (include/tomo_hip.h, "The two-point covariance"): pairs[hz][hy + Ry][hx + Rx] = the
voxel pairs a lag (hz, hy, hx) apart that are both set and both inside the stack, by shifted slices and np.count_nonzero -- no
words, no shifts of bits, no accumulators: nothing of the kernel is repeated here.  pairs_fft is the independent second method, the
zero-padded float64 autocorrelation, rounded; pairs_loop the slow third opinion, a loop over all pairs of set voxels.
tests/test_two_point_cpu.py holds the three against each other and against hand values."""
import itertools

import numpy as np

FORWARD = tuple(s for s in itertools.product((-1, 0, 1), repeat=3) if s > (0, 0, 0))       # ascending (dz, dy, dx)


def box(R):
    """max_lag -> (Rz, Ry, Rx)."""
    return (int(R),) * 3 if np.isscalar(R) else tuple(int(r) for r in R)


def _cut(n, h):
    """The slices of an axis of n entries at which p and p + h both lie inside -> (slice of p, slice of p + h), or None."""
    if abs(h) >= n:
        return None
    return (slice(0, n - h), slice(h, n)) if h >= 0 else (slice(-h, n), slice(0, n + h))


def pairs(v, Rz, Ry, Rx):
    """int64 (Rz + 1, 2 Ry + 1, 2 Rx + 1) of the bool volume v."""
    v = np.asarray(v, dtype=bool)
    out = np.zeros((Rz + 1, 2 * Ry + 1, 2 * Rx + 1), dtype=np.int64)
    for hz in range(Rz + 1):
        cz = _cut(v.shape[0], hz)
        for hy in range(-Ry, Ry + 1):
            cy = _cut(v.shape[1], hy)
            for hx in range(-Rx, Rx + 1):
                cx = _cut(v.shape[2], hx)
                if cz and cy and cx:
                    out[hz, hy + Ry, hx + Rx] = np.count_nonzero(v[cz[0], cy[0], cx[0]] & v[cz[1], cy[1], cx[1]])
    return out


def inside(shape, R):
    """P(h) int64 over the box: the voxel pairs of the stack a lag h apart, counted per axis."""
    Rz, Ry, Rx = box(R)
    nz, ny, nx = shape
    out = np.zeros((Rz + 1, 2 * Ry + 1, 2 * Rx + 1), dtype=np.int64)
    for hz in range(Rz + 1):
        for hy in range(-Ry, Ry + 1):
            for hx in range(-Rx, Rx + 1):
                out[hz, hy + Ry, hx + Rx] = max(0, nz - hz) * max(0, ny - abs(hy)) * max(0, nx - abs(hx))
    return out


def pairs_fft(v, Rz, Ry, Rx):
    """The same table from the zero-padded float64 autocorrelation -> (int64 table, the largest distance of a value from an
    integer).  Padded to n + R per axis: no lag of the box wraps onto a voxel."""
    v = np.asarray(v, dtype=bool)
    size = tuple(n + r for n, r in zip(v.shape, (Rz, Ry, Rx)))
    f = np.fft.rfftn(v.astype(np.float64), size, axes=(0, 1, 2))
    c = np.fft.irfftn(f * np.conj(f), size, axes=(0, 1, 2))     # c[h] = sum over p of v[p] v[p + h], h modulo the padded size
    z = np.arange(Rz + 1)[:, None, None]
    y = (np.arange(-Ry, Ry + 1) % size[1])[None, :, None]
    x = (np.arange(-Rx, Rx + 1) % size[2])[None, None, :]
    got = c[z, y, x]
    return np.rint(got).astype(np.int64), float(np.abs(got - np.rint(got)).max())


def pairs_loop(v, Rz, Ry, Rx):
    """The same table from a loop over all ordered pairs of set voxels."""
    pts = [tuple(int(a) for a in p) for p in np.argwhere(np.asarray(v, dtype=bool))]
    out = np.zeros((Rz + 1, 2 * Ry + 1, 2 * Rx + 1), dtype=np.int64)
    for p in pts:
        for q in pts:
            hz, hy, hx = q[0] - p[0], q[1] - p[1], q[2] - p[2]
            if 0 <= hz <= Rz and abs(hy) <= Ry and abs(hx) <= Rx:
                out[hz, hy + Ry, hx + Rx] += 1
    return out


def noise(density, shape, seed):
    return np.random.default_rng(seed).random(shape) < density


def ball(R, n):
    """The voxels whose centres lie within R of the centre of an n^3 box."""
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    c = (n - 1) / 2.0
    return (z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2 <= float(R) ** 2
