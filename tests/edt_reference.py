"""Host reference for the distance-transform tests: the exact Euclidean distance transform with a coordinate table per axis,
in plain NumPy (the GPU machine may not have SciPy, and SciPy's `sampling` cannot express slice depths that change).

edt_squared(): three separable passes (x, then y, then z).  Every pass takes the EXHAUSTIVE minimum over all sites of its
line -- O(n^2) per line, no envelope logic -- in float64, d2 = ((dx^2 + dy^2) + dz^2), every d the difference of two table
entries.  Rounding is monotone, so the minimum per line of the rounded partial sums is the rounded 3-D minimum.
tests/golden/make_distance_golden.py holds edt() against scipy.ndimage.distance_transform_edt on padded volumes: 0 ulp.

Tables: positions() -> (zt, yt, xt) with n + 2 entries each; entry i + 1 is the centre of index i, entries 0 and n + 1 are
the virtual background sites outside the volume.  inside=True: sites = unset voxels and all virtual positions; inside=False:
sites = set voxels only (no site: +inf).

fixtures(): the volumes of the tests, by name; the golden file stores them bit-packed next to SciPy's answers."""
import numpy as np

UNIFORM = (0.5, 0.7, 0.9)            # (depth, mm_y, mm_x) of the uniform mm spacing
CHUNK = 1 << 16                      # elements a pass keeps in flight: the working set stays in cache


def pack(vol):
    """A bool volume as BitVolume.bits holds it: int64 (nz, ny, words), bit b of word w = voxel 64 w + b, tail bits zero."""
    a = np.asarray(vol) != 0
    nz, ny, nx = a.shape
    wx = (nx + 63) // 64
    by = np.zeros((nz, ny, wx * 8), dtype=np.uint8)
    pb = np.packbits(a, axis=2, bitorder="little")
    by[:, :, :pb.shape[2]] = pb
    return by.view("<u8").astype(np.uint64).view(np.int64).reshape(nz, ny, wx)


def unpack(bits, shape):
    by = np.ascontiguousarray(bits).view(np.uint8).reshape(shape[0], shape[1], -1)
    return np.unpackbits(by, axis=2, bitorder="little")[:, :, :shape[2]].astype(bool)


# ----------------------------------------------------------------------------- coordinates
def sided_depths(nz):
    """Three-sided slice depths in the pattern of VoxelProcessor.calculate_slice_depths: [0.8] * a + [0.25] * b + [1.3] * c."""
    a = nz // 3
    b = (nz - a) // 2
    return np.array([0.8] * a + [0.25] * b + [1.3] * (nz - a - b), dtype=np.float64)


def spacing(kind, nz):
    """-> (slice_depths or None, mm_y, mm_x) as the product's functions take them."""
    if kind == "unit":
        return None, 1.0, 1.0
    if kind == "uniform":
        return np.full(nz, UNIFORM[0]), UNIFORM[1], UNIFORM[2]
    if kind == "sided":
        return sided_depths(nz), UNIFORM[1], UNIFORM[2]
    raise ValueError(kind)


SPACINGS = ("unit", "uniform", "sided")


def positions(shape, slice_depths=None, mm_y=1.0, mm_x=1.0):
    """-> (zt, yt, xt): the slice centres cum[k] + d[k] / 2 between zc[0] - d[0] and zc[-1] + d[-1]; j * mm_y and i * mm_x
    for j, i = -1 .. n."""
    nz, ny, nx = shape
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64)
    assert d.shape == (nz,)
    cum = np.cumsum(np.concatenate([[0.0], d]))
    zc = cum[:-1] + d / 2
    zt = np.concatenate([[zc[0] - d[0]], zc, [zc[-1] + d[-1]]])
    return zt, np.arange(-1, ny + 1, dtype=np.float64) * mm_y, np.arange(-1, nx + 1, dtype=np.float64) * mm_x


# ----------------------------------------------------------------------------- the transform
def _line_pass(f, p, vval, axis):
    """out[t] = min over the slots s = 0 .. n + 1 of (f(s) + (p[t + 1] - p[s]) ** 2) along `axis`; f(0) = f(n + 1) = vval."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    rest = f.shape[1:]
    f2 = np.ascontiguousarray(f).reshape(n, -1)
    out = np.empty_like(f2)
    d = p[1:-1, None] - p[None, :]                               # (n, n + 2) coordinate differences, float64
    dsq = d * d
    cols = max(1, CHUNK // n)
    for a in range(0, f2.shape[1], cols):
        fc = f2[:, a:a + cols]
        best = np.full(fc.shape, np.inf)
        tmp = np.empty_like(best)
        for s in range(n + 2):
            if s == 0 or s == n + 1:
                if not np.isfinite(vval):
                    continue
                np.add(vval, dsq[:, s][:, None], out=tmp)
            else:
                np.add(fc[s - 1][None, :], dsq[:, s][:, None], out=tmp)
            np.minimum(best, tmp, out=best)
        out[:, a:a + cols] = best
    return np.moveaxis(out.reshape((n,) + rest), 0, axis)


def edt_squared(v, zt, yt, xt, inside=True):
    """float64 (nz, ny, nx): the squared distance to the nearest site (+inf without one)."""
    v = np.asarray(v) != 0
    if inside:
        f, vval = np.where(v, np.inf, 0.0), 0.0
    else:
        f, vval = np.where(v, 0.0, np.inf), np.inf
    f = _line_pass(f, np.asarray(xt, dtype=np.float64), vval, 2)
    f = _line_pass(f, np.asarray(yt, dtype=np.float64), vval, 1)
    return _line_pass(f, np.asarray(zt, dtype=np.float64), vval, 0)


def edt(v, zt, yt, xt, inside=True):
    """float32 (nz, ny, nx) = float32(sqrt(d2))."""
    return np.sqrt(edt_squared(v, zt, yt, xt, inside)).astype(np.float32)


def offset_from(v, d2, r):
    """The ball erosion (r < 0, d2 = inside) / dilation (r > 0, d2 = outside) given the squared distances, in float64."""
    v = np.asarray(v) != 0
    if r < 0:
        return v & (d2 > r * r)
    if r > 0:
        return v | (d2 <= r * r)
    return v.copy()


def offset(v, r, zt, yt, xt):
    return offset_from(v, None if r == 0 else edt_squared(v, zt, yt, xt, r < 0), r)


def sphere_from(v, dist):
    """(radius, (k, j, i)) from the inside distance: its maximum and the first voxel in raster order that attains it."""
    if not np.asarray(v).any():
        return None
    flat = int(np.argmax(dist))
    return float(dist.reshape(-1)[flat]), tuple(int(i) for i in np.unravel_index(flat, dist.shape))


def sphere(v, zt, yt, xt):
    return sphere_from(v, edt(v, zt, yt, xt, True))


# ----------------------------------------------------------------------------- the volumes of the tests
def _ellipsoid(shape, centre, radii):
    z, y, x = np.indices(shape)
    return (((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2) <= 1.0


def _tall():
    v = np.zeros((130, 6, 67), dtype=bool)
    v[2:128, 1:5, 3:66] = True
    v[40, 2, 30] = v[100, 3, 64] = False
    return v


def fixtures():
    """name -> bool volume, in a fixed order."""
    out = {}
    out["one"] = np.ones((1, 1, 1), dtype=bool)
    out["tail"] = np.ones((2, 3, 65), dtype=bool)
    out["empty"] = np.zeros((3, 5, 70), dtype=bool)
    hole = np.ones((9, 40, 131), dtype=bool)
    hole[4, 17, 64] = False
    out["hole"] = hole
    ell = _ellipsoid((24, 50, 150), (10.5, 27.0, 66.0), (8.0, 18.0, 55.0))
    assert not (ell[0].any() or ell[-1].any() or ell[:, 0].any() or ell[:, -1].any() or ell[:, :, 0].any() or ell[:, :, -1].any())
    out["ellipsoid"] = ell
    rng = np.random.default_rng(17)
    out["speckle"] = _ellipsoid((17, 33, 200), (8.0, 15.0, 110.0), (6.5, 12.0, 80.0)) ^ (rng.random((17, 33, 200)) < 0.01)
    out["tall"] = _tall()
    out["wide"] = np.ascontiguousarray(_tall().transpose(1, 0, 2))
    big = _ellipsoid((70, 130, 260), (30.0, 60.0, 120.0), (34.0, 50.0, 125.0))       # touches z = 0 and x = 0
    assert big[0].any() and big[:, :, 0].any() and not big[-1].any() and not big[:, :, -1].any()
    for k, j, i in ((30, 60, 120), (12, 80, 63), (50, 40, 192), (31, 61, 128)):
        big[k, j, i] = False
    big[20:23, 30:33, 200:204] = False
    out["big"] = big
    return out
