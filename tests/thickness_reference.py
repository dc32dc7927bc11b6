"""Host reference for the local-thickness tests, in plain NumPy on top of edt_reference (which it imports and leaves alone).

Definition (include/tomo_hip.h, pipeline.local_thickness).  D2(q) = the float64 squared inside distance of set voxel q,
|pq|^2 = ((dx^2 + dy^2) + dz^2) in float64, every d a difference of two entries of the coordinate tables.  For ascending
squared radii r_1^2 < ... < r_K^2

    level(p) = max{ k : there is a set voxel q with D2(q) >= r_k^2 and |pq|^2 < r_k^2 }

at a set voxel p, 0 without such a k or at an unset voxel.  Two forms that tests/test_thickness_cpu.py holds against each other:

direct()     the brute force over all pairs of set voxels, max{D2(q) : |pq|^2 < D2(q)}: with every distinct D2 as a level this
             is r_level^2.
by_levels()  one exhaustive OUTSIDE transform (edt_reference.edt_squared, inside=False) of the eroded set per level; later
             levels overwrite, which is the max.

expected() turns a level map into everything pipeline.local_thickness returns.  fixtures(): the volumes of the tests."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as E  # noqa: E402

ROWS = 256                           # set voxels per chunk of the brute force


# ----------------------------------------------------------------------------- coordinates
def dyadic_depths(nz):
    """[0.75] * a + [0.25] * b + [1.25] * c, split as edt_reference.sided_depths does."""
    a = nz // 3
    b = (nz - a) // 2
    return np.array([0.75] * a + [0.25] * b + [1.25] * (nz - a - b), dtype=np.float64)


def spacing(kind, nz):
    """-> (slice_depths or None, mm_y, mm_x).  "dyadic": every coordinate, square and partial sum is exact in float64, so no
    choice of site can go wrong by rounding and equality is bit for bit."""
    if kind == "dyadic":
        return dyadic_depths(nz), 0.5, 0.75
    if kind in ("unit", "sided"):
        return E.spacing(kind, nz)
    raise ValueError(kind)


def tables(shape, kind):
    return E.positions(shape, *spacing(kind, shape[0]))


def slice_weights(shape, kind):
    """(mm_x * mm_y) * depth[k]: the volume of one voxel of slice k."""
    depths, mm_y, mm_x = spacing(kind, shape[0])
    d = np.ones(shape[0]) if depths is None else np.asarray(depths, dtype=np.float64)
    return (mm_x * mm_y) * d


# ----------------------------------------------------------------------------- the two forms
def direct(v, d2, zt, yt, xt):
    """float64 (nz, ny, nx): max{D2(q) : |pq|^2 < D2(q)} over the set voxels q at a set voxel p, 0 at an unset one."""
    v = np.asarray(v) != 0
    out = np.zeros(v.shape, dtype=np.float64)
    k, j, i = np.nonzero(v)
    if len(k) == 0:
        return out
    z, y, x, dq = zt[k + 1], yt[j + 1], xt[i + 1], d2[v]
    best = np.zeros(len(k), dtype=np.float64)
    for a in range(0, len(k), ROWS):
        s = slice(a, a + ROWS)
        dx, dy, dz = x[s, None] - x[None, :], y[s, None] - y[None, :], z[s, None] - z[None, :]
        pq = (dx * dx + dy * dy) + dz * dz
        best[s] = np.where(pq < dq[None, :], dq[None, :], 0.0).max(axis=1)
    out[v] = best
    return out


def eroded(v, d2, r2):
    """The centres where the open ball of squared radius r2 fits."""
    return (np.asarray(v) != 0) & (d2 >= r2)


def cover(v, d2, tabs, r2):
    """(the opening by the open ball of squared radius r2, the outside squared distances to the eroded set or None)."""
    v = np.asarray(v) != 0
    e = eroded(v, d2, r2)
    if not e.any():
        return np.zeros(v.shape, dtype=bool), None
    out = E.edt_squared(e, *tabs, inside=False)
    return v & (out < r2), out


def by_levels(v, d2, tabs, r2s):
    """int32 (nz, ny, nx): the level map, 1-based, 0 = none."""
    level = np.zeros(np.asarray(v).shape, dtype=np.int32)
    for k, r2 in enumerate(r2s):
        level[cover(v, d2, tabs, r2)[0]] = k + 1
    return level


def distinct_levels(v, d2):
    """All distinct D2 over the set voxels, ascending: the levels of the exact mode."""
    return np.unique(d2[np.asarray(v) != 0])


# ----------------------------------------------------------------------------- what local_thickness returns
def expected(v, level, radii, weights):
    """dict of the fields of pipeline.LocalThickness from a level map, the radii (float64, ascending) and the slice weights."""
    v = np.asarray(v) != 0
    radii = np.asarray(radii, dtype=np.float64)
    K = len(radii)
    table = np.concatenate([[np.float32(0)], (2.0 * radii).astype(np.float32)]).astype(np.float32)
    thickness = np.where(v, table[level], np.float32(0)).astype(np.float32)
    voxels = np.zeros(K, dtype=np.int64)
    volume = np.zeros(K, dtype=np.float64)
    for k in range(K):
        acc = 0.0
        for z in range(v.shape[0]):
            n = int((v[z] & (level[z] == k + 1)).sum())
            acc = acc + n * weights[z]
            voxels[k] += n
        volume[k] = acc
    d = [2.0 * float(r) for r in radii]
    w = [float(x) for x in volume]
    total = math.fsum(w)
    if total > 0:
        mean = math.fsum(a * b for a, b in zip(w, d)) / total
        std = math.sqrt(math.fsum(a * ((b - mean) * (b - mean)) for a, b in zip(w, d)) / total)
        top = max(b for a, b in zip(w, d) if a > 0)
    else:
        mean = std = top = 0.0
    return {"thickness": thickness, "radii_mm": radii, "level_voxels": voxels, "level_volume_mm3": volume,
            "uncovered_voxels": int((v & (level == 0)).sum()), "mean_mm": mean, "std_mm": std, "max_mm": top}


# ----------------------------------------------------------------------------- the volumes of the tests
def _ball(shape, centre, r):
    z, y, x = np.indices(shape)
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= r * r


def fixtures():
    """name -> bool volume, in a fixed order; none has more than about 6 000 set voxels."""
    out = {}
    out["one"] = np.ones((1, 1, 1), dtype=bool)
    out["empty"] = np.zeros((3, 5, 70), dtype=bool)
    out["full"] = np.ones((5, 7, 66), dtype=bool)               # touches every face: the virtual sites decide
    plate = np.zeros((12, 20, 70), dtype=bool)
    plate[4:7, 2:18, 3:67] = True
    out["plate"] = plate
    bell = _ball((16, 24, 80), (8, 12, 9), 6) | _ball((16, 24, 80), (8, 12, 70), 4)
    bell[7:10, 11:14, 9:71] = True                              # thick, thin and thick again in one object
    out["dumbbell"] = bell
    shape = (10, 18, 67)
    z, y, x = np.indices(shape)
    ell = ((z - 4.5) / 4.0) ** 2 + ((y - 8.5) / 7.0) ** 2 + ((x - 33.0) / 30.0) ** 2 <= 1.0
    out["speckle"] = ell ^ (np.random.default_rng(23).random(shape) < 0.03)
    out["shell"] = _ball((15, 15, 67), (7, 7, 33), 6.5) & ~_ball((15, 15, 67), (7, 7, 33), 3.5)
    edge = np.zeros((9, 14, 131), dtype=bool)                   # crosses the words at 64 and 128, touches x = 0 and x = 130
    edge[3:6, 4:10, :] = True
    edge[1:8, 2:12, 58:72] = True
    edge[2:7, 3:11, 122:131] = True
    out["edge"] = edge
    for name, v in out.items():
        assert v.sum() <= 6500, name
    return out
