"""Host reference for the caliper (Feret) diameters and the oriented box per component (pipeline.component_caliper /
cavity_caliper), in plain NumPy on top of components_reference.label -- for small dense arrays.

The definition (include/tomo_hip.h, tomo_cc_caliper).  Coordinates are those of the distance transform: voxel (k, j, i) sits
at (zc[k], j * mm_y, i * mm_x), zc the slice centres (the inner entries of pipeline.distance_positions), d_k the depth of
slice k.  A direction is a unit vector u = (u_z, u_y, u_x) in float64; u and -u give the same width.
Shared directions: three float64 tables PZ[m][k] = zc[k] * u_z, PY[m][j] = (j * mm_y) * u_y, PX[m][i] = (i * mm_x) * u_x; the
projection of a voxel is p = ((PZ[m][k] + PY[m][j]) + PX[m][i]) + 0.0 -- additions only, in this order; the + 0.0 turns -0.0
into +0.0.  extent "centres": hi = max p, lo = min p over the voxels of the component.  extent "voxels": the union of the voxel
boxes, hi = max(p + H[m][k]), lo = min(p - H[m][k]) with H[m][k] = 0.5 * ((|u_z| * d_k + |u_y| * mm_y) + |u_x| * mm_x).
width = hi - lo.  The largest and the smallest width take the first direction among equals.
Per-component directions (oriented): the three directions of a component are the rows a of its principal axes; p = ((zc[k] *
a_z + (j * mm_y) * a_y) + (i * mm_x) * a_x) + 0.0 and H = 0.5 * ((|a_z| * d_k + |a_y| * mm_y) + |a_x| * mm_x), every product and
sum rounded on its own (NumPy never fuses).  The centre of the oriented box is the midpoint 0.5 * (hi + lo) along each axis
mapped back to (z, y, x): (mid_0 * a_0 + mid_1 * a_1) + mid_2 * a_2; its volume (e_0 * e_1) * e_2.

Everything here runs over ALL voxels of `labels == c` (one np.nonzero sorted by label, reduced per component), never over run
ends; `only` restricts the voxels, which is how tests/test_caliper_cpu.py shows that the run ends alone give the same bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import component_moments_reference as M  # noqa: E402
import component_props_reference as P  # noqa: E402
import component_thickness_reference as R  # noqa: E402
import components_reference as C  # noqa: E402

KINDS = ("unit", "dyadic", "odd")
EXTENTS = ("voxels", "centres")
RULES = R.RULES
FIELDS = ("labels", "voxels", "directions", "hi_mm", "lo_mm", "width_mm", "max_mm", "max_index", "max_direction", "min_mm",
          "min_index", "min_direction")
ORIENTED = ("axes", "oriented_extent_mm", "oriented_center_mm", "oriented_volume_mm3")


def spacing(kind, nz):
    """-> (depths float64 (nz,), mm_y, mm_x).  unit; dyadic: every product is exact; odd: nothing is."""
    k = np.arange(nz)
    if kind == "unit":
        return np.ones(nz), 1.0, 1.0
    if kind == "dyadic":
        return np.array([0.5, 1.0, 2.0])[k % 3], 0.5, 0.25
    if kind == "odd":
        return np.array([0.9, 1.3, 0.45])[k % 3], 0.3, 0.7
    raise ValueError(kind)


def fixtures():
    """name -> bool volume, in a fixed order: the seven built shapes of the moments, grains, and from components_reference the
    noise volume with thousands of components and two word-seam volumes.  nx = 40, 48, 70, 130, 131, 200; ny < 64 in all but
    none, so a wave straddles slices; every volume but `single` and `pair` has more rows than one workgroup holds or close."""
    out = {name: f() for name, f in M.BUILT.items()}
    out["grains"] = R.grains()
    c = C.fixtures()
    for name in ("noise_031", "words_70", "words_130"):
        out[name] = c[name]
    return out


def direction_sets():
    """name -> float64 (M, 3): the sets of the GPU tier.  13 and 64 of the default construction, one single oblique direction,
    and 67 -- no multiple of the kernel's batch of 8: the last batch is partial.  The construction is restated here."""
    def default(count):
        out = np.zeros((count, 3))
        out[0, 0] = out[1, 1] = out[2, 2] = 1.0
        n = count - 3
        i = np.arange(n, dtype=np.float64)
        z = (i + 0.5) / n
        r = np.sqrt(1.0 - z * z)
        phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
        rows = np.stack([z, r * np.sin(phi), r * np.cos(phi)], axis=1)
        out[3:] = rows / np.sqrt((rows * rows).sum(axis=1))[:, None]
        return out
    one = np.array([[2.0, -3.0, 6.0]]) / 7.0                    # exact: 4 + 9 + 36 = 49; a negative component
    return {"d13": default(13), "d64": default(64), "one": one, "d67": default(67)}


class Grid:
    """The coordinates of a volume of `shape` under a spacing."""

    def __init__(self, shape, kind):
        nz, ny, nx = shape
        self.depth, self.mm_y, self.mm_x = spacing(kind, nz)
        self.zc = P.slice_centres(self.depth)
        self.yt = np.arange(ny, dtype=np.float64) * self.mm_y
        self.xt = np.arange(nx, dtype=np.float64) * self.mm_x


def voxels_by_label(labels, n, only=None):
    """(k, j, i, starts): the set voxels sorted by label (stable: raster order inside a component), starts[c - 1] = the first of
    label c.  only: a bool mask of the voxels to keep -- every label must keep at least one."""
    lab = labels if only is None else np.where(only, labels, 0)
    k, j, i = np.nonzero(lab)
    c = lab[k, j, i]
    order = np.argsort(c, kind="stable")
    k, j, i, c = k[order], j[order], i[order], c[order]
    starts = np.searchsorted(c, np.arange(1, n + 1))
    assert n == 0 or (c[starts] == np.arange(1, n + 1)).all()
    return k, j, i, starts


def extremes(labels, n, grid, directions, extent, only=None):
    """hi, lo float64 (n, M) of every component along the shared directions, over all its voxels (or those of `only`)."""
    u = np.asarray(directions, dtype=np.float64)
    m = len(u)
    if n == 0:
        return np.zeros((0, m)), np.zeros((0, m))
    k, j, i, starts = voxels_by_label(labels, n, only)
    pz, py, px = grid.zc[None, :] * u[:, 0:1], grid.yt[None, :] * u[:, 1:2], grid.xt[None, :] * u[:, 2:3]
    p = ((pz[:, k] + py[:, j]) + px[:, i]) + 0.0
    if extent == "voxels":
        a = np.abs(u)
        h = 0.5 * ((a[:, 0:1] * grid.depth[None, :] + a[:, 1:2] * grid.mm_y) + a[:, 2:3] * grid.mm_x)
        up, down = p + h[:, k], p - h[:, k]
    else:
        assert extent == "centres"
        up = down = p
    return np.ascontiguousarray(np.maximum.reduceat(up, starts, axis=1).T), np.ascontiguousarray(np.minimum.reduceat(down, starts, axis=1).T)


def caliper(labels, n, grid, directions, extent, min_voxels=0, largest=False, keep=None):
    """-> dict of the arrays of pipeline.ComponentCaliper (FIELDS) for the selected components in ascending label.  keep: a bool
    (n,) mask applied on top of the rule (the enclosed components, for the pores)."""
    u = np.ascontiguousarray(directions, dtype=np.float64)
    sizes = C.sizes(labels, n)
    pick = P.selected(sizes, min_voxels, largest) if n else np.zeros(0, dtype=np.int64)
    if keep is not None:
        pick = pick[keep[pick]]
    hi, lo = extremes(labels, n, grid, u, extent)
    hi, lo = np.ascontiguousarray(hi[pick]), np.ascontiguousarray(lo[pick])
    width = hi - lo
    imax = np.argmax(width, axis=1).astype(np.int64) if len(pick) else np.zeros(0, dtype=np.int64)       # the first among equals
    imin = np.argmin(width, axis=1).astype(np.int64) if len(pick) else np.zeros(0, dtype=np.int64)
    rows = np.arange(len(pick))
    return {"labels": pick.astype(np.int64) + 1, "voxels": sizes[pick].astype(np.int64), "directions": u, "hi_mm": hi, "lo_mm": lo,
            "width_mm": width, "max_mm": width[rows, imax], "max_index": imax, "max_direction": u[imax], "min_mm": width[rows, imin],
            "min_index": imin, "min_direction": u[imin], "pick": pick}


def oriented(labels, n, grid, pick, axes, extent):
    """-> dict of the ORIENTED arrays for the components `pick` (0-based, ascending) measured along the rows of axes (m, 3, 3)."""
    axes = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1, 3, 3)
    m = len(pick)
    assert len(axes) == m
    if m == 0:
        return {"axes": axes, "oriented_extent_mm": np.zeros((0, 3)), "oriented_center_mm": np.zeros((0, 3)),
                "oriented_volume_mm3": np.zeros(0)}
    row_of = np.zeros(n + 1, dtype=np.int64)
    row_of[pick + 1] = np.arange(1, m + 1)
    k, j, i, starts = voxels_by_label(row_of[labels], m)
    a = np.repeat(axes, np.diff(np.concatenate([starts, [len(k)]])), axis=0)                 # (N, 3, 3): the axes of every voxel's component
    p = ((grid.zc[k][:, None] * a[:, :, 0] + grid.yt[j][:, None] * a[:, :, 1]) + grid.xt[i][:, None] * a[:, :, 2]) + 0.0
    if extent == "voxels":
        b = np.abs(a)
        h = 0.5 * ((b[:, :, 0] * grid.depth[k][:, None] + b[:, :, 1] * grid.mm_y) + b[:, :, 2] * grid.mm_x)
        up, down = p + h, p - h
    else:
        up = down = p
    hi, lo = np.maximum.reduceat(up, starts, axis=0), np.minimum.reduceat(down, starts, axis=0)
    ext = hi - lo
    mid = 0.5 * (hi + lo)
    centre = (mid[:, 0:1] * axes[:, 0, :] + mid[:, 1:2] * axes[:, 1, :]) + mid[:, 2:3] * axes[:, 2, :]
    return {"axes": axes, "oriented_extent_mm": np.ascontiguousarray(ext), "oriented_center_mm": np.ascontiguousarray(centre),
            "oriented_volume_mm3": (ext[:, 0] * ext[:, 1]) * ext[:, 2]}


def run_ends(v):
    """The set voxels that begin or end an x-run."""
    v = np.asarray(v) != 0
    left = np.zeros_like(v)
    right = np.zeros_like(v)
    left[:, :, 1:] = v[:, :, :-1]
    right[:, :, :-1] = v[:, :, 1:]
    return v & ~(left & right)


def enclosed_mask(labels, n):
    """bool (n,): the components whose inclusive index box touches no face of the stack."""
    tab = P.table(labels, n)
    nz, ny, nx = labels.shape
    return ((tab[:, 1] > 0) & (tab[:, 2] < nz - 1) & (tab[:, 3] > 0) & (tab[:, 4] < ny - 1) & (tab[:, 5] > 0) & (tab[:, 6] < nx - 1)) if n else np.zeros(0, dtype=bool)


def pores(v, connectivity, kind, directions, extent, min_voxels=0, max_voxels=None):
    """The reference for the cavities of v: the enclosed components of the complement under 32 - connectivity in the size window."""
    outside = ~(np.asarray(v) != 0)
    labels, n = C.label(outside, 32 - connectivity)
    keep = enclosed_mask(labels, n)
    if max_voxels is not None:
        keep = keep & (C.sizes(labels, n) <= max_voxels)
    return labels, n, caliper(labels, n, Grid(v.shape, kind), directions, extent, min_voxels, False, keep)


def diameter(points):
    """The largest pairwise distance of the rows of points (N, 3), float64."""
    d = points[:, None, :] - points[None, :, :]
    return float(np.sqrt((d * d).sum(axis=2).max()))
