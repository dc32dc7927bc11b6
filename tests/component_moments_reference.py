"""Host reference for the per-component second moments (pipeline.component_moments), in plain NumPy on top of
components_reference.label and component_props_reference.selected -- for small dense arrays.

The definition (include/tomo_hip.h, tomo_cc_moments): a set voxel (k, j, i) of component c is a point mass at
p = (zc[k], j * mm_y, i * mm_x) -- zc the slice centres of pipeline.distance_positions -- of weight w[k] = (mm_x * mm_y) *
depth[k].  W = sum w, centre = sum w p / W, covariance = sum w (p - centre)(p - centre)^T / W in (z, y, x) order; no d^2 / 12
for a voxel's own extent.  Principal variances: the eigenvalues, descending (clamped at 0); principal axes: the unit
eigenvectors as ROWS in that order, the component of largest magnitude positive (the first such on a tie); a zero matrix has
zeros and the identity; ellipsoid axes 2 sqrt(5 lambda).

moments(): per selected component the definition from the coordinates np.nonzero(labels == c) gives, in np.longdouble and
two passes (the centre first, then the sums about it).  One np.nonzero of the label array sorted by label (stable: every
component keeps its raster order) stands for the np.nonzero per component, so that the noise volumes' tens of thousands of
components take one pass.  Eigenvalues and eigenvectors: np.linalg.eigh of the float64 covariance."""
import numpy as np

import component_props_reference as P

GAP = 1e-6                   # an eigenvalue gap above GAP * D^2 pins the axes on either side of it (Davis-Kahan: |dC| / gap)
AXES_MIN_VOXELS = 8          # the selection under which at least half the components of a golden volume must have both gaps


def sign_rule(v):
    """Rows of (..., 3, 3): the component of largest magnitude made positive, the first such on a tie."""
    v = np.array(v, dtype=np.float64)
    k = np.argmax(np.abs(v), axis=-1)                            # argmax returns the first maximum
    lead = np.take_along_axis(v, k[..., None], axis=-1)
    return np.where(lead < 0, -v, v)


def eigen(cov):
    """(m, 3, 3) symmetric float64 -> (variances (m, 3) descending, clamped at 0; axes (m, 3, 3), rows, sign rule)."""
    cov = np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3)
    if not len(cov):
        return np.zeros((0, 3)), np.zeros((0, 3, 3))
    lam, vec = np.linalg.eigh(cov)                               # ascending, eigenvectors in columns
    lam = np.maximum(lam[:, ::-1], 0.0)
    axes = sign_rule(np.transpose(vec, (0, 2, 1))[:, ::-1, :])
    zero = ~cov.any(axis=(1, 2))
    lam[zero] = 0.0
    axes[zero] = np.eye(3)
    return lam, axes


def scale2(rows, slice_depths, mm_y, mm_x):
    """D^2 per table row: the squared diagonal of the component's box in mm, voxel extents included (along z the summed
    depths of the box's slices)."""
    edges = np.concatenate([[0.0], np.cumsum(np.asarray(slice_depths, dtype=np.float64))])
    dz = edges[rows[:, 2] + 1] - edges[rows[:, 1]]
    dy = (rows[:, 4] - rows[:, 3] + 1) * mm_y
    dx = (rows[:, 6] - rows[:, 5] + 1) * mm_x
    return dz * dz + dy * dy + dx * dx


def moments(labels, tab, slice_depths, mm_y, mm_x, min_voxels=0, largest=False):
    """-> dict of the arrays of pipeline.ComponentMoments for the selected components, in ascending label, and "scale2"."""
    ld = np.longdouble
    depths = np.asarray(slice_depths, dtype=np.float64)
    pick = P.selected(tab[:, 0], min_voxels, largest)
    m = len(pick)
    rows = tab[pick]
    out = {"labels": pick.astype(np.int64) + 1, "voxels": rows[:, 0], "scale2": scale2(rows, depths, mm_y, mm_x)}
    if m == 0:
        out.update(volume_mm3=np.zeros(0), center_of_mass_mm=np.zeros((0, 3)), covariance_mm2=np.zeros((0, 3, 3)),
                   principal_variances_mm2=np.zeros((0, 3)), principal_axes=np.zeros((0, 3, 3)), ellipsoid_axes_mm=np.zeros((0, 3)))
        return out
    zc = P.slice_centres(depths)
    row_of = np.full(len(tab) + 1, -1, dtype=np.int64)
    row_of[pick + 1] = np.arange(m)
    k, j, i = np.nonzero(labels)
    r = row_of[labels[k, j, i]]
    order = np.argsort(r, kind="stable")
    order = order[r[order] >= 0]
    k, j, i, r = k[order], j[order], i[order], r[order]
    starts = np.searchsorted(r, np.arange(m))
    w = ((mm_x * mm_y) * depths).astype(ld)[k]
    p = np.stack([zc.astype(ld)[k], j.astype(ld) * ld(mm_y), i.astype(ld) * ld(mm_x)], axis=1)
    total = np.add.reduceat(w, starts)
    centre = np.add.reduceat(w[:, None] * p, starts, axis=0) / total[:, None]
    d = p - centre[r]
    cov = np.empty((m, 3, 3), dtype=ld)
    for a in range(3):
        for b in range(a, 3):
            cov[:, a, b] = cov[:, b, a] = np.add.reduceat(w * d[:, a] * d[:, b], starts) / total
    cov = cov.astype(np.float64)
    lam, axes = eigen(cov)
    out.update(volume_mm3=total.astype(np.float64), center_of_mass_mm=centre.astype(np.float64), covariance_mm2=cov,
               principal_variances_mm2=lam, principal_axes=axes, ellipsoid_axes_mm=2.0 * np.sqrt(5.0 * lam))
    return out


def gaps_hold(ref):
    """Per component: both eigenvalue gaps exceed GAP * D^2 (the axes are then compared one by one)."""
    lam = ref["principal_variances_mm2"]
    return np.minimum(lam[:, 0] - lam[:, 1], lam[:, 1] - lam[:, 2]) > GAP * ref["scale2"]


def axis_pinned(ref):
    """(m, 3) bool: the eigenvalue of that axis is further than GAP * D^2 from both its neighbours -- the axis is pinned
    whatever the other two do.  All three where gaps_hold()."""
    lam = ref["principal_variances_mm2"]
    g = np.diff(-lam, axis=1) > GAP * ref["scale2"][:, None]     # (m, 2): gap 0-1, gap 1-2
    return np.stack([g[:, 0], g[:, 0] & g[:, 1], g[:, 1]], axis=1)


# ----------------------------------------------------------------------------- the built volumes of the tests
def ellipsoid():
    """Semi-axes (12, 9, 20) in a 32 x 24 x 48 box, centred: full axes (24, 18, 40)."""
    z, y, x = np.indices((32, 24, 48)).astype(np.float64)
    return ((z - 15.5) / 12) ** 2 + ((y - 11.5) / 9) ** 2 + ((x - 23.5) / 20) ** 2 <= 1.0


def tilted_rod():
    """A two-voxel-wide rod in 40^3 about the line z = x / 2: the voxels within half a slice of it, one per even column and
    two per odd one, so that it is one component under connectivity 6 too.  Along (-0.447, 0, -0.894) up to the sign rule."""
    v = np.zeros((40, 40, 40), dtype=bool)
    for x in range(2, 39):
        v[x // 2:(x + 1) // 2 + 1, 19:21, x] = True
    return v


def plane():
    v = np.zeros((5, 20, 70), dtype=bool)
    v[3] = True
    return v


def corner_rod():
    """A rod along z in the far corner: the largest offsets of the volume, no extent in the plane."""
    v = np.zeros((20, 33, 131), dtype=bool)
    v[3:, 32, 130] = True
    return v


def single():
    v = np.zeros((3, 4, 70), dtype=bool)
    v[1, 2, 65] = True
    return v


def pair():
    """Two voxels either side of the word seam x = 63 / 64."""
    v = np.zeros((2, 3, 70), dtype=bool)
    v[1, 1, 63:65] = True
    return v


def dumbbell():
    """Two far-apart voxels joined by one row: one above the row's first voxel, one below its last."""
    v = np.zeros((3, 6, 200), dtype=bool)
    v[1, 2, 3] = True
    v[1, 3, 3:197] = True
    v[1, 4, 196] = True
    return v


BUILT = {"ellipsoid": ellipsoid, "tilted_rod": tilted_rod, "plane": plane, "corner_rod": corner_rod, "single": single,
         "pair": pair, "dumbbell": dumbbell}
# which axes are pinned (axis_pinned) by construction, under any of the spacings of the tests: all three unless the shape
# is thin -- rank <= 1 (two eigenvalues are exactly 0), one voxel (rank 0), or a row whose transverse variance is far below
# GAP * D^2
PINNED = {"ellipsoid": (True, True, True), "tilted_rod": (True, True, True), "plane": (True, True, True),
          "corner_rod": (True, False, False), "single": (False, False, False), "pair": (True, False, False),
          "dumbbell": (True, False, False)}
