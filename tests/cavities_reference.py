"""Host reference for the cavity calls (pipeline.cavity_table / cavity_volume / fill_cavities, ComponentRuns.background /
cavity_owners, volume_calculator.closed_porosity): the definitions, literally, in NumPy / SciPy -- for small dense arrays.

Foreground connectivity k is 6 or 26, the background has the complementary k' = 32 - k, everything outside the stack is
background.  A cavity is a component of the complement under k' whose inclusive index box touches no face of the stack; its
label is its label in that labelling (raster order of the first voxel); its owner is the foreground component (label under k)
of the voxel left of the cavity's first voxel in raster order.  The size window lo <= voxels <= hi (hi None: no upper bound)
applies to the cavity's own voxels.

cavities(): (labels, owners, sizes) of all cavities, ascending label.
fill():     the volume OR the cavities inside the window; without a window that is scipy.ndimage.binary_fill_holes with the
            BACKGROUND's structure (tests/test_cavities_cpu.py holds it to that).
table():    the arrays of pipeline.Cavities; volume, box and centroids are component_props_reference's numbers for the mask of
            the cavity (the reference's own slice loop), so the GPU tests compare with == and tobytes().
The labelling is topology_reference.label (SciPy's where it imports)."""
import numpy as np

import component_props_reference as P
import topology_reference as T


def background(v, k):
    """-> (labels of the complement under 32 - k, n, its measurement table int64 (n, 10))."""
    v = np.asarray(v) != 0
    labels, n = T.label(~v, 32 - k)
    return labels, n, P.table(labels, n)


def enclosed(tab, shape):
    """Rows of a measurement table whose inclusive index box touches no face of a stack of that shape."""
    nz, ny, nx = shape
    return ((tab[:, 1] > 0) & (tab[:, 2] < nz - 1) & (tab[:, 3] > 0) & (tab[:, 4] < ny - 1) & (tab[:, 5] > 0) & (tab[:, 6] < nx - 1))


def window(sizes, lo=0, hi=None):
    sizes = np.asarray(sizes)
    return (sizes >= lo) & (sizes <= (np.iinfo(np.int64).max if hi is None else hi))


def owners_of(v, k, bg_labels, n_bg):
    """int64 (n_bg,): for every component of the complement the foreground label left of its first voxel (0 at x = 0)."""
    v = np.asarray(v) != 0
    fg, _ = T.label(v, k)
    flat = bg_labels.ravel()
    idx = np.flatnonzero(flat)
    first = np.zeros(n_bg + 1, dtype=np.int64)
    first[flat[idx][::-1]] = idx[::-1]                             # the last write is the lowest index
    first = first[1:]
    nx = v.shape[2]
    return np.where(first % nx > 0, fg.ravel()[np.maximum(first - 1, 0)], 0).astype(np.int64)


def all_owners(v, k):
    """ComponentRuns.cavity_owners: int64 (n_bg,), the owner of every enclosed background component, 0 for the others."""
    labels, n, tab = background(v, k)
    if n == 0 or not np.asarray(v).any():
        return np.zeros(n, dtype=np.int64)
    return np.where(enclosed(tab, np.shape(v)), owners_of(v, k, labels, n), 0)


def cavities(v, k):
    """-> (labels, owners, sizes) of every cavity, int64, in ascending label."""
    labels, n, tab = background(v, k)
    pick = np.flatnonzero(enclosed(tab, np.shape(v))) if n else np.zeros(0, dtype=np.int64)
    own = owners_of(v, k, labels, n)[pick] if n else np.zeros(0, dtype=np.int64)
    return pick.astype(np.int64) + 1, own, tab[pick, 0]


def cavity_mask(v, k, lo=0, hi=None):
    """The voxels of the cavities inside the window."""
    bg_labels, _, _ = background(v, k)
    labels, _, sizes = cavities(v, k)
    return np.isin(bg_labels, labels[window(sizes, lo, hi)])


def fill(v, k, lo=0, hi=None):
    return (np.asarray(v) != 0) | cavity_mask(v, k, lo, hi)


def table(v, k, depths=None, mm_y=1.0, mm_x=1.0, lo=0, hi=None):
    """-> dict of the arrays of pipeline.Cavities for the cavities inside the window, in ascending label."""
    v = np.asarray(v) != 0
    depths = np.ones(v.shape[0]) if depths is None else np.asarray(depths, dtype=np.float64)
    bg_labels, n, tab = background(v, k)
    labels, own, sizes = cavities(v, k)
    keep = window(sizes, lo, hi)
    labels, own = labels[keep], own[keep]
    pick = labels - 1
    rows = tab[pick] if n else np.zeros((0, P.COLUMNS), dtype=np.int64)
    counts = P.slice_counts(bg_labels, n)[pick] if n else np.zeros((0, v.shape[0]), dtype=np.int64)
    vol, moment = P.volume_of(counts, mm_x, mm_y, depths)
    cidx = rows[:, 7:10] / rows[:, 0][:, None]
    cmm = np.stack([moment / vol, cidx[:, 1] * mm_y, cidx[:, 2] * mm_x], axis=1) if len(pick) else np.zeros((0, 3))
    return {"labels": labels, "owner": own, "voxels": rows[:, 0], "index_box": rows[:, 1:7], "volume_mm3": vol,
            "centroid_mm": cmm, "centroid_index": cidx}


def per_owner(t):
    """owner label -> (cavity voxels, cavity volume added in ascending cavity label, sequential float64) from table()'s dict."""
    out = {}
    for o, n, vol in zip(t["owner"], t["voxels"], t["volume_mm3"]):
        have = out.get(int(o), (0, 0.0))
        out[int(o)] = (have[0] + int(n), have[1] + float(vol))
    return out


def porosity(v, k, depths, mm_x, mm_y, lo=0, hi=None):
    """volume_calculator.closed_porosity's dict."""
    v = np.asarray(v) != 0
    depths = np.asarray(depths, dtype=np.float64)
    t = table(v, k, depths, mm_y, mm_x, lo, hi)
    rows = []
    for i in range(len(t["labels"])):
        box = P.box_of(np.concatenate([[t["voxels"][i]], t["index_box"][i]]), mm_x, mm_y, depths)
        rows.append({'label': int(t["labels"][i]), 'owner': int(t["owner"][i]), 'voxels': int(t["voxels"][i]),
                     'volume_mm3': float(t["volume_mm3"][i]), 'bounding_box': {a: box[a] for a in ('x', 'y', 'z')},
                     'dimensions': box['dimensions'], 'centroid_mm': tuple(float(x) for x in t["centroid_mm"][i]),
                     'centroid_index': tuple(float(x) for x in t["centroid_index"][i]),
                     'equivalent_diameter_mm': float(np.cbrt(6.0 * t["volume_mm3"][i] / np.pi))})
    cavity = 0.0
    for r in rows:
        cavity += r['volume_mm3']
    solid = float(P.volume_of(v.sum(axis=(1, 2), dtype=np.int64)[None, :], mm_x, mm_y, depths)[0][0])
    whole = solid + cavity
    return {'cavities': len(rows), 'cavity_voxels': int(t["voxels"].sum()), 'cavity_volume_mm3': cavity, 'voxel_volume_mm3': solid,
            'closed_porosity': cavity / whole if whole else 0.0, 'table': rows}


# ----------------------------------------------------------------------------- the volumes of the tests
def pores():
    """(9, 12, 140): two blocks either side of an empty column pair; voids of 1, 2, 4, 6 and 12 voxels, one across the word edge
    at x = 64, a pair that touches only diagonally (one cavity under 6, two under 26), a pit open to the empty slice 0 (no
    cavity), and in the second block a large void that crosses x = 128 and holds an island with a void of its own."""
    v = np.zeros((9, 12, 140), dtype=bool)
    v[1:8, 1:11, 2:70] = True
    v[1:8, 1:11, 72:138] = True
    v[3, 3, 10] = False
    v[3, 5, 63:65] = False
    v[4:6, 6:9, 30] = False
    v[2:5, 2:4, 40:42] = False
    v[2, 8, 20] = v[3, 9, 21] = False
    v[1, 5, 50] = False
    v[2:7, 3:9, 100:132] = False
    v[4, 2, 80] = False
    v[3:6, 4:8, 110:120] = True
    v[4, 5:7, 114:116] = False
    return v


def big_noise():
    """More background components than one tile of the selection scan holds (1024), under both connectivities."""
    return T.noise(0.93, shape=(16, 24, 140), seed=11)


def fixtures():
    """topology_reference's fixtures and the two of this file, in a fixed order."""
    out = dict(T.fixtures())
    out["pores"] = pores()
    out["big_noise"] = big_noise()
    return out
