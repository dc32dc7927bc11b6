"""Host reference for the per-component measurements (pipeline.component_table / component_properties), in plain NumPy on
top of components_reference.label -- for small dense arrays.

measure():    components_reference.label of a bool volume, then table() -> (labels, n, table).
table():      per component the integers of tomo_cc_measure, from np.nonzero of the label array.
properties(): the arrays of pipeline.ComponentProperties for the components the keep rule selects.  The volume is the
              reference's own loop (volume_calculator.py:23-35: slice by slice, np.sum(mask[z]) * (mm_x * mm_y * depth[z]),
              added to a float that starts at 0.0), the box its arithmetic (:59-94), the z centroid the same loop with every
              slice's volume times the slice centre, the in-plane centroids exact integer sums divided by the voxel count.
Everything is sequential float64 in a fixed order, the order the device code documents, so the GPU tests compare with ==."""
import numpy as np

import components_reference as C

COLUMNS = 10


def slice_centres(slice_depths):
    """Centre of slice z in millimetres: the depths in front of it plus half its own (voxel_processor.py:110-119; entries
    1 .. nz of pipeline.distance_positions' z table)."""
    d = np.asarray(slice_depths, dtype=np.float64)
    out = np.empty(len(d), dtype=np.float64)
    pos = 0.0
    for z in range(len(d)):
        out[z] = pos + d[z] / 2.0
        pos += d[z]
    return out


def table(labels, n):
    """-> int64 (n, 10): voxels, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x of component 1..n, from np.nonzero
    in one pass over the set voxels (the noise volumes hold tens of thousands of components)."""
    out = np.zeros((n, COLUMNS), dtype=np.int64)
    idx = np.nonzero(labels)
    c = labels[idx].astype(np.int64) - 1
    out[:, 0] = np.bincount(c, minlength=n)
    for k, a in enumerate(idx):
        a = a.astype(np.int64)
        lo = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
        hi = np.full(n, -1, dtype=np.int64)
        total = np.zeros(n, dtype=np.int64)
        np.minimum.at(lo, c, a)
        np.maximum.at(hi, c, a)
        np.add.at(total, c, a)
        out[:, 1 + 2 * k], out[:, 2 + 2 * k], out[:, 7 + k] = lo, hi, total
    return out


def measure(vol, connectivity=6):
    labels, n = C.label(vol, connectivity)
    return labels, n, table(labels, n)


def slice_counts(labels, n):
    """np.sum((labels == c)[z]) for every component and slice -> int64 (n, nz)."""
    nz = labels.shape[0]
    z = np.nonzero(labels)[0]
    c = labels[labels != 0].astype(np.int64) - 1
    return np.bincount(c * nz + z, minlength=n * nz).reshape(n, nz).astype(np.int64)


def selected(sizes, min_voxels=0, largest=False):
    """0-based components the keep rule selects, ascending (components_reference.keep_from's rule)."""
    sizes = np.asarray(sizes)
    ok = sizes >= min_voxels
    if largest:
        only = np.zeros(len(sizes), dtype=bool)
        if ok.any():
            only[int(np.argmax(np.where(ok, sizes, -1)))] = True      # argmax returns the first maximum
        ok = only
    return np.flatnonzero(ok)


def volume_of(counts, mm_x, mm_y, slice_depths):
    """The reference's calculate_voxel_volume_variable_depth for every row of counts (the voxels per slice of one mask), and
    next to it the same loop weighted with the slice centres -> (volume, moment), float64 per row.  The loop over the slices
    is the reference's; NumPy only carries it out for all rows at once, element by element."""
    zc = slice_centres(slice_depths)
    total, moment = np.zeros(len(counts), dtype=np.float64), np.zeros(len(counts), dtype=np.float64)
    for z in range(min(counts.shape[1], len(slice_depths))):
        v = counts[:, z] * (mm_x * mm_y * slice_depths[z])
        total += v
        moment += v * zc[z]
    return total, moment


def box_of(row, mm_x, mm_y, slice_depths):
    """The reference's calculate_bounding_box_variable_depth from the index box of a table row."""
    z0, z1, y0, y1, x0, x1 = (int(v) for v in row[1:7])
    edges = np.cumsum(np.concatenate([[0], slice_depths]))
    top = min(z1 + 1, len(edges) - 1)
    x, y, z = (x0 * mm_x, x1 * mm_x), (y0 * mm_y, y1 * mm_y), (edges[z0], edges[top])
    return {'x': x, 'y': y, 'z': z, 'dimensions': (x[1] - x[0], y[1] - y[0], z[1] - z[0])}


def properties(labels, tab, slice_depths, mm_y, mm_x, min_voxels=0, largest=False):
    """-> dict of the arrays of pipeline.ComponentProperties for the selected components, in ascending label."""
    slice_depths = np.asarray(slice_depths, dtype=np.float64)
    pick = selected(tab[:, 0], min_voxels, largest)
    rows = tab[pick]
    vol, moment = volume_of(slice_counts(labels, len(tab))[pick], mm_x, mm_y, slice_depths)
    cidx = rows[:, 7:10] / rows[:, 0][:, None]
    cmm = np.stack([moment / vol, cidx[:, 1] * mm_y, cidx[:, 2] * mm_x], axis=1) if len(pick) else np.zeros((0, 3))
    return {"labels": pick.astype(np.int64) + 1, "voxels": rows[:, 0], "index_box": rows[:, 1:7], "index_sums": rows[:, 7:10],
            "volume_mm3": vol, "centroid_index": cidx, "centroid_mm": cmm}
