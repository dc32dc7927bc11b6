"""Host reference for the branch table of a skeleton (include/tomo_hip.h, "The branch table of a skeleton"): the definition
restated in NumPy and pure Python, for small dense arrays.

split():        degrees from 26 shifted sums of the padded volume; R = the set voxels of degree 2, N the other set voxels.
table():        branches = components_reference.label(R, 26), nodes = label(N, 26); the edge counts per branch, slice and column
                from 26 shifted comparisons (a step to a node voxel always counts, a step to a regular voxel only forwards); the
                length as the sequential float64 sum over the slices and the columns; the attachments from the same shifts.
prune_round():  one round of pruning;  prune(): `rounds` of them, or to the fixed point.
Everything is sequential float64 in the documented order, so the GPU tests compare with ==."""
import math

import numpy as np

import component_props_reference as P
import components_reference as C
import surface_reference as SR

STEPS = SR.STEPS                     # the 26 offsets (dz, dy, dx)
COLUMNS = 11


def degrees(vol):
    """Per voxel the number of set 26-neighbours."""
    vol = np.asarray(vol, dtype=bool)
    nz, ny, nx = vol.shape
    p = np.pad(vol, 1).astype(np.int32)
    n = np.zeros(vol.shape, dtype=np.int32)
    for dz, dy, dx in STEPS:
        n += p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    return n


def split(vol):
    """-> (R, N, degrees)."""
    vol = np.asarray(vol, dtype=bool)
    deg = degrees(vol)
    regular = vol & (deg == 2)
    return regular, vol & ~regular, deg


def steps(slice_depths, nz, mm_y=1.0, mm_x=1.0):
    """The step lengths -> float64 (nz, 11): sqrt(((dx mm_x)^2 + (dy mm_y)^2) + dzc^2), one entry at a time."""
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    assert len(d) == nz
    zc = P.slice_centres(d)
    out = np.zeros((nz, COLUMNS), dtype=np.float64)
    for k in range(nz):
        for c in range(COLUMNS):
            az, ay, ax = SR.CLASSES[c if c < 7 else c - 4]
            dzc = 0.0
            if az and c < 7 and k + 1 < nz:
                dzc = float(zc[k + 1]) - float(zc[k])
            if az and c >= 7 and k > 0:
                dzc = float(zc[k]) - float(zc[k - 1])
            out[k, c] = math.sqrt(((ax * float(mm_x)) * (ax * float(mm_x)) + (ay * float(mm_y)) * (ay * float(mm_y))) + dzc * dzc)
    return out


def lengths(counts, F):
    """The sequential sum of count * step over the slices in ascending k, inside a slice in ascending column, for every row of
    counts (m, nz, 11) at once: NumPy only carries the loop out for all rows, element by element."""
    s = np.zeros(len(counts), dtype=np.float64)
    for k in range(counts.shape[1]):
        for c in range(COLUMNS):
            s = s + counts[:, k, c].astype(np.float64) * float(F[k][c])
    return s


def _shifted(padded, shape, step):
    nz, ny, nx = shape
    dz, dy, dx = step
    return padded[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def edge_counts(regular, nodes, labels, n):
    """-> int64 (n, nz, 11): the edges of every branch, filed at the regular voxel that counts them."""
    shape = regular.shape
    pr, pn = np.pad(regular, 1), np.pad(nodes, 1)
    out = np.zeros((n, shape[0], COLUMNS), dtype=np.int64)
    for step in STEPS:
        hit = regular & _shifted(pn, shape, step)
        if step > (0, 0, 0):                                                          # raster-later: a forward neighbour
            hit |= regular & _shifted(pr, shape, step)
        z = np.nonzero(hit)[0]
        np.add.at(out[:, :, SR.column(*step)], (labels[hit].astype(np.int64) - 1, z), 1)
    return out


def attachments(regular, nodes, labels, n):
    """-> (attach int64 (n, 2): the lowest and the highest flat index of an attached node voxel, -1 where there is none;
    count int64 (n,): the attachments with multiplicity)."""
    shape = regular.shape
    nz, ny, nx = shape
    pn = np.pad(nodes, 1)
    lo = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full(n, -1, dtype=np.int64)
    count = np.zeros(n, dtype=np.int64)
    for dz, dy, dx in STEPS:
        hit = regular & _shifted(pn, shape, (dz, dy, dx))
        z, y, x = np.nonzero(hit)
        flat = ((z + dz).astype(np.int64) * ny + (y + dy)) * nx + (x + dx)
        c = labels[hit].astype(np.int64) - 1
        np.minimum.at(lo, c, flat)
        np.maximum.at(hi, c, flat)
        np.add.at(count, c, 1)
    lo[count == 0] = -1
    return np.stack([lo, hi], axis=1), count


def positions_of(flat, shape, zc, mm_y, mm_x):
    """The (z, y, x) position in mm of the voxels at the flat indices."""
    nz, ny, nx = shape
    flat = np.asarray(flat, dtype=np.int64)
    k, rest = flat // (ny * nx), flat % (ny * nx)
    return zc[k], (rest // nx) * float(mm_y), (rest % nx) * float(mm_x)


def chord(attach, shape, zc, mm_y, mm_x):
    """The Euclidean distance between the two attached voxels, float64 sqrt(((dx)^2 + (dy)^2) + dz^2); NaN for a cycle."""
    attach = np.asarray(attach, dtype=np.int64).reshape(-1, 2)
    cycle = attach[:, 0] < 0
    (za, ya, xa), (zb, yb, xb) = (positions_of(np.where(cycle, 0, attach[:, i]), shape, zc, mm_y, mm_x) for i in (0, 1))
    dz, dy, dx = zb - za, yb - ya, xb - xa
    return np.where(cycle, np.nan, np.sqrt((dx * dx + dy * dy) + dz * dz))


def table(vol, slice_depths=None, mm_y=1.0, mm_x=1.0, min_voxels=0):
    """-> dict: regular, node_voxels (bool volumes), voxels, regular_voxels, node_voxel_count, isolated, branches and nodes
    (dicts of arrays, one row per selected branch / per node in ascending label), counts (per selected branch (nz, 11)),
    attach_count, branch_labels and node_labels (the label arrays)."""
    vol = np.asarray(vol, dtype=bool)
    shape = vol.shape
    nz = shape[0]
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    zc = P.slice_centres(d)
    F = steps(d, nz, mm_y, mm_x)
    regular, nodes, deg = split(vol)
    bl, nb = C.label(regular, 26)
    nl, nn = C.label(nodes, 26)
    counts = edge_counts(regular, nodes, bl, nb)
    attach, acount = attachments(regular, nodes, bl, nb)
    sizes = C.sizes(bl, nb)
    pick = np.flatnonzero(sizes >= max(0, int(min_voxels)))
    counts, attach, acount = counts[pick], attach[pick], acount[pick]
    flat_nodes = np.concatenate([[0], nl.reshape(-1)])                                # label of flat index i at i + 1; -1 -> 0
    node_of = flat_nodes[attach + 1].astype(np.int64)
    ntab = P.table(nl, nn)
    props = P.properties(nl, ntab, d, float(mm_y), float(mm_x))
    idx = np.nonzero(nodes)
    which = nl[idx].astype(np.int64) - 1
    end_voxels = np.bincount(which[deg[idx] <= 1], minlength=nn).astype(np.int64)
    junction_voxels = np.bincount(which[deg[idx] >= 3], minlength=nn).astype(np.int64)
    one = np.bincount(which[deg[idx] == 1], minlength=nn)
    free_end = (ntab[:, 0] == 1) & (one == 1)
    free = np.concatenate([[False], free_end])[node_of]                               # (m, 2); a cycle reads node 0: False
    cycle = acount == 0
    kind = np.where(cycle, 0, 3 - free.sum(axis=1)).astype(np.int64)
    long = lengths(counts, F)
    chords = chord(attach, shape, zc, mm_y, mm_x)
    with np.errstate(divide="ignore", invalid="ignore"):
        tort = np.where(cycle, np.nan, np.where(chords == 0, np.inf, long / chords))
    branches = {"label": pick.astype(np.int64) + 1, "voxels": sizes[pick], "length_mm": long, "step_counts": SR.fold(counts.sum(axis=1)),
                "attach_index": attach, "nodes": node_of, "chord_mm": chords, "tortuosity": tort, "kind": kind}
    per_node = np.bincount(node_of[~cycle].reshape(-1), minlength=nn + 1)[1:].astype(np.int64)
    nodes_rows = {"label": np.arange(1, nn + 1, dtype=np.int64), "voxels": ntab[:, 0].copy(), "end_voxels": end_voxels,
                  "junction_voxels": junction_voxels, "branches": per_node, "index_box": ntab[:, 1:7].copy(),
                  "centroid_index": props["centroid_index"], "centroid_mm": props["centroid_mm"], "free_end": free_end}
    return {"regular": regular, "node_voxels": nodes, "voxels": int(vol.sum()), "regular_voxels": int(regular.sum()),
            "node_voxel_count": int(nodes.sum()), "isolated": int((vol & (deg == 0)).sum()), "branches": branches, "nodes": nodes_rows,
            "counts": counts, "attach_count": acount, "branch_labels": bl, "node_labels": nl}


def prune_round(vol, min_length_mm, slice_depths=None, mm_y=1.0, mm_x=1.0):
    """One round -> (the pruned volume, removed branches, removed voxels): every branch of kind 2 shorter than min_length_mm
    goes, with the free-end voxel it hangs from; the other node stays."""
    vol = np.asarray(vol, dtype=bool)
    t = table(vol, slice_depths, mm_y, mm_x)
    b = t["branches"]
    gone = (b["kind"] == 2) & (b["length_mm"] < float(min_length_mm))
    out = vol.copy()
    if gone.any():
        out &= ~np.isin(t["branch_labels"], b["label"][gone])
        ends = b["nodes"][gone]
        ends = ends[np.concatenate([[False], t["nodes"]["free_end"]])[ends]]          # of the two nodes the free end
        out &= ~np.isin(t["node_labels"], ends)
    return out, int(gone.sum()), int(vol.sum() - out.sum())


def prune(vol, min_length_mm, slice_depths=None, mm_y=1.0, mm_x=1.0, rounds=1):
    """-> (volume, removed branches, removed voxels, the rounds that removed something); rounds=None: to the fixed point."""
    vol = np.asarray(vol, dtype=bool)
    branches = voxels = done = 0
    while rounds is None or done < rounds:
        vol, nb, nv = prune_round(vol, min_length_mm, slice_depths, mm_y, mm_x)
        if nb == 0:
            break
        branches, voxels, done = branches + nb, voxels + nv, done + 1
    return vol, branches, voxels, done


# ------------------------------------------------------------------------------------------------ shapes
def bar(shape, start, step, n):
    """n voxels from `start` in steps of `step`."""
    v = np.zeros(shape, dtype=bool)
    for i in range(n):
        v[start[0] + i * step[0], start[1] + i * step[1], start[2] + i * step[2]] = True
    return v


def ring(shape=(3, 8, 8), z=1, lo=1, hi=6):
    """A square ring in slice z: the border of [lo, hi]^2 without its four corners (with them the voxels beside a corner would
    have three neighbours under the 26-adjacency)."""
    v = np.zeros(shape, dtype=bool)
    v[z, lo:hi + 1, lo:hi + 1] = True
    v[z, lo + 1:hi, lo + 1:hi] = False
    for y in (lo, hi):
        for x in (lo, hi):
            v[z, y, x] = False
    return v


def lollipop():
    """The ring with a stick along x."""
    v = ring((3, 8, 16))
    v[1, 3, 7:14] = True
    return v


def plus(arm=4, shape=(3, 11, 11)):
    v = np.zeros(shape, dtype=bool)
    c = shape[1] // 2
    v[1, c, c - arm:c + arm + 1] = True
    v[1, c - arm:c + arm + 1, c] = True
    return v


def ypsilon(shape=(3, 12, 70), at=(1, 5, 30), long=20, short=3):
    """A bar along x with an arm of `short` voxels along y at its middle: the arm is a spur."""
    v = np.zeros(shape, dtype=bool)
    z, y, x = at
    v[z, y, x - long:x + long + 1] = True
    v[z, y + 1:y + 1 + short, x] = True
    return v


def one_step_spur():
    """A bar with a one-step spur: the spur voxel touches three voxels of the bar and is a junction voxel of their node."""
    v = np.zeros((3, 5, 12), dtype=bool)
    v[1, 2, 1:11] = True
    v[1, 3, 5] = True
    return v


def end_beside_junction():
    """A junction voxel j = (3, 3, 3) with two diagonal arms of three voxels and an end voxel e = (3, 3, 4) that touches j alone:
    j and e are one node of two voxels, which is no free end."""
    v = np.zeros((7, 7, 6), dtype=bool)
    v[3, 3, 3] = v[3, 3, 4] = True
    for t in (1, 2, 3):
        v[3 - t, 3 - t, 3 - t] = True
        v[3 + t, 3 + t, 3 - t] = True
    return v
