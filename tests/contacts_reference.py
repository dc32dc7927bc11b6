"""Host reference for the contact table between zones (pipeline.zone_contacts), in plain NumPy: thirteen shifted comparisons,
np.unique over the keys, per-slice counts and the sequential float64 sum.  Nothing here calls the device code and nothing
hashes: the rows come from np.unique.  The factor table F and the step weights are handed in (pipeline.surface_factors and
geodesic_reference.weights: host NumPy, the definitions the table is stated in).

The definition (include/tomo_hip.h).  A voxel takes part when it is set and its entry in `zones` is positive.  A contact pair
is an unordered pair of 26-adjacent voxels that take part and lie in different zones; it is counted once, at its raster-earlier
voxel p, which looks at its 13 forward neighbours.  It belongs to the zone pair (min, max) of the labels, to the slice of p and
to the class (|dz|, |dy|, |dx|) of the step, in surface_reference.CLASSES' order.

brute() is the same table by a plain triple loop over ALL 26 neighbours, every unordered pair met twice and halved."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_reference as G  # noqa: E402
import surface_reference as S  # noqa: E402
import zones_reference as Z  # noqa: E402

FORWARD = [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1)] + [(1, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
FACE_CLASSES = (0, 1, 3)          # x, y, z: what a contact under connectivity 6 needs


def klass(off):
    return S.CLASSES.index(tuple(abs(a) for a in off))


def labels_of(v, zones):
    """The label where a voxel takes part, 0 elsewhere -> int64."""
    v = np.asarray(v) != 0
    z = np.asarray(zones).astype(np.int64)
    return np.where(v & (z > 0), z, 0)


def pair_list(v, zones):
    """Every contact pair -> int64 arrays (a, b, k, class, p, q, direction), p and q flat indices, in no particular order."""
    z = labels_of(v, zones)
    nz, ny, nx = z.shape
    cols = [[] for _ in range(7)]
    for d, off in enumerate(FORWARD):
        zq = Z._shifted(z, off, 0)
        hit = (z > 0) & (zq > 0) & (zq != z)
        p = np.flatnonzero(hit.reshape(-1))
        zp, zn = z.reshape(-1)[p], zq.reshape(-1)[p]
        q = p + (off[0] * ny + off[1]) * nx + off[2]
        for col, a in zip(cols, (np.minimum(zp, zn), np.maximum(zp, zn), p // (ny * nx), np.full(len(p), klass(off)), p, q,
                                 np.full(len(p), d))):
            col.append(np.asarray(a, dtype=np.int64))
    return tuple(np.concatenate(c) for c in cols)


def area_of(counts, F, directions=13):
    """The sequential float64 sum over the slices in ascending k and the classes in ascending order; class c reads column c of F."""
    s = 0.0
    for k in range(len(counts)):
        for c in range(7):
            if directions == 13 or c in FACE_CLASSES:
                s += float(counts[k][c]) * float(F[k][c])
    return s


def areas(per_slice, F, directions=13):
    """area_of for every row at once: the same additions in the same order per row, the rows side by side."""
    s = np.zeros(len(per_slice), dtype=np.float64)
    for k in range(per_slice.shape[1]):
        for c in range(7):
            if directions == 13 or c in FACE_CLASSES:
                s = s + per_slice[:, k, c].astype(np.float64) * float(F[k][c])
    return s


def contacts(v, zones, F, directions=13, connectivity=26, values=None, dist=None, weights=None):
    """-> dict of host arrays, the rows sorted by (zone_a, zone_b): zone_a, zone_b, pairs, pair_counts (P, 7), slice_counts
    (P, nz, 7), area_mm2, z_range (P, 2), first_index (P, 3); with values: value_max float32, value_index (P, 3); with dist and
    weights = (wxy, wz): path_mm float32."""
    v = np.asarray(v) != 0
    shape = v.shape
    nz = shape[0]
    a, b, k, cls, p, q, d = pair_list(v, zones)
    keys, row = np.unique((a << 32) | b, return_inverse=True)
    row = row.reshape(-1)
    P = len(keys)
    per_slice = np.zeros((P, nz, 7), dtype=np.int64)
    np.add.at(per_slice, (row, k, cls), 1)
    z_lo, z_hi = np.full(P, nz, dtype=np.int64), np.full(P, -1, dtype=np.int64)
    first = np.full(P, v.size, dtype=np.int64)
    np.minimum.at(z_lo, row, k)
    np.maximum.at(z_hi, row, k)
    np.minimum.at(first, row, p)
    out = {"zone_a": keys >> 32, "zone_b": keys & 0xFFFFFFFF, "pairs": np.bincount(row, minlength=P).astype(np.int64),
           "pair_counts": per_slice.sum(axis=1), "slice_counts": per_slice,
           "area_mm2": areas(per_slice, F, directions),
           "z_range": np.stack([z_lo, z_hi], axis=1).reshape(-1, 2), "first_index": unravel(first, shape)}
    if values is not None:
        val = np.asarray(values, dtype=np.float32).reshape(-1)
        assert not np.isnan(val).any()
        top = np.full(P, -np.inf, dtype=np.float32)
        np.maximum.at(top, row, np.maximum(val[p], val[q]))
        where = np.full(P, v.size, dtype=np.int64)
        for idx in (p, q):
            at = val[idx] == top[row]
            np.minimum.at(where, row[at], idx[at])
        out["value_max"], out["value_index"] = top + np.float32(0.0), unravel(where, shape)
    if dist is not None:
        wxy, wz = weights
        dd = np.asarray(dist, dtype=np.float32).reshape(-1)
        w = np.array([[G.step_weight(wxy, wz, kk, off) if kk + off[0] < nz else np.inf for off in FORWARD] for kk in range(nz)],
                     dtype=np.float32)
        way = (dd[p] + w[k, d]).astype(np.float32) + dd[q]                # two rounded float32 additions
        assert way.dtype == np.float32
        best = np.full(P, np.inf, dtype=np.float32)
        np.minimum.at(best, row, way)
        out["path_mm"] = best
    if connectivity == 6:
        keep = out["pair_counts"][:, list(FACE_CLASSES)].sum(axis=1) > 0
        out = {name: col[keep] for name, col in out.items()}
    else:
        assert connectivity == 26
    return out


def unravel(flat, shape):
    return np.stack(np.unravel_index(np.asarray(flat, dtype=np.int64), shape), axis=1).astype(np.int64).reshape(-1, 3)


def brute(v, zones):
    """{(a, b): (pairs, [per class])} by a triple loop over all 26 neighbours: every unordered pair is met from both ends."""
    z = labels_of(v, zones)
    nz, ny, nx = z.shape
    twice = {}
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                own = int(z[k, j, i])
                if own <= 0:
                    continue
                for dz, dy, dx in S.STEPS:
                    kk, jj, ii = k + dz, j + dy, i + dx
                    if 0 <= kk < nz and 0 <= jj < ny and 0 <= ii < nx:
                        other = int(z[kk, jj, ii])
                        if other > 0 and other != own:
                            n = twice.setdefault((min(own, other), max(own, other)), [0] * 8)
                            n[0] += 1
                            n[1 + klass((dz, dy, dx))] += 1
    assert all(c % 2 == 0 for n in twice.values() for c in n)
    return {key: (n[0] // 2, [c // 2 for c in n[1:]]) for key, n in twice.items()}


def coordination(table, labels=None):
    """-> (labels, neighbours, area): per zone the distinct zones it touches and its summed contact area, the rows in order."""
    za, zb, area = table["zone_a"], table["zone_b"], table["area_mm2"]
    if labels is None:
        labels = np.unique(np.concatenate([za, zb]))
    labels = np.asarray(labels, dtype=np.int64)
    n = {int(c): 0 for c in labels}
    s = {int(c): 0.0 for c in labels}
    for half in (za, zb):                                        # zone_a of every row first, then zone_b: the product's order
        for r in range(len(half)):
            c = int(half[r])
            if c in n:
                n[c] += 1
                s[c] += float(area[r])
    return labels, np.array([n[int(c)] for c in labels], dtype=np.int64), np.array([s[int(c)] for c in labels], dtype=np.float64)


# ----------------------------------------------------------------------------- the maps of the tests
def every_voxel_its_own_zone(v):
    """zone = flat index + 1 at every set voxel: the most zone pairs a volume can have."""
    v = np.asarray(v) != 0
    return np.where(v, np.arange(1, v.size + 1, dtype=np.int64).reshape(v.shape), 0).astype(np.int32)


def few_labels(shape, n=5, seed=3):
    """n labels drawn at random: few keys, every wave full of contacts."""
    return np.random.default_rng(seed).integers(1, n + 1, shape).astype(np.int32)


def high_labels(shape, seed=4):
    """Labels next to 2^31 - 1."""
    top = np.iinfo(np.int32).max
    return (top - np.random.default_rng(seed).integers(0, 7, shape)).astype(np.int32)


def mixed_signs(v, seed=5):
    """Positive entries on unset voxels and negative ones on set voxels among the labels 1 .. 9."""
    v = np.asarray(v) != 0
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 10, v.shape).astype(np.int32)
    m[v & (rng.random(v.shape) < 0.2)] = -3
    m[v & (rng.random(v.shape) < 0.05)] = 0
    return m


def halves(shape, axis, at):
    """Everything set; zone 1 below index `at` along `axis`, zone 2 from it on -> (volume, zones)."""
    idx = np.indices(shape)[axis]
    return np.ones(shape, dtype=bool), np.where(idx < at, 1, 2).astype(np.int32)
