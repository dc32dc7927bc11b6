"""Host reference for the geodesic zones of markers, the cut between zones and the separation of touching objects, in plain
NumPy on top of geodesic_reference (dijkstra), edt_reference (offset_from) and components_reference, which it imports and
leaves alone.  Nothing here calls the product.

The definitions (include/tomo_hip.h).  dist = geodesic_reference.dijkstra from the marker voxels.  An edge q -> p between
neighbouring set voxels is TIGHT when fl32(dist(q) + w(q, p)) == dist(p) with dist(p) finite.  zone(p) = the smallest marker
label among the markers from which p can be reached along tight edges; 0 at unset voxels and where no marker reaches.  That is
the least fixed point of zone(p) = min(zone(p), zone(q) over tight q -> p) over a FIXED graph, so every order ends at the same
bytes: zones() sweeps the cells in raster and anti-raster order in turn (reverse=True: the other way round) until a sweep
changes nothing.  cut(): a set voxel p is cleared when some set neighbour q has 0 < zone(q) < zone(p).  separate(): the markers
are the ball erosion of the volume, labelled under the call's connectivity."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import edt_reference as E  # noqa: E402
import geodesic_reference as G  # noqa: E402
import thickness_reference as T  # noqa: E402

F32 = np.float32
NONE = np.iinfo(np.int64).max


def _shifted(a, off, fill):
    """b[p] = a[p + off], `fill` where p + off lies outside."""
    out = np.full(a.shape, fill, dtype=a.dtype)
    src, dst = [], []
    for n, d in zip(a.shape, off):
        dst.append(slice(max(0, -d), n - max(0, d)))
        src.append(slice(max(0, d), n - max(0, -d)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def marker_map(v, markers, connectivity):
    """markers as the int32 map the definitions speak of: an integer map is taken as it is, a bool volume is labelled under the
    connectivity (1 .. n in raster order of the first voxel).  Entries on unset voxels stay; zones() ignores them."""
    m = np.asarray(markers)
    assert m.shape == np.asarray(v).shape
    if m.dtype == bool:
        return C.label(m, connectivity)[0].astype(np.int32)
    return m.astype(np.int32)


def tight_edges(v, dist, wxy, wz, connectivity):
    """Per offset `off`: the bool volume of the voxels p whose neighbour q = p + off gives a tight edge q -> p."""
    v = np.asarray(v) != 0
    nz = v.shape[0]
    out = []
    for off in G.offsets(connectivity):
        w = np.array([G.step_weight(wxy, wz, k, off) if 0 <= k + off[0] < nz else np.inf for k in range(nz)], dtype=np.float32)
        dq = _shifted(dist, off, G.INF)                              # +inf at unset voxels and outside: never tight
        with np.errstate(invalid="ignore"):
            cand = dq + w[:, None, None]                             # float32 + float32: one rounded addition
        out.append((off, v & np.isfinite(dist) & (cand == dist)))
    return out


def zones(v, markers, wxy, wz, connectivity=26, reverse=False, limit=100000):
    """-> (zones int32, dist float32, sweeps): the label fixed point by in-place sweeps over the fixed tight graph."""
    v = np.asarray(v) != 0
    m = marker_map(v, markers, connectivity)
    seeds = v & (m > 0)
    dist = G.dijkstra(v, seeds, wxy, wz, connectivity)
    zone = np.where(seeds, m.astype(np.int64), NONE)
    nz, ny, nx = v.shape
    preds = [[] for _ in range(v.size)]
    for off, tight in tight_edges(v, dist, wxy, wz, connectivity):
        step = (off[0] * ny + off[1]) * nx + off[2]
        for p in np.flatnonzero(tight.reshape(-1)).tolist():
            preds[p].append(p + step)
    cells = [p for p in np.flatnonzero(v.reshape(-1)).tolist() if preds[p]]
    z = zone.reshape(-1).tolist()
    for sweep in range(limit):
        changed = False
        forward = (sweep % 2 == 0) != bool(reverse)
        for p in (cells if forward else reversed(cells)):
            best = z[p]
            for q in preds[p]:
                if z[q] < best:
                    best = z[q]
            if best < z[p]:
                z[p] = best
                changed = True
        if not changed:
            out = np.array(z, dtype=np.int64).reshape(v.shape)
            out[out == NONE] = 0
            return out.astype(np.int32), dist, sweep + 1
    raise AssertionError("no fixed point within the limit")


def cut(v, zone, connectivity=26):
    """The volume without the set voxels p that have a set neighbour q with 0 < zone(q) < zone(p) -> bool volume."""
    v = np.asarray(v) != 0
    z = np.where(v, np.asarray(zone).astype(np.int64), 0)
    clear = np.zeros(v.shape, dtype=bool)
    for off in G.offsets(connectivity):
        zq = _shifted(z, off, 0)
        clear |= v & (zq > 0) & (zq < z)
    return v & ~clear


def separate(v, kind, radius_mm, connectivity=6, min_marker_voxels=1):
    """-> dict: 'volume' (bool), 'markers' (count), 'cut_voxels', 'zones' (int32), 'marker_volume' (bool), 'dist'."""
    v = np.asarray(v) != 0
    r = float(radius_mm)
    assert r > 0
    tabs = T.tables(v.shape, kind)
    mv = E.offset_from(v, E.edt_squared(v, *tabs, True), -r)
    labels, n = C.label(mv, connectivity)
    if min_marker_voxels > 1:
        mv = C.keep_from(mv, labels, n, min_marker_voxels)
        labels, n = C.label(mv, connectivity)
    wxy, wz = G.weights(v.shape, kind)
    zone, dist, _ = zones(v, labels, wxy, wz, connectivity)
    out = cut(v, zone, connectivity)
    return {"volume": out, "markers": n, "cut_voxels": int(v.sum() - out.sum()), "zones": zone, "marker_volume": mv, "dist": dist}


# ----------------------------------------------------------------------------- the volumes and markers of the tests
DUMBBELL_CASES = (("unit", 3.0), ("sided", 2.0), ("sided", 3.0), ("dyadic", 2.0))    # two markers, two components after
DUMBBELL_WHOLE = ("dyadic", 3.0)                                                      # no marker: the volume comes back


def dumbbell():
    """(14, 18, 80): two balls of radius 6 at (7, 9, 58) and (7, 8, 69), the neck on the word and tile boundary x = 63 | 64."""
    z, y, x = np.indices((14, 18, 80))
    a = (z - 7) ** 2 + (y - 9) ** 2 + (x - 58) ** 2 <= 36
    b = (z - 7) ** 2 + (y - 8) ** 2 + (x - 69) ** 2 <= 36
    return a | b


def default_markers(v, every=97):
    """Every `every`-th set voxel in raster order, labelled 1 .. n -> int32 map."""
    v = np.asarray(v) != 0
    m = np.zeros(v.shape, dtype=np.int32)
    on = np.flatnonzero(v.reshape(-1))[::every]
    m.reshape(-1)[on] = np.arange(1, len(on) + 1, dtype=np.int32)
    return m


def scattered_markers(v, every=97):
    """default_markers with labels that are neither consecutive nor in raster order, some entries on unset voxels (ignored) and
    some negative ones on set voxels (ignored as well) -> int32 map."""
    v = np.asarray(v) != 0
    m = default_markers(v, every)
    n = int(m.max())
    if n:
        relabel = np.concatenate([[0], 5 + 7 * np.random.default_rng(n).permutation(n)]).astype(np.int32)
        m = relabel[m]
    off = np.flatnonzero(~v.reshape(-1))[::max(1, every // 3)]
    m.reshape(-1)[off] = 3 + (np.arange(len(off), dtype=np.int32) % 11)
    neg = np.flatnonzero(v.reshape(-1) & (m.reshape(-1) == 0))[::every]
    m.reshape(-1)[neg] = -4
    return m


def end_markers(v):
    """One marker at each end of a path volume in raster order: label 2 at the first set voxel, label 1 at the last."""
    v = np.asarray(v) != 0
    m = np.zeros(v.shape, dtype=np.int32)
    on = np.flatnonzero(v.reshape(-1))
    m.reshape(-1)[on[0]], m.reshape(-1)[on[-1]] = 2, 1
    return m
