"""CPU tier of the geodesic zones, the cut and the separation: the reference (tests/zones_reference.py) against the definition
computed another way and against itself in another order -- the claim the tiled label sweep rests on: the tight graph is
fixed, so every order ends at the same bytes --, the properties of the cut, the dumbbell, and the plumbing (exports, argument
checks before any device use, flags off by default).  None of it needs a GPU."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import geodesic_reference as G  # noqa: E402
import test_abi  # noqa: E402
import zones_reference as Z  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

FIXTURES = G.fixtures()
NOISE = ("noise_tiles", "noise_words")
NEW_SYMBOLS = ("tomo_zone_seed_labels", "tomo_zone_sweep", "tomo_zone_cut")
_cache = {}


def swept(name, conn, kind):
    """The reference's zones of a noise fixture, computed once and shared, read-only -> (zones, dist, sweeps)."""
    key = (name, conn, kind)
    if key not in _cache:
        v = FIXTURES[name]
        _cache[key] = Z.zones(v, Z.default_markers(v), *G.weights(v.shape, kind), conn)
    return _cache[key]


def by_definition(v, markers, dist, wxy, wz, conn):
    """zone(p) = the smallest label that reaches p along tight edges: per label in ascending order a breadth-first search over
    the tight edges, the first label wins (what a later label reaches through a taken voxel, the earlier one reached too).
    The tight test is made edge by edge with scalar np.float32 additions."""
    nz, ny, nx = v.shape
    flat_v = v.reshape(-1).tolist()
    d = list(dist.reshape(-1))                                                       # np.float32 scalars
    succ = collections.defaultdict(list)
    for q in np.flatnonzero(v.reshape(-1)).tolist():
        if not np.isfinite(d[q]):
            continue
        k, rest = divmod(q, ny * nx)
        j, i = divmod(rest, nx)
        for off in G.offsets(conn):
            a, b, c = k + off[0], j + off[1], i + off[2]
            if 0 <= a < nz and 0 <= b < ny and 0 <= c < nx:
                p = (a * ny + b) * nx + c
                if flat_v[p] and np.isfinite(d[p]) and d[q] + np.float32(G.step_weight(wxy, wz, k, off)) == d[p]:
                    succ[q].append(p)
    zone = np.zeros(v.size, dtype=np.int32)
    m = np.where(v, markers, 0).reshape(-1)
    for label in sorted(set(m[m > 0].tolist())):
        todo = collections.deque(np.flatnonzero(m == label).tolist())
        for p in todo:
            zone[p] = label
        while todo:
            q = todo.popleft()
            for p in succ[q]:
                if zone[p] == 0:
                    zone[p] = label
                    todo.append(p)
    return zone.reshape(v.shape)


# ------------------------------------------------------------------ the fixed point
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_the_sweeps_end_at_the_definition(conn, kind):
    for name in NOISE:
        v = FIXTURES[name]
        markers = Z.default_markers(v)
        assert markers.max() >= 40 and ((markers > 0) <= v).all()
        zone, dist, sweeps = swept(name, conn, kind)
        w = G.weights(v.shape, kind)
        assert dist.tobytes() == G.dijkstra(v, markers > 0, *w, conn).tobytes()
        want = by_definition(v, markers, dist, *w, conn)
        assert zone.dtype == np.int32 and zone.tobytes() == want.tobytes(), (name, conn, kind)
        assert (zone[~v] == 0).all() and ((zone > 0) == np.isfinite(dist)).all()
        assert (zone[markers > 0] == markers[markers > 0]).all()                     # a marker voxel keeps its label
        assert sweeps >= 2
        print("%s/%d/%s: %d markers, %d sweeps" % (name, conn, kind, markers.max(), sweeps))


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_forward_and_reversed_orders_give_the_same_bytes(conn, kind):
    for name in NOISE:
        v = FIXTURES[name]
        zone, dist, _ = swept(name, conn, kind)
        other, dist2, _ = Z.zones(v, Z.default_markers(v), *G.weights(v.shape, kind), conn, reverse=True)
        assert other.tobytes() == zone.tobytes() and dist2.tobytes() == dist.tobytes(), (name, conn, kind)


def test_unit_spacing_is_where_ties_abound():
    """Under unit spacing many voxels have tight edges from voxels of several zones: the minimum decides there."""
    v = FIXTURES["noise_tiles"]
    zone, dist, _ = swept("noise_tiles", 6, "unit")
    mixed = np.zeros(v.shape, dtype=bool)
    lo = np.where(zone > 0, zone, np.iinfo(np.int32).max)
    for off, tight in Z.tight_edges(v, dist, *G.weights(v.shape, "unit"), 6):
        zq = Z._shifted(lo, off, np.iinfo(np.int32).max)
        mixed |= tight & (zq > zone)
    assert mixed.sum() >= 50


def test_markers_ignored_and_kept():
    v = FIXTURES["noise_tiles"]
    w = G.weights(v.shape, "sided")
    plain = Z.default_markers(v)
    odd = Z.scattered_markers(v)
    assert ((odd > 0) & ~v).any() and ((odd < 0) & v).any() and ((odd > 0) & v).sum() == (plain > 0).sum()
    a, da, _ = Z.zones(v, plain, *w, 26)
    b, db, _ = Z.zones(v, odd, *w, 26)
    assert da.tobytes() == db.tobytes()
    assert set(np.unique(b)) <= set(np.unique(np.where(v, odd, 0)[np.where(v, odd, 0) > 0])) | {0}
    # the bool form: labelled under the connectivity, in raster order
    mb = np.zeros(v.shape, dtype=bool)
    mb[2:4, 3:6, 10:14] = True
    mb[6:8, 12:15, 50:55] = True
    labels, n = C.label(mb, 26)
    assert n == 2 and Z.zones(v, mb, *w, 26)[0].tobytes() == Z.zones(v, labels, *w, 26)[0].tobytes()


# ------------------------------------------------------------------ the cut
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_after_the_cut_every_component_lies_in_one_zone(conn):
    for name, kind in (("noise_tiles", "unit"), ("noise_words", "sided"), ("noise_tiles", "dyadic")):
        v = FIXTURES[name]
        zone, _, _ = swept(name, conn, kind)
        out = Z.cut(v, zone, conn)
        assert (out <= v).all() and out.sum() < v.sum()
        assert (out[zone == 0] == v[zone == 0]).all()                               # a component without a marker is untouched
        labels, n = C.label(out, conn)
        lo = np.full(n + 1, np.iinfo(np.int32).max, dtype=np.int64)
        hi = np.full(n + 1, -1, dtype=np.int64)
        np.minimum.at(lo, labels[out], zone[out])
        np.maximum.at(hi, labels[out], zone[out])
        assert (lo[1:] == hi[1:]).all(), (name, conn, kind)
        z = np.where(out, zone, 0)
        for off in G.offsets(conn):                                                  # no two adjacent voxels of different zones
            zq = Z._shifted(z, off, 0)
            assert not ((z > 0) & (zq > 0) & (zq != z)).any(), (name, conn, kind, off)
        cleared = v & ~out                                                           # the lower label keeps the contact
        low = np.zeros(v.shape, dtype=bool)
        zv = np.where(v, zone, 0)
        for off in G.offsets(conn):
            zq = Z._shifted(zv, off, 0)
            low |= (zq > 0) & (zq < zv)
        assert np.array_equal(cleared, v & low)


def test_a_rod_is_cut_on_the_side_of_the_higher_label():
    v = np.ones((1, 1, 9), dtype=bool)
    m = np.zeros(v.shape, dtype=np.int32)
    m[0, 0, 0], m[0, 0, 8] = 2, 1
    for conn in C.CONNECTIVITIES:
        zone, dist, _ = Z.zones(v, m, *G.weights(v.shape, "unit"), conn)
        assert dist[0, 0].tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0]
        assert zone[0, 0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]                    # the middle voxel: a tie, the lower label
        assert Z.cut(v, zone, conn)[0, 0].tolist() == [True, True, True, False, True, True, True, True, True]


# ------------------------------------------------------------------ the dumbbell
def test_the_dumbbell():
    v = Z.dumbbell()
    assert v.shape == (14, 18, 80) and v.sum() == 1848
    assert v[:, :, 63].any() and v[:, :, 64].any() and v[:, :, 63].sum() < 40          # the neck, on the word and tile boundary
    for conn in C.CONNECTIVITIES:
        assert C.label(v, conn)[1] == 1
        for kind, r in Z.DUMBBELL_CASES:
            s = Z.separate(v, kind, r, conn)
            assert s["markers"] == 2 and C.label(s["volume"], conn)[1] == 2, (kind, r, conn)
            assert 30 <= s["cut_voxels"] <= 55 and s["cut_voxels"] == v.sum() - s["volume"].sum()
            assert set(np.unique(s["zones"])) == {0, 1, 2} and ((s["zones"] > 0) == v).all()
            labels, _ = C.label(s["volume"], conn)
            assert labels[7, 9, 58] != labels[7, 8, 69] and labels[7, 9, 58] > 0 and labels[7, 8, 69] > 0
            print("dumbbell %s r=%g conn=%d: %d voxels cut" % (kind, r, conn, s["cut_voxels"]))
        s = Z.separate(v, *Z.DUMBBELL_WHOLE, conn)
        assert s["markers"] == 0 and s["cut_voxels"] == 0 and np.array_equal(s["volume"], v) and not s["zones"].any()
    s = Z.separate(v, "unit", 3.0, 6, min_marker_voxels=10 ** 6)                       # every marker dropped
    assert s["markers"] == 0 and np.array_equal(s["volume"], v)


# ------------------------------------------------------------------ the plumbing
def test_exports_and_signatures():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert [s for s in syms if s.startswith("tomo_zone_")] == sorted(NEW_SYMBOLS)
    assert {"zone_calls", "zone_sweeps", "zone_cuts", "separate_components"} <= set(pipeline.COUNTERS)


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(8)]
    a, b, c, d, e, f, g, h = (ctypes.addressof(x) for x in bufs)                      # distinct host buffers, never dereferenced
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        assert L.tomo_zone_seed_labels(a, b, *bad, c, d, e, None) == -1
        assert L.tomo_zone_sweep(a, *bad, 6, b, c, d, e, f, g, h, None) == -1
        assert L.tomo_zone_cut(a, b, *bad, 6, c, d, None) == -1
    big = (1 << 12, 1 << 13, 1 << 12)                                                 # 2^31 words
    assert L.tomo_zone_seed_labels(a, b, *big, c, d, e, None) == -3
    assert L.tomo_zone_sweep(a, *big, 6, b, c, d, e, f, g, h, None) == -3
    assert L.tomo_zone_cut(a, b, *big, 6, c, d, None) == -3
    assert L.tomo_zone_cut(a, b, 1 << 15, 1 << 15, 1 << 15, 26, c, d, None) == -3    # 2^31 tiles and more
    for k in (0, 1, 5, 6, 7):
        args = [a, b, 4, 4, 4, c, d, e]
        args[k] = None
        assert L.tomo_zone_seed_labels(*args, None) == -1
    assert L.tomo_zone_seed_labels(a, b, 4, 4, 4, c, b, e, None) == -1                # the zone map over the marker map
    good = [a, 4, 4, 4, 26, b, c, d, e, f, g, h]
    for k in (0, 5, 6, 7, 8, 9, 10, 11):
        args = list(good)
        args[k] = None
        assert L.tomo_zone_sweep(*args, None) == -1
    for conn in (0, 4, 8, 18, 27, -6):
        assert L.tomo_zone_sweep(a, 4, 4, 4, conn, b, c, d, e, f, g, h, None) == -1
        assert L.tomo_zone_cut(a, b, 4, 4, 4, conn, c, d, None) == -1
    assert L.tomo_zone_sweep(a, 4, 4, 4, 6, b, c, d, e, f, f, h, None) == -1          # one array for both sets of flags
    assert L.tomo_zone_sweep(a, 4, 4, 4, 6, b, c, d, d, f, g, h, None) == -1          # the zone map over the distance map
    for k in (0, 1, 6, 7):
        args = [a, b, 4, 4, 4, 26, c, d]
        args[k] = None
        assert L.tomo_zone_cut(*args, None) == -1
    assert L.tomo_zone_cut(a, b, 4, 4, 4, 26, a, d, None) == -1                       # in place
    assert L.tomo_zone_cut(a, b, 4, 4, 4, 26, b, d, None) == -1


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(pipeline._lib, "lib", boom)
    monkeypatch.setattr(volume_calculator, "to_device_volume", boom)


def host_volume(shape=(3, 4, 70)):
    return pipeline.BitVolume(torch.zeros((shape[0], shape[1], (shape[2] + 63) // 64), dtype=torch.int64), shape)


BAD_DEPTHS = (np.ones(4), np.ones(2), [], [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0])
BAD_PIXELS = (0.0, -0.5, np.nan, np.inf)
BAD_RADII = (0.0, -1.0, np.nan, np.inf, None, "3", True)


def test_argument_errors(no_device):
    vol = host_volume()
    ok = torch.zeros(vol.shape, dtype=torch.int32)
    for call in (lambda **k: pipeline.geodesic_zones(vol, k.pop("markers", ok), **k),
                 lambda **k: pipeline.separate_components(vol, k.pop("radius_mm", 2.0), **k)):
        for bad in BAD_DEPTHS:
            with pytest.raises(ValueError):
                call(slice_depths=bad)
        for bad in BAD_PIXELS:
            with pytest.raises(ValueError):
                call(mm_per_pixel_y=bad)
            with pytest.raises(ValueError):
                call(mm_per_pixel_x=bad)
        for bad in (0, 18, 7, None):
            with pytest.raises(ValueError, match="connectivity"):
                call(connectivity=bad)
        with pytest.raises(AssertionError, match="device"):                           # good arguments reach the device
            call(slice_depths=[0.5, 1.0, 2.0], mm_per_pixel_y=0.7)
    for bad in (torch.zeros(vol.shape, dtype=torch.int64), torch.zeros(vol.shape, dtype=torch.float32), np.zeros(vol.shape, dtype=np.int32),
                "markers", None):
        with pytest.raises(TypeError, match="markers"):
            pipeline.geodesic_zones(vol, bad)
    for bad in (torch.zeros((3, 4, 71), dtype=torch.int32), torch.zeros((4, 70), dtype=torch.int32), host_volume((3, 4, 71)),
                host_volume((4, 4, 70))):
        with pytest.raises(ValueError, match="markers"):
            pipeline.geodesic_zones(vol, bad)
    with pytest.raises(AssertionError, match="device"):
        pipeline.geodesic_zones(vol, host_volume())
    for bad in (torch.zeros(vol.shape, dtype=torch.int64), np.zeros(vol.shape, dtype=np.int32), None):
        with pytest.raises(TypeError, match="zones"):
            pipeline.split_zones(vol, bad)
    with pytest.raises(ValueError, match="zones"):
        pipeline.split_zones(vol, torch.zeros((3, 4, 71), dtype=torch.int32))
    for bad in (0, 18, None):
        with pytest.raises(ValueError, match="connectivity"):
            pipeline.split_zones(vol, ok, bad)
    with pytest.raises(AssertionError, match="device"):
        pipeline.split_zones(vol, ok)
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius_mm"):
            pipeline.separate_components(vol, bad)
        with pytest.raises(ValueError, match="radius_mm"):
            volume_calculator.separate_grains(v, 0.9, 0.7, np.ones(3), bad)
        if bad is not None:
            with pytest.raises(ValueError, match="radius_mm"):
                volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), separate_mm=bad)
    for bad in (-1, 2.5, np.nan, "3", True):
        with pytest.raises(ValueError, match="min_marker_voxels"):
            pipeline.separate_components(vol, 2.0, min_marker_voxels=bad)
        with pytest.raises(ValueError, match="min_marker_voxels"):
            volume_calculator.separate_grains(v, 0.9, 0.7, np.ones(3), 2.0, min_marker_voxels=bad)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool)):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.separate_grains(bad, 0.9, 0.7, np.ones(3), 2.0)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            volume_calculator.separate_grains(v, 0.9, 0.7, bad, 2.0)
    with pytest.raises(ValueError, match="connectivity"):
        volume_calculator.separate_grains(v, 0.9, 0.7, np.ones(3), 2.0, connectivity=18)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.separate_grains(v, 0.9, 0.7, np.ones(3), 2.0)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), separate_mm=2.0)


def test_the_volume_budget_raises_before_anything_is_allocated(no_device, monkeypatch):
    """Three per-voxel maps: dist, zones and the marker map."""
    vol = host_volume()
    monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", 12 * 3 * 4 * 70 - 1)
    with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET") as e:
        pipeline.geodesic_zones(vol, torch.zeros(vol.shape, dtype=torch.int32))
    assert all(word in str(e.value) for word in ("distance map", "zone map", "marker map"))
    with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET"):
        pipeline.geodesic_zones(vol, host_volume())
    with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET"):
        pipeline.separate_components(vol, 2.0)
    monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", 12 * 3 * 4 * 70)
    with pytest.raises(AssertionError, match="device"):
        pipeline.geodesic_zones(vol, torch.zeros(vol.shape, dtype=torch.int32))


def test_the_flags_are_off_by_default():
    p = inspect.signature(volume_calculator.component_properties).parameters
    assert p["separate_mm"].default is None
    g = inspect.signature(volume_calculator.separate_grains).parameters
    assert list(g) == ["voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "radius_mm", "connectivity", "min_marker_voxels"]
    assert (g["connectivity"].default, g["min_marker_voxels"].default) == (6, 1)
    z = inspect.signature(pipeline.geodesic_zones).parameters
    assert list(z) == ["vol", "markers", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity"] and z["connectivity"].default == 26
    c = inspect.signature(pipeline.split_zones).parameters
    assert list(c) == ["vol", "zones", "connectivity"] and c["connectivity"].default == 26
    s = inspect.signature(pipeline.separate_components).parameters
    assert list(s) == ["vol", "radius_mm", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "min_marker_voxels"]
    assert (s["connectivity"].default, s["min_marker_voxels"].default) == (6, 1)
    assert [f.name for f in pipeline.Separation.__dataclass_fields__.values()] == ["volume", "markers", "cut_voxels", "zones", "sweeps"]
