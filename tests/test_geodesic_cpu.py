"""CPU tier of the geodesic distance: the reference (tests/geodesic_reference.py) against itself in another order -- the claim
the tiled kernel rests on: every order of relaxations ends at the same bytes --, locality (the whole-volume map under a
component is the map of that component alone), the weight tables of the product against the reference's, rods and the coil, and
the plumbing (exports, argument checks before any device use, flags off by default).  None of it needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caliper_reference as F  # noqa: E402
import components_reference as C  # noqa: E402
import geodesic_reference as G  # noqa: E402
import test_abi  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

FIXTURES = G.fixtures()
NEW_SYMBOLS = ("tomo_geo_tiles", "tomo_geo_seed_bits", "tomo_geo_seed_index", "tomo_geo_sweep", "tomo_geo_reach")
SMALL = ("words_65", "one_voxel", "corner", "edge", "tie", "serpentine", "snake3d", "comb", "ring", "coil", "weave")    # the in-place Python sweeps are slow


def test_fixtures():
    assert list(FIXTURES)[:len(C.fixtures())] == list(C.fixtures())
    assert list(FIXTURES)[-5:] == ["noise_tiles", "noise_words", "weave", "coil", "ring"]
    assert FIXTURES["noise_tiles"].shape == (9, 17, 65) and FIXTURES["noise_words"].shape == (17, 9, 130)
    assert FIXTURES["weave"].shape == (2, 20, 130) and FIXTURES["coil"].shape == (12, 24, 70)
    for name in ("weave", "coil", "ring"):
        for conn in C.CONNECTIVITIES:
            assert C.label(FIXTURES[name], conn)[1] == 1, (name, conn)
    w = FIXTURES["weave"]                                                            # it crosses the three kinds of tile face often
    assert (w[0, 7] & w[0, 8]).sum() >= 60 and (w[0, :, 63] & w[0, :, 64]).sum() >= 5 and (w[0, 2] & w[1, 2]).sum() >= 60


# ------------------------------------------------------------------ the weights
@pytest.mark.parametrize("kind", G.KINDS)
def test_weights_equal_the_reference(kind):
    for nz in (1, 2, 3, 9, 17):
        depths, mm_y, mm_x = T.spacing(kind, nz)
        wxy, wz = pipeline.geodesic_weights(depths, nz, mm_y, mm_x)
        rxy, rz = G.weights((nz, 4, 5), kind)
        assert wxy.dtype == np.float32 and wxy.shape == (3,) and wz.dtype == np.float32 and wz.shape == (max(nz - 1, 1), 4)
        assert wxy.tobytes() == rxy.tobytes() and wz.tobytes() == rz.tobytes(), (kind, nz)
    wxy, wz = pipeline.geodesic_weights(None, 3)
    s2, s3 = np.float32(np.sqrt(2.0)), np.float32(np.sqrt(3.0))
    assert wxy.tolist() == [1.0, 1.0, s2] and wz.tolist() == [[1.0, s2, s2, s3]] * 2


# ------------------------------------------------------------------ order independence
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_every_order_of_relaxations_ends_at_the_same_bytes(conn, kind):
    """Dijkstra (ascending distance) and Bellman-Ford (raster and anti-raster sweeps in place) to a fixed point."""
    for name in SMALL:
        v = FIXTURES[name]
        w = G.weights(v.shape, kind)
        seeds = G.default_seeds(v, 41)
        a = G.dijkstra(v, seeds, *w, conn)
        b, sweeps = G.bellman_ford(v, seeds, *w, conn)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), (name, conn, kind)
        assert np.isinf(a[~v]).all() and (a[G.seeds_mask(v.shape, seeds) & v] == 0).all()
        assert sweeps >= (3 if name in ("weave", "coil", "ring") else 1), (name, sweeps)   # the paths run against the raster order


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_locality(conn):
    """The whole-volume multi-source map under a component is the map of the mask `labels == c` alone."""
    for name, kind in (("noise_031", "sided"), ("corner", "unit"), ("tie", "dyadic"), ("noise_tiles", "sided")):
        v = FIXTURES[name]
        w = G.weights(v.shape, kind)
        labels, n = C.label(v, conn)
        seeds = G.default_seeds(v, 23)
        whole = G.dijkstra(v, seeds, *w, conn)
        sizes = C.sizes(labels, n)
        for c in (np.argsort(-sizes, kind="stable")[:4] + 1):
            mask = labels == c
            alone = G.dijkstra(mask, seeds, *w, conn)
            assert alone[mask].tobytes() == whole[mask].tobytes(), (name, conn, int(c))
        reached = G.reach(v, whole)
        touched = np.unique(labels[G.seeds_mask(v.shape, seeds) & v])
        assert np.array_equal(reached, np.isin(labels, touched) & v)                  # reconstruction: the components a seed touches


# ------------------------------------------------------------------ rods, the coil, the ring
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_rod_reads_the_integers(axis, conn):
    v = G.rod(axis, 11)
    start = [1, 1, 1]
    d = G.dijkstra(v, [start], *G.weights(v.shape, "unit"), conn)
    assert d[v].tolist() == [float(i) for i in range(11)]
    rows, _ = G.per_component(v, conn, "unit", sweeps=2)
    far = list(start)
    far[axis] = 11
    assert len(rows) == 1 and rows[0]["length_mm"] == 10.0 and rows[0]["chord_mm"] == 10.0 and rows[0]["tortuosity"] == 1.0
    assert sorted(rows[0]["ends_index"]) == sorted([tuple(start), tuple(far)])
    rows, _ = G.per_component(np.ones((1, 1, 1), dtype=bool), conn, "unit")
    assert rows[0]["length_mm"] == 0.0 and rows[0]["tortuosity"] == 1.0 and rows[0]["ends_index"] == [(0, 0, 0), (0, 0, 0)]


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_the_coil_is_longer_than_it_is_wide(conn):
    v = FIXTURES["coil"]
    rows, _ = G.per_component(v, conn, "unit")
    labels, n = C.label(v, conn)
    feret = F.caliper(labels, n, F.Grid(v.shape, "unit"), F.direction_sets()["d64"], "voxels")
    assert len(rows) == 1 and rows[0]["tortuosity"] > 2.0
    assert rows[0]["length_mm"] > feret["max_mm"][0] and rows[0]["length_mm"] > 2.0 * feret["max_mm"][0]
    two, _ = G.per_component(v, conn, "unit", sweeps=2)
    assert two[0]["length_mm"] <= rows[0]["length_mm"]                                # every search is a lower bound, and they rise


def test_the_ring():
    rows, _ = G.per_component(FIXTURES["ring"], 6, "unit")
    assert rows[0]["length_mm"] == 36.0 and rows[0]["voxels"] == 72                  # half way round


# ------------------------------------------------------------------ the plumbing
def test_exports_and_signatures():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert [s for s in syms if s.startswith("tomo_geo_")] == sorted(NEW_SYMBOLS)
    assert {"geodesic_sweeps", "geodesic_calls"} <= set(pipeline.COUNTERS)
    assert (pipeline.GEODESIC_SWEEP_BATCH, pipeline.GEODESIC_SWEEP_LIMIT, pipeline.GEODESIC_VOLUME_BUDGET) == (8, 1 << 16, 1 << 33)


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(8)]
    a, b, c, d, e, f, g, h = (ctypes.addressof(x) for x in bufs)                      # distinct host buffers, never dereferenced
    assert L.tomo_geo_tiles(8, 8, 64) == 1 and L.tomo_geo_tiles(9, 17, 65) == 12 and L.tomo_geo_tiles(1, 1, 1) == 1
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        assert L.tomo_geo_tiles(*bad) == -1
        assert L.tomo_geo_seed_bits(a, b, *bad, c, d, None) == -1
        assert L.tomo_geo_seed_index(a, *bad, b, None, 1, c, d, e, None) == -1
        assert L.tomo_geo_sweep(a, *bad, 6, b, c, d, e, f, g, None) == -1
        assert L.tomo_geo_reach(a, b, *bad, 1.0, c, None) == -1
    assert L.tomo_geo_tiles(1 << 15, 1 << 15, 1 << 15) == -3                         # 2^31 tiles and more
    assert L.tomo_geo_tiles(1 << 12, 1 << 13, 1 << 12) == -3                         # 2^31 words
    for k in range(4):
        args = [a, b, 4, 4, 4, c, d]
        args[(0, 1, 5, 6)[k]] = None
        assert L.tomo_geo_seed_bits(*args, None) == -1
    for k in (0, 4, 7, 8, 9):
        args = [a, 4, 4, 4, b, None, 3, c, d, e]
        args[k] = None
        assert L.tomo_geo_seed_index(*args, None) == -1
    assert L.tomo_geo_seed_index(a, 4, 4, 4, b, None, 0, c, d, e, None) == -1
    assert L.tomo_geo_seed_index(a, 4, 4, 4, b, None, -2, c, d, e, None) == -1
    good = [a, 4, 4, 4, 26, b, c, d, e, f, g]
    for k in (0, 5, 6, 7, 8, 9, 10):
        args = list(good)
        args[k] = None
        assert L.tomo_geo_sweep(*args, None) == -1
    for conn in (0, 4, 8, 18, 27, -6):
        assert L.tomo_geo_sweep(a, 4, 4, 4, conn, b, c, d, e, f, g, None) == -1
    assert L.tomo_geo_sweep(a, 4, 4, 4, 6, b, c, d, e, e, g, None) == -1             # one array for both sets of flags
    assert L.tomo_geo_sweep(a, 1 << 12, 1 << 13, 1 << 12, 6, b, c, d, e, f, g, None) == -3
    for k in (0, 1, 6):
        args = [a, b, 4, 4, 4, 1.0, c]
        args[k] = None
        assert L.tomo_geo_reach(*args, None) == -1
    assert L.tomo_geo_reach(a, b, 4, 4, 4, -1.0, c, None) == -1
    assert L.tomo_geo_reach(a, b, 4, 4, 4, float("nan"), c, None) == -1
    assert L.tomo_geo_reach(a, b, 4, 4, 4, 1.0, a, None) == -1


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
BAD_SEEDS = (host_volume((3, 4, 71)), host_volume((4, 4, 70)), np.zeros((2, 2), dtype=np.int64), np.zeros(3, dtype=np.int64),
             np.zeros((1, 3)), [[0, 0, 70]], [[3, 0, 0]], [[0, -1, 0]], "seeds")


def test_argument_errors(no_device):
    vol = host_volume()
    ok = np.array([[0, 0, 0]])
    for call in (lambda **k: pipeline.geodesic_distance(vol, k.pop("seeds", ok), **k),
                 lambda **k: pipeline.geodesic_reach(vol, k.pop("seeds", ok), **k),
                 lambda **k: pipeline.component_geodesic(vol, **k), lambda **k: pipeline.cavity_geodesic(vol, **k)):
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
    for bad in BAD_SEEDS:
        with pytest.raises(ValueError, match="seed"):
            pipeline.geodesic_distance(vol, bad)
        with pytest.raises(ValueError, match="seed"):
            pipeline.geodesic_reach(vol, bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_mm"):
            pipeline.geodesic_reach(vol, ok, bad)
    for bad in (1, 0, -3, 2.5, None, True, "3"):
        with pytest.raises(ValueError, match="sweeps"):
            pipeline.component_geodesic(vol, sweeps=bad)
        with pytest.raises(ValueError, match="sweeps"):
            pipeline.cavity_geodesic(vol, sweeps=bad)
        with pytest.raises(ValueError, match="sweeps"):
            volume_calculator.component_properties(np.ones((3, 4, 5), dtype=bool), 0.9, 0.7, np.ones(3), geodesic=True, geodesic_sweeps=bad)
    for bad in (-1, 2.5, np.nan, "3", True):
        with pytest.raises(ValueError, match="min_voxels"):
            pipeline.cavity_geodesic(vol, min_voxels=bad)
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool)):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.component_properties(bad, 0.9, 0.7, np.ones(3), geodesic=True)
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.closed_porosity(bad, 0.9, 0.7, np.ones(3), pore_geodesic=True)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            volume_calculator.component_properties(v, 0.9, 0.7, bad, geodesic=True)
        with pytest.raises(ValueError):
            volume_calculator.closed_porosity(v, 0.9, 0.7, bad, pore_geodesic=True)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), geodesic=True)


def test_the_volume_budget_raises_before_anything_is_allocated(no_device, monkeypatch):
    monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", 4 * 3 * 4 * 70 - 1)
    tables = pipeline._geodesic_tables((3, 4, 70), None, 1.0, 1.0)
    with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET"):
        pipeline._GeodesicPlan(host_volume(), tables, 26)


def test_the_flags_are_off_by_default():
    p = inspect.signature(volume_calculator.component_properties).parameters
    assert p["geodesic"].default is False and p["geodesic_sweeps"].default == 3
    assert inspect.signature(volume_calculator.closed_porosity).parameters["pore_geodesic"].default is False
    r = inspect.signature(pipeline.component_geodesic).parameters
    assert list(r) == ["vol", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "sweeps", "min_voxels", "largest"]
    assert (r["connectivity"].default, r["sweeps"].default, r["min_voxels"].default, r["largest"].default) == (6, 3, 0, False)
    s = inspect.signature(pipeline.ComponentRuns.geodesic).parameters
    assert list(s) == ["self", "slice_depths", "mm_y", "mm_x", "sweeps", "min_voxels", "largest", "max_voxels", "enclosed"]
    assert s["max_voxels"].kind is inspect.Parameter.KEYWORD_ONLY and s["enclosed"].kind is inspect.Parameter.KEYWORD_ONLY
    d = inspect.signature(pipeline.geodesic_distance).parameters
    assert list(d) == ["vol", "seeds", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity"] and d["connectivity"].default == 26
    q = inspect.signature(pipeline.geodesic_reach).parameters
    assert list(q) == ["vol", "seeds", "max_mm", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity"]


def test_zero_rows_have_the_declared_dtypes():
    tables = pipeline._geodesic_tables((3, 4, 70), None, 1.0, 1.0)
    t = pipeline._component_geodesic_from(tables, np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4), dtype=np.int64))
    want = {"labels": (np.int64, (0,)), "voxels": (np.int64, (0,)), "length_mm": (np.float64, (0,)), "ends_index": (np.int64, (0, 2, 3)),
            "ends_mm": (np.float64, (0, 2, 3)), "chord_mm": (np.float64, (0,)), "tortuosity": (np.float64, (0,))}
    assert isinstance(t, pipeline.ComponentGeodesic) and len(t) == 0
    assert {k: (getattr(t, k).dtype, getattr(t, k).shape) for k in want} == want
