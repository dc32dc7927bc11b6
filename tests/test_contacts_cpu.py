"""CPU tier of the contact table between zones: the reference (tests/contacts_reference.py) against the definition computed
another way, its totals, the area of a flat interface, and the plumbing (exports, argument checks before any device use,
signatures, the host arithmetic of ZoneContacts).  None of it needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_reference as R  # noqa: E402
import surface_reference as S  # noqa: E402
import test_abi  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

NEW_SYMBOLS = ("tomo_contact_count", "tomo_contact_insert", "tomo_contact_hist", "tomo_contact_finish")
SHAPE = (6, 7, 9)


def small_case(seed=11):
    rng = np.random.default_rng(seed)
    v = rng.random(SHAPE) < 0.7
    zones = rng.integers(-1, 5, SHAPE).astype(np.int32)            # -1 and 0 take no part, entries on unset voxels neither
    return v, zones


def factors(kind, nz, directions=13):
    depths, mm_y, mm_x = T.spacing(kind, nz)
    return pipeline.surface_factors(depths, nz, mm_y, mm_x, directions)


# ------------------------------------------------------------------ the reference against the definition
def test_the_reference_against_a_triple_loop_over_all_26_neighbours():
    v, zones = small_case()
    assert ((zones > 0) & ~v).any() and ((zones <= 0) & v).any()
    t = R.contacts(v, zones, factors("unit", SHAPE[0]))
    want = R.brute(v, zones)
    assert len(want) >= 5 and [(int(a), int(b)) for a, b in zip(t["zone_a"], t["zone_b"])] == sorted(want)
    for r, key in enumerate(sorted(want)):
        assert (int(t["pairs"][r]), t["pair_counts"][r].tolist()) == want[key], key
    assert (t["slice_counts"].sum(axis=1) == t["pair_counts"]).all() and (t["pair_counts"].sum(axis=1) == t["pairs"]).all()
    for kind, directions in (("unit", 13), ("sided", 13), ("sided", 3)):                        # the sum, row by row and side by side
        F = factors(kind, SHAPE[0], directions)
        want_area = [R.area_of(t["slice_counts"][r], F, directions) for r in range(len(t["pairs"]))]
        assert R.areas(t["slice_counts"], F, directions).tolist() == want_area and max(want_area) > 0.0
    assert (t["z_range"][:, 0] <= t["z_range"][:, 1]).all() and t["z_range"].max() <= SHAPE[0] - 1
    z = R.labels_of(v, zones)
    for r in range(len(t["pairs"])):                                 # the first voxel takes part and lies in one of the two zones
        k, j, i = t["first_index"][r]
        assert z[k, j, i] in (t["zone_a"][r], t["zone_b"][r]) and t["z_range"][r, 0] == k


def test_the_counts_of_all_rows_add_up_to_the_unlike_adjacent_pairs():
    v, zones = small_case(12)
    z = np.pad(R.labels_of(v, zones), 1)
    core = z[1:-1, 1:-1, 1:-1]
    twice = 0
    for dz, dy, dx in S.STEPS:
        q = z[1 + dz:1 + dz + SHAPE[0], 1 + dy:1 + dy + SHAPE[1], 1 + dx:1 + dx + SHAPE[2]]
        twice += int(((core > 0) & (q > 0) & (q != core)).sum())
    for conn in (26, 6):
        t = R.contacts(v, zones, factors("unit", SHAPE[0]), connectivity=conn)
        if conn == 26:
            assert twice % 2 == 0 and int(t["pairs"].sum()) == twice // 2 > 100
        else:                                                        # the rows that share a face, with the same bytes
            whole = R.contacts(v, zones, factors("unit", SHAPE[0]))
            keep = whole["pair_counts"][:, [0, 1, 3]].sum(axis=1) > 0
            assert all(np.array_equal(t[name], whole[name][keep]) for name in whole)


def test_a_row_never_sees_the_end_of_the_previous_row():
    v = np.zeros((2, 4, 5), dtype=bool)
    zones = np.zeros(v.shape, dtype=np.int32)
    v[0, 1, 4] = v[0, 2, 0] = v[0, 3, 4] = v[1, 0, 0] = True        # ends of rows and of a slice: flat neighbours, not lattice neighbours
    zones[0, 1, 4], zones[0, 2, 0], zones[0, 3, 4], zones[1, 0, 0] = 1, 2, 3, 4
    assert len(R.contacts(v, zones, factors("unit", 2))["pairs"]) == 0
    v[0, 2, 4], zones[0, 2, 4] = True, 5                            # a lattice neighbour of both ends in column 4
    t = R.contacts(v, zones, factors("unit", 2))
    assert list(zip(t["zone_a"].tolist(), t["zone_b"].tolist())) == [(1, 5), (3, 5)] and t["pair_counts"][:, 1].tolist() == [1, 1]


@pytest.mark.parametrize("kind", ["unit", "sided"])
def test_the_area_of_a_flat_interface(kind):
    """An (8, 8, 8) block cut into two zones by a plane through its middle, directions = 13, against the plane's true area.  The
    estimator is surface_area's, and so is its bias on a flat axis-aligned face: every face of the plane is crossed by one axis
    line, but the diagonal lines through the voxels at the rim of the stack are missing.  Measured here from the reference, as
    the share of the true area: unit spacing 0.7981 for each of the three planes (the closed form below; an unbounded plane
    reads 0.9266, surface_area's 8^3 cube with its shared edges 0.8615); sided spacing 0.7153 (z), 0.7867 (y), 0.7886 (x).  The
    tolerance is that bias: the estimate lies below the true area by at most 0.2019 (unit) and 0.2847 (sided)."""
    shape = (8, 8, 8)
    depths, mm_y, mm_x = T.spacing(kind, shape[0])
    d = np.ones(shape[0]) if depths is None else np.asarray(depths, dtype=np.float64)
    F = pipeline.surface_factors(depths, shape[0], mm_y, mm_x, 13)
    true = (shape[1] * mm_y * shape[2] * mm_x, d.sum() * shape[2] * mm_x, d.sum() * shape[1] * mm_y)
    for axis in range(3):
        v, zones = R.halves(shape, axis, shape[axis] // 2)
        t = R.contacts(v, zones, F)
        assert len(t["pairs"]) == 1 and (t["zone_a"][0], t["zone_b"][0]) == (1, 2) and t["pairs"][0] == 64 + 4 * 56 + 4 * 49
        share = float(t["area_mm2"][0]) / true[axis]
        print("%s, plane across axis %d: %.4f of the true area" % (kind, axis, share))
        assert 0.0 < 1.0 - share <= (0.2019 if kind == "unit" else 0.2847) + 5e-5
        if kind == "unit":                                           # 64 faces, 2 * 2 * 56 edge diagonals, 4 * 49 corner diagonals
            w = S.CUBIC
            closed = (64 * 2 * w[0] + 224 * 2 * w[1] / np.sqrt(2.0) + 196 * 2 * w[2] / np.sqrt(3.0)) / 64
            assert abs(share - closed) < 1e-9 and abs(closed - 0.7981) < 5e-5
    t3 = R.contacts(v, zones, pipeline.surface_factors(depths, shape[0], mm_y, mm_x, 3), directions=3)
    assert abs(float(t3["area_mm2"][0]) / true[2] - 2.0 / 3.0) < 1e-12                # directions = 3: two thirds of the faces


def test_values_and_paths_of_the_reference():
    v, zones = R.halves((3, 4, 6), 2, 3)
    values = np.zeros(v.shape, dtype=np.float32)
    values[1, 2, 2] = values[2, 1, 3] = 2.5                         # a tie on the interface: the lower index wins
    values[0, 0, 0] = 9.0                                           # not on the interface
    dist = np.full(v.shape, np.inf, dtype=np.float32)
    dist[:, :, 2], dist[:, :, 3] = 2.0, 1.0
    dist[0, 0, 2] = 0.5
    wxy, wz = np.array([1.0, 1.0, 1.5], dtype=np.float32), np.full((2, 4), 2.0, dtype=np.float32)
    t = R.contacts(v, zones, factors("unit", 3), values=values, dist=dist, weights=(wxy, wz))
    assert t["value_max"].dtype == np.float32 and t["value_max"].tolist() == [2.5] and t["value_index"].tolist() == [[1, 2, 2]]
    assert t["path_mm"].dtype == np.float32 and t["path_mm"].tolist() == [2.5]                 # 0.5 + 1.0 + 1.0 along x
    none = R.contacts(v, zones, factors("unit", 3), dist=np.full(v.shape, np.inf, dtype=np.float32), weights=(wxy, wz))
    assert np.isinf(none["path_mm"]).all()


# ------------------------------------------------------------------ the plumbing
def test_exports_and_signatures():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert [s for s in syms if s.startswith("tomo_contact_")] == sorted(NEW_SYMBOLS)
    assert {"zone_contacts", "contact_launches"} <= set(pipeline.COUNTERS)
    assert pipeline.CONTACT_TABLE_BUDGET == 1 << 30


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(16)]
    p = [ctypes.addressof(x) for x in bufs]                           # distinct host buffers, never dereferenced
    count = lambda *shape: [p[0], p[1], *shape, p[2]]                                                         # noqa: E731
    insert = lambda *shape: [p[0], p[1], *shape, p[2], p[3], p[4], p[5], 64, p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13]]   # noqa: E731
    hist = lambda *shape: [p[0], p[1], *shape, p[2], 64, p[3], p[4], p[5], p[6], p[7], 5, p[8], 9, p[9], p[10]]      # noqa: E731
    finish = [5, p[0], 64, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], 9, p[11], 4, 13, p[12], p[13]]
    calls = ((L.tomo_contact_count, count), (L.tomo_contact_insert, insert), (L.tomo_contact_hist, hist))
    for fn, make in calls:
        for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
            assert fn(*make(*bad), None) == -1
        assert fn(*make(1 << 12, 1 << 13, 1 << 12), None) == -3       # 2^31 words
        assert fn(*make(1 << 15, 1 << 15, 1 << 15), None) == -3
        good = make(4, 4, 4)
        for k, a in enumerate(good):
            if a in p[:2]:                                           # bits and zones are never optional
                args = list(good)
                args[k] = None
                assert fn(*args, None) == -1
        args = list(good)
        args[1] = args[0]                                            # the map over the bits
        assert fn(*args, None) == -1
    # insert: every output is needed, none may alias another or an input; the optional maps come with their outputs
    good = insert(4, 4, 4)
    for k in (10, 11, 12, 13, 14, 17):
        args = list(good)
        args[k] = None
        assert L.tomo_contact_insert(*args, None) == -1
    for k, other in ((10, 11), (12, 13), (14, 10), (15, 16), (17, 10), (10, 0), (15, 5)):
        args = list(good)
        args[k] = args[other]
        assert L.tomo_contact_insert(*args, None) == -1
    for k in (15, 16, 7, 8):                                         # values without value_max, dist without path or weights
        args = list(good)
        args[k] = None
        assert L.tomo_contact_insert(*args, None) == -1
    for cap, code in ((0, -1), (-64, -1), (48, -1), (65, -1), (1 << 31, -3), (1 << 40, -3)):
        args = list(good)
        args[9] = cap
        assert L.tomo_contact_insert(*args, None) == code
        args = list(hist(4, 4, 4))
        args[6] = cap
        assert L.tomo_contact_hist(*args, None) == code
        args = list(finish)
        args[2] = cap
        assert L.tomo_contact_finish(*args, None) == code
    # hist
    good = hist(4, 4, 4)
    for k in (7, 8, 9, 11, 13, 16):
        args = list(good)
        args[k] = None
        assert L.tomo_contact_hist(*args, None) == -1
    for k, v in ((12, 0), (12, -1), (12, 65), (14, 0), (14, -3)):   # rows and entries positive, no more rows than slots
        args = list(good)
        args[k] = v
        assert L.tomo_contact_hist(*args, None) == -1
    args = list(good)
    args[14] = 1 << 60
    assert L.tomo_contact_hist(*args, None) == -3
    for k, other in ((13, 7), (15, 13), (16, 13), (13, 0)):
        args = list(good)
        args[k] = args[other]
        assert L.tomo_contact_hist(*args, None) == -1
    args = list(good)
    args[15] = None                                                  # values without value_index
    assert L.tomo_contact_hist(*args, None) == -1
    # finish
    for k in (1, 3, 4, 5, 6, 7, 11, 12, 14, 17, 18):
        args = list(finish)
        args[k] = None
        assert L.tomo_contact_finish(*args, None) == -1
    for k, v in ((0, 0), (0, -2), (0, 65), (13, 0), (15, 0), (16, 6), (16, 26)):
        args = list(finish)
        args[k] = v
        assert L.tomo_contact_finish(*args, None) == -1
    args = list(finish)
    args[13] = 1 << 60
    assert L.tomo_contact_finish(*args, None) == -3
    for k, other in ((17, 12), (17, 3), (18, 17)):
        args = list(finish)
        args[k] = args[other]
        assert L.tomo_contact_finish(*args, None) == -1
    args = list(finish)
    args[10] = None                                                  # value_max without value_index
    assert L.tomo_contact_finish(*args, None) == -1


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


def test_argument_errors(no_device):
    vol = host_volume()
    ok = torch.zeros(vol.shape, dtype=torch.int32)
    fine = torch.zeros(vol.shape, dtype=torch.float32)
    for call in (lambda **k: pipeline.zone_contacts(vol, k.pop("zones", ok), **k),
                 lambda **k: pipeline.separate_with_contacts(vol, 2.0, **k)):
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
        for bad in (0, 6, 26, None):
            with pytest.raises(ValueError, match="directions"):
                call(directions=bad)
        with pytest.raises(AssertionError, match="device"):           # good arguments reach the device
            call(slice_depths=[0.5, 1.0, 2.0], mm_per_pixel_y=0.7, directions=3)
    for bad in (torch.zeros(vol.shape, dtype=torch.int64), fine, np.zeros(vol.shape, dtype=np.int32), None):
        with pytest.raises(TypeError, match="zones"):
            pipeline.zone_contacts(vol, bad)
    for bad in (torch.zeros((3, 4, 71), dtype=torch.int32), torch.zeros((4, 70), dtype=torch.int32)):
        with pytest.raises(ValueError, match="zones"):
            pipeline.zone_contacts(vol, bad)
    for name in ("values", "dist"):
        for bad in (torch.zeros(vol.shape, dtype=torch.float64), ok, np.zeros(vol.shape, dtype=np.float32), "map"):
            with pytest.raises(TypeError, match=name):
                pipeline.zone_contacts(vol, ok, **{name: bad})
        with pytest.raises(ValueError, match=name):
            pipeline.zone_contacts(vol, ok, **{name: torch.zeros((3, 4, 71), dtype=torch.float32)})
    with pytest.raises(AssertionError, match="device"):
        pipeline.zone_contacts(vol, ok, values=fine, dist=fine)
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in (0.0, -1.0, np.nan, None, "3", True):
        with pytest.raises(ValueError, match="radius_mm"):
            pipeline.separate_with_contacts(vol, bad)
        with pytest.raises(ValueError, match="radius_mm"):
            volume_calculator.grain_contacts(v, 0.9, 0.7, np.ones(3), bad)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="min_marker_voxels"):
            volume_calculator.grain_contacts(v, 0.9, 0.7, np.ones(3), 2.0, min_marker_voxels=bad)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool), [[[True]]]):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.grain_contacts(bad, 0.9, 0.7, np.ones(3), 2.0)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            volume_calculator.grain_contacts(v, 0.9, 0.7, bad, 2.0)
    with pytest.raises(ValueError, match="connectivity"):
        volume_calculator.grain_contacts(v, 0.9, 0.7, np.ones(3), 2.0, connectivity=18)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.grain_contacts(v, 0.9, 0.7, np.ones(3), 2.0)


def test_the_capacity_of_the_table(monkeypatch):
    assert pipeline._contact_capacity(1) == 64 and pipeline._contact_capacity(32) == 64 and pipeline._contact_capacity(33) == 128
    assert pipeline._contact_capacity(45000) == 131072
    assert pipeline._contact_capacity(10 ** 12) == 1 << 24             # 2^30 bytes hold 2^24 slots of 44 bytes, not 2^25
    monkeypatch.setattr(pipeline, "CONTACT_TABLE_BUDGET", 44 * 1024 - 1)
    assert pipeline._contact_capacity(45000) == 512 and pipeline._contact_capacity(10) == 64
    monkeypatch.setattr(pipeline, "CONTACT_TABLE_BUDGET", 43)
    with pytest.raises(_lib.TomoError, match="CONTACT_TABLE_BUDGET"):
        pipeline._contact_capacity(10)
    monkeypatch.setattr(pipeline, "CONTACT_TABLE_BUDGET", 1 << 50)
    assert pipeline._contact_capacity(10 ** 12) == 1 << 30             # what the kernels index


def test_signatures_and_defaults():
    z = inspect.signature(pipeline.zone_contacts).parameters
    assert list(z) == ["vol", "zones", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "directions", "values", "dist"]
    assert (z["slice_depths"].default, z["connectivity"].default, z["directions"].default, z["values"].default, z["dist"].default) == (
        None, 26, 13, None, None)
    g = inspect.signature(volume_calculator.grain_contacts).parameters
    assert list(g) == ["voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "radius_mm", "connectivity", "min_marker_voxels"]
    assert (g["connectivity"].default, g["min_marker_voxels"].default) == (6, 1)
    s = inspect.signature(pipeline.separate_with_contacts).parameters
    assert list(s)[:7] == list(inspect.signature(pipeline.separate_components).parameters) and s["directions"].default == 13
    assert [f.name for f in pipeline.ZoneContacts.__dataclass_fields__.values()] == [
        "zone_a", "zone_b", "pairs", "pair_counts", "area_mm2", "z_range", "first_index", "value_max", "value_index", "path_mm"]


def test_coordination_is_host_arithmetic_over_the_rows():
    v, zones = small_case(13)
    t = R.contacts(v, zones, factors("sided", SHAPE[0]))
    c = pipeline.ZoneContacts(t["zone_a"], t["zone_b"], t["pairs"], t["pair_counts"], t["area_mm2"], t["z_range"], t["first_index"])
    assert len(c) == len(t["pairs"]) >= 5 and c.value_max is None and c.path_mm is None
    for labels in (None, np.array([9, 4, 1, 77, 2]), np.arange(1, 5)):
        got = c.coordination(labels)
        want = R.coordination(t, labels)
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), labels
    labels, n, area = c.coordination(np.array([77, 1]))
    assert n[0] == 0 and area[0] == 0.0 and n[1] == int(((t["zone_a"] == 1) | (t["zone_b"] == 1)).sum())
    assert c.coordination()[1].sum() == 2 * len(c)
    with pytest.raises(ValueError, match="distinct"):
        c.coordination([1, 2, 1])
    empty = pipeline._empty_contacts(None, None)
    assert len(empty) == 0 and empty.pair_counts.shape == (0, 7) and empty.first_index.shape == (0, 3)
    assert [a.tolist() for a in empty.coordination([3, 1])] == [[3, 1], [0, 0], [0.0, 0.0]] and len(empty.coordination()[0]) == 0
