"""CPU tier of the per-component inscribed sphere and local thickness: the claim the GPU path rests on -- distance and local
thickness are local to a component, so the arrays of the whole volume under the mask of a component are the arrays of that
mask -- held bit for bit with one NumPy transform per component; the condition on the radii that lets the GPU tier demand
equality; and the plumbing (exports, argument checks before any device use, flags off by default).  None of it needs a GPU."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import component_thickness_reference as R  # noqa: E402
import components_reference as C  # noqa: E402
import edt_reference as E  # noqa: E402
import test_abi  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

FIXTURES = R.fixtures()
NEW_SYMBOLS = ("tomo_cc_value_max", "tomo_cc_value_first", "tomo_cc_value_rows", "tomo_cc_level_hist", "tomo_cc_level_sums")


def test_fixtures():
    assert list(FIXTURES) == ["grains", "dumbbell", "shell", "edge", "one", "empty", "full"]
    g = FIXTURES["grains"]
    assert g.shape == (9, 14, 131) and g.dtype == bool and g.sum() <= 6500 and np.array_equal(R.grains(), g)       # seeded
    l6, n6 = C.label(g, 6)
    l26, n26 = C.label(g, 26)
    assert n6 > n26 > 50 and (C.sizes(l6, n6) == 1).sum() > 50                    # many one-voxel components
    a, b = l6[1, 7, 2], l6[3, 9, 4]                                               # the corner contact: (2, 8, 3) and (3, 9, 4)
    assert a and b and a != b and l26[1, 7, 2] == l26[3, 9, 4] and C.sizes(l6, n6)[a - 1] == C.sizes(l6, n6)[b - 1] == 8
    assert len(set(l6[6, 3, 8:13]) | set(l6[6, 2, 16:22])) == 2 and 0 not in set(l6[6, 3, 8:13])       # two components, one word
    bar = l6[7, 11, 0]
    assert bar and l6[7, 11, 130] == bar and (l6[:, :, 0] == bar).any() and (l6[:, :, 130] == bar).any()       # touches x = 0 and x = 130
    assert (g[:, :, 60:68].all(axis=2) & g[:, :, 124:131].all(axis=2)).any()         # one run across the words at 64 and 128
    box = l6[4, 2, 41]
    dist = E.edt(g, *T.tables(g.shape, "unit"))
    top = np.argwhere((l6 == box) & (dist == dist[l6 == box].max()))
    assert len(set(top[:, 0])) == 2 and len(set(top[:, 1])) == 2 and top[:, 2].min() < 64 < top[:, 2].max()        # the plateau
    p = R.pore_box()
    for conn in C.CONNECTIVITIES:
        rows = R.enclosed(p, conn, "unit")
        assert [(r["voxels"], r["radius_mm"]) for r in rows] == [(27, 2.0), (64, 1.0)]   # the cube and the crack: sizes apart
        assert len(R.enclosed(T.fixtures()["shell"], conn, "unit")) == 1


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_distance_and_levels_are_local_to_a_component(conn, kind):
    """edt_squared and by_levels of the mask of EVERY component of grains == the whole-volume arrays under the mask, bit for
    bit: what one transform for all components rests on."""
    v = FIXTURES["grains"]
    radii = np.asarray(R.RADII[kind], dtype=np.float64)
    tabs, d2, level = R.whole(v, kind, radii)
    labels, n = C.label(v, conn)
    assert n > 100
    bad = []
    for c in range(1, n + 1):
        mask = labels == c
        own = E.edt_squared(mask, *tabs, True)
        if own[mask].tobytes() != d2[mask].tobytes() or own[~mask].any():
            bad.append((c, "d2"))
        if not np.array_equal(T.by_levels(mask, own, tabs, radii * radii), level * mask):
            bad.append((c, "level"))
    assert not bad, bad[:10]


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_cavities_are_local_too(conn):
    """The same for an enclosed cavity as a component of the complement: the virtual sites outside the stack never decide."""
    for name, v in R.pore_fixtures().items():
        outside = ~v
        tabs, d2, level = R.whole(outside, "sided", R.RADII["sided"])
        labels, n = C.label(outside, 32 - conn)
        radii = np.asarray(R.RADII["sided"])
        rows = R.enclosed(v, conn, "sided")
        assert rows
        for r in rows:
            mask = labels == r["label"]
            own = E.edt_squared(mask, *tabs, True)
            assert own[mask].tobytes() == d2[mask].tobytes(), (name, r["label"])
            assert np.array_equal(T.by_levels(mask, own, tabs, radii * radii), level * mask), (name, r["label"])


@pytest.mark.parametrize("name", list(FIXTURES) + ["pores:shell", "pores:pore_box"])
def test_inputs_are_off_the_sided_radii(name):
    """A condition on the INPUTS (tests/test_gpu_thickness.py, check_inputs_off_the_radii): no reference D2 of a set voxel and no
    outside squared distance to an eroded set lies within 1e-9 r^2 of an r^2, so the 1 ulp the transform is free in cannot move
    a decision and the GPU tier can demand equality."""
    v = ~R.pore_fixtures()[name[6:]] if name.startswith("pores:") else FIXTURES[name]
    tabs = T.tables(v.shape, "sided")
    d2 = E.edt_squared(v, *tabs, True)
    for r in R.RADII["sided"]:
        r2 = r * r
        assert not (np.abs(d2[v] - r2) <= 1e-9 * r2).any(), (name, r)
        out = T.cover(v, d2, tabs, r2)[1]
        if out is not None:
            fin = out[np.isfinite(out)]
            assert not (np.abs(fin - r2) <= 1e-9 * r2).any(), (name, r)
    if v.any():
        assert d2[v].max() < R.RADII["sided"][-1] ** 2                               # the last level is never launched


def test_exact_spacings_take_exact_radii():
    for kind in ("unit", "dyadic"):                                                  # everything is a small multiple of 1 / 64: exact
        r2 = np.asarray(R.RADII[kind]) ** 2 * 64.0
        assert np.array_equal(r2, np.rint(r2))
        for v in FIXTURES.values():
            d2 = E.edt_squared(v, *T.tables(v.shape, kind), True) * 64.0
            assert np.array_equal(d2, np.rint(d2))
    g = FIXTURES["grains"]                                                           # ... and the ties are there to be decided
    assert (E.edt_squared(g, *T.tables(g.shape, "unit"), True)[g] == 4.0).any()


def test_the_reference_selects_like_the_keep_rule():
    v = FIXTURES["grains"]
    for conn in C.CONNECTIVITIES:
        labels, n = C.label(v, conn)
        rows = R.per_component(v, conn, "unit")
        assert [r["voxels"] for r in rows] == C.sizes(labels, n).tolist()
        for min_voxels, largest in R.RULES:
            kept = C.keep_from(v, labels, n, min_voxels, largest)
            assert [r["label"] for r in R.select(rows, min_voxels, largest)] == sorted(set(labels[kept].tolist()))
    assert R.select([], 0, True) == []


# ------------------------------------------------------------------ plumbing
def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    syms = test_abi.header_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(L, s), s
    assert L.tomo_abi_version() == 9
    assert {"component_thickness", "components_value", "components_levels"} <= set(pipeline.COUNTERS)


def test_new_exports_answer_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = np.zeros(1024, dtype=np.int64)
    a, b, c, d, e, f = (buf.ctypes.data + 512 * i for i in range(6))                 # distinct host addresses, never read
    head = (a, 4, 4, 4, b, 8, c, d, e)
    assert L.tomo_cc_value_max(None, 4, 4, 4, None, 8, None, None, None, None, None, None, 8, None) == -1
    assert L.tomo_cc_value_max(*head, None, None, f, 8, None) == -1                  # neither dist nor d2
    assert L.tomo_cc_value_max(*head, f, f, f, 8, None) == -1                        # both
    assert L.tomo_cc_value_max(*head, f, None, None, 8, None) == -1
    assert L.tomo_cc_value_max(*head, f, None, f, 0, None) == -1
    assert L.tomo_cc_value_max(a, 4, 0, 4, b, 8, c, d, e, f, None, f, 8, None) == -1
    assert L.tomo_cc_value_max(a, 4, 4, 4, b, 1 << 31, c, d, e, f, None, f, 8, None) == -3
    assert L.tomo_cc_value_first(*head, f, None, a, None, 8, None) == -1
    assert L.tomo_cc_value_first(*head, f, None, a, a, 8, None) == -1                # first is best
    assert L.tomo_cc_value_first(*head, None, None, a, b, 8, None) == -1
    assert L.tomo_cc_value_rows(None, a, b, 8, e, c, d, f, 8, None) == -1
    assert L.tomo_cc_value_rows(a, a, b, 8, e, c, d, f, 0, None) == -1
    assert L.tomo_cc_value_rows(a, a, b, 1 << 31, e, c, d, f, 8, None) == -3
    hist_head = (*head, a, 8, b, c)
    assert L.tomo_cc_level_hist(*hist_head, None, 8, f, 3, None) == -1
    assert L.tomo_cc_level_hist(*hist_head, f, 8, None, 3, None) == -1
    assert L.tomo_cc_level_hist(*hist_head, f, 8, f, 3, None) == -1                  # the histogram is the level map
    assert L.tomo_cc_level_hist(*hist_head, f, 8, a, -1, None) == -1
    assert L.tomo_cc_level_hist(*hist_head, f, 0, a, 3, None) == -1
    assert L.tomo_cc_level_hist(*hist_head, f, 1 << 59, a, 3, None) == -3
    fin = (a, 8, e, b, c, d)
    assert L.tomo_cc_level_sums(*fin, None, 8, f, 4, 3, a, b, c, 8, None) == -1
    assert L.tomo_cc_level_sums(*fin, f, 8, None, 4, 3, a, b, c, 8, None) == -1
    assert L.tomo_cc_level_sums(*fin, f, 8, f, 4, -1, a, b, c, 8, None) == -1
    assert L.tomo_cc_level_sums(*fin, f, 8, f, 4, 3, a, None, c, 8, None) == -1      # levels without their volumes
    assert L.tomo_cc_level_sums(*fin, f, 8, f, 0, 3, a, b, c, 8, None) == -1
    assert L.tomo_cc_level_sums(*fin, f, 8, f, 4, 3, a, b, c, 1 << 31, None) == -3


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(pipeline._lib, "lib", boom)
    monkeypatch.setattr(volume_calculator, "to_device_volume", boom)


def host_volume(shape=(3, 4, 70)):
    return pipeline.BitVolume(torch.zeros((shape[0], shape[1], (shape[2] + 63) // 64), dtype=torch.int64), shape)


BAD_RADII = ([], [0.0, 1.0], [-1.0], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [1.0, np.inf])
BAD_DEPTHS = (np.ones(4), np.ones(2), [], [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0])
BAD_PIXELS = (0.0, -0.5, np.nan, np.inf)


def test_component_thickness_argument_errors(no_device, monkeypatch):
    vol = host_volume()
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radii_mm"):
            pipeline.component_thickness(vol, radii_mm=bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            pipeline.component_thickness(vol, slice_depths=bad)
    for bad in BAD_PIXELS:
        with pytest.raises(ValueError):
            pipeline.component_thickness(vol, mm_per_pixel_y=bad)
        with pytest.raises(ValueError):
            pipeline.component_thickness(vol, mm_per_pixel_x=bad, radii_mm=[1.0])
    for bad in (0, 18, 7, None):
        with pytest.raises(ValueError, match="connectivity"):
            pipeline.component_thickness(vol, connectivity=bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            pipeline.cavity_sizes(vol, slice_depths=bad)
    for bad in (-1, 2.5, np.nan, "3", True):
        with pytest.raises(ValueError, match="min_voxels"):
            pipeline.cavity_sizes(vol, min_voxels=bad)
    monkeypatch.setattr(pipeline, "LOCAL_THICKNESS_VOLUME_BUDGET", 8 * 3 * 4 * 70 - 1)
    with pytest.raises(ValueError, match="LOCAL_THICKNESS_VOLUME_BUDGET"):
        pipeline.component_thickness(vol, radii_mm=[1.0])
    with pytest.raises(AssertionError, match="device"):                              # without radii no d2: the guard does not apply
        pipeline.component_thickness(vol)


def test_drop_in_argument_errors(no_device):
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool), [[[True]]]):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.component_properties(bad, 0.9, 0.7, np.ones(3), thickness=True)
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.closed_porosity(bad, 0.9, 0.7, np.ones(3), pore_size=True)
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radii_mm"):
            volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), thickness=True, thickness_radii_mm=bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            volume_calculator.component_properties(v, 0.9, 0.7, bad, thickness=True)
        with pytest.raises(ValueError):
            volume_calculator.closed_porosity(v, 0.9, 0.7, bad, pore_size=True)
    with pytest.raises(ValueError):
        volume_calculator.component_properties(v, 0.0, 0.7, np.ones(3), thickness=True, thickness_radii_mm=[1.0])


def test_the_flags_are_off_by_default():
    p = inspect.signature(volume_calculator.component_properties).parameters
    assert p["thickness"].default is False and p["thickness_radii_mm"].default is None
    assert inspect.signature(volume_calculator.closed_porosity).parameters["pore_size"].default is False
    q = inspect.signature(pipeline.component_thickness).parameters
    assert list(q) == ["vol", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "min_voxels", "largest", "radii_mm"]
    assert (q["connectivity"].default, q["min_voxels"].default, q["largest"].default, q["radii_mm"].default) == (6, 0, False, None)


def test_zero_rows_have_the_declared_dtypes():
    for radii in (None, np.array([1.0, 2.0])):
        t = pipeline._component_thickness_from((3, 4, 70), None, 1.0, 1.0, np.zeros((0, 4), dtype=np.int64), radii)
        assert len(t) == 0
        kinds = {k: (getattr(t, k).dtype, getattr(t, k).shape) for k in ("labels", "voxels", "radius_mm", "center_index", "center_mm")}
        assert kinds == {"labels": (np.int64, (0,)), "voxels": (np.int64, (0,)), "radius_mm": (np.float64, (0,)),
                         "center_index": (np.int64, (0, 3)), "center_mm": (np.float64, (0, 3))}
        if radii is None:
            assert t.radii_mm is None and t.level_voxels is None and t.mean_mm is None
        else:
            assert t.level_voxels.dtype == np.int64 and t.level_voxels.shape == (0, 2)
            assert t.level_volume_mm3.dtype == np.float64 and t.level_volume_mm3.shape == (0, 2)
            assert t.uncovered_voxels.dtype == np.int64 and t.uncovered_voxels.shape == (0,)
            assert all(getattr(t, k).dtype == np.float64 and getattr(t, k).shape == (0,) for k in ("mean_mm", "std_mm", "max_mm"))
