"""CPU tier of the local thickness: the NumPy helper held against itself two ways (all pairs of set voxels / one outside
transform per level), the max rule, and the argument checks of the new functions and exports -- none of which needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as E  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

FIXTURES = T.fixtures()
NAMES = list(FIXTURES)


def test_fixtures():
    assert NAMES == ["one", "empty", "full", "plate", "dumbbell", "speckle", "shell", "edge"]
    shapes = {"one": (1, 1, 1), "empty": (3, 5, 70), "full": (5, 7, 66), "plate": (12, 20, 70), "dumbbell": (16, 24, 80),
              "speckle": (10, 18, 67), "shell": (15, 15, 67), "edge": (9, 14, 131)}
    for name, v in FIXTURES.items():
        assert v.shape == shapes[name] and v.dtype == bool and v.sum() <= 6500
    assert FIXTURES["full"].all() and not FIXTURES["empty"].any()
    assert FIXTURES["edge"][:, :, 0].any() and FIXTURES["edge"][:, :, 130].any()
    hollow = FIXTURES["shell"]
    assert not hollow[7, 7, 33] and hollow[7, 7, 28]
    again = T.fixtures()
    assert all(np.array_equal(again[k], FIXTURES[k]) for k in NAMES)             # seeded


def test_dyadic_spacing_is_exact():
    for nz in (1, 5, 16):
        depths, mm_y, mm_x = T.spacing("dyadic", nz)
        assert len(depths) == nz and set(depths) <= {0.75, 0.25, 1.25} and (mm_y, mm_x) == (0.5, 0.75)
        zt, yt, xt = E.positions((nz, 24, 131), depths, mm_y, mm_x)
        for t in (zt, yt, xt):
            assert np.array_equal(t * 8, np.rint(t * 8))                         # multiples of 1 / 8: squares and sums are exact
    assert T.spacing("unit", 4) == E.spacing("unit", 4)
    assert np.array_equal(T.spacing("sided", 7)[0], E.sided_depths(7))
    with pytest.raises(ValueError):
        T.spacing("uniform", 3)


@pytest.mark.parametrize("kind", ["unit", "dyadic"])
@pytest.mark.parametrize("name", NAMES)
def test_levels_equal_all_pairs(name, kind):
    """by_levels with every distinct D2 as a level == the brute force over all pairs, bit for bit."""
    v = FIXTURES[name]
    tabs = T.tables(v.shape, kind)
    d2 = E.edt_squared(v, *tabs, True)
    r2s = T.distinct_levels(v, d2)
    level = T.by_levels(v, d2, tabs, r2s)
    assert level.dtype == np.int32 and np.array_equal(level > 0, v)              # every set voxel lies in its own ball
    got = np.concatenate([[0.0], r2s])[level]
    assert np.array_equal(got, T.direct(v, d2, *tabs))
    assert (got >= d2).all()                                                     # at least its own ball
    if v.any():
        top = np.float32(2.0 * np.sqrt(got.max()))
        assert top == 2 * np.float32(E.sphere(v, *tabs)[0])
        exp = T.expected(v, level, np.sqrt(r2s), T.slice_weights(v.shape, kind))
        assert exp["uncovered_voxels"] == 0 and exp["level_voxels"].sum() == v.sum()
        assert exp["thickness"].max() == top and np.float32(exp["max_mm"]) == top
        assert exp["thickness"][v].min() <= exp["mean_mm"] <= exp["max_mm"] and exp["std_mm"] >= 0


def coverage(name, kind, r2s):
    v = FIXTURES[name]
    tabs = T.tables(v.shape, kind)
    d2 = E.edt_squared(v, *tabs, True)
    return [int(T.cover(v, d2, tabs, r2)[0].sum()) for r2 in (T.distinct_levels(v, d2) if r2s is None else r2s)]


def test_openings_are_not_monotone():
    """A larger ball can cover MORE voxels than a smaller one: `level` is a maximum, not a first failure."""
    cov = coverage("dumbbell", "unit", None)
    assert any(a < b for a, b in zip(cov, cov[1:]))
    cov = coverage("full", "unit", [1.0, 2.25, 4.0, 9.0])                        # the radii of the GPU tier under unit spacing
    assert cov[1] < cov[2] == FIXTURES["full"].sum()
    v = FIXTURES["full"]
    tabs = T.tables(v.shape, "unit")
    d2 = E.edt_squared(v, *tabs, True)
    level = T.by_levels(v, d2, tabs, [1.0, 2.25, 4.0, 9.0])
    first_failure = np.zeros(v.shape, dtype=np.int32)
    alive = v.copy()
    for k, r2 in enumerate([1.0, 2.25, 4.0, 9.0]):
        alive &= T.cover(v, d2, tabs, r2)[0]
        first_failure[alive] = k + 1
    assert (level >= first_failure).all() and (level > first_failure).any()


def test_strict_and_closed_comparisons():
    """D2 >= r^2 admits a centre at exactly r; |pq|^2 < r^2 leaves out a voxel at exactly r."""
    v = np.zeros((5, 5, 5), dtype=bool)
    v[1:4, 1:4, 1:4] = True
    v[2, 2, 0] = True
    tabs = E.positions(v.shape)
    d2 = E.edt_squared(v, *tabs, True)
    assert d2[2, 2, 2] == 4.0 and (d2[v] >= 4.0).sum() == 1
    opened, _ = T.cover(v, d2, tabs, 4.0)                        # the one centre (2, 2, 2) fits a ball of exactly 2
    assert opened[2, 2, 1] and not opened[2, 2, 0]               # (2, 2, 0) sits at exactly 2: outside the open ball
    assert not T.cover(v, d2, tabs, np.nextafter(4.0, 5.0))[0].any()


# ------------------------------------------------------------------ argument errors, before any device use
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


def test_local_thickness_argument_errors(no_device):
    vol = host_volume()
    assert pipeline.LOCAL_THICKNESS_MAX_LEVELS == 512 and pipeline.LOCAL_THICKNESS_VOLUME_BUDGET >= 8 * 512 ** 3
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radii_mm"):
            pipeline.local_thickness(vol, radii_mm=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_levels"):
            pipeline.local_thickness(vol, max_levels=bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            pipeline.local_thickness(vol, slice_depths=bad)
    for bad in BAD_PIXELS:
        with pytest.raises(ValueError):
            pipeline.local_thickness(vol, mm_per_pixel_y=bad)
        with pytest.raises(ValueError):
            pipeline.local_thickness(vol, mm_per_pixel_x=bad, radii_mm=[1.0])
    assert {"local_thickness", "opening_volume"} <= set(pipeline.COUNTERS)


def test_local_thickness_volume_budget(no_device, monkeypatch):
    monkeypatch.setattr(pipeline, "LOCAL_THICKNESS_VOLUME_BUDGET", 8 * 3 * 4 * 70 - 1)
    with pytest.raises(ValueError, match="LOCAL_THICKNESS_VOLUME_BUDGET"):
        pipeline.local_thickness(host_volume())


def test_opening_volume_argument_errors(no_device):
    vol = host_volume()
    for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius_mm"):
            pipeline.opening_volume(vol, bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            pipeline.opening_volume(vol, 1.0, slice_depths=bad)
    for bad in BAD_PIXELS:
        with pytest.raises(ValueError):
            pipeline.opening_volume(vol, 1.0, mm_per_pixel_y=bad)
        with pytest.raises(ValueError):
            pipeline.opening_volume(vol, 1.0, mm_per_pixel_x=bad)


def test_thickness_statistics_argument_errors(no_device):
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((3, 4, 5), dtype=np.float32), np.ones((4, 5), dtype=bool), [[[True]]]):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.thickness_statistics(bad, 0.9, 0.7, np.ones(3))
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radii_mm"):
            volume_calculator.thickness_statistics(v, 0.9, 0.7, np.ones(3), radii_mm=bad)
    for bad in BAD_DEPTHS:
        with pytest.raises(ValueError):
            volume_calculator.thickness_statistics(v, 0.9, 0.7, bad)
    with pytest.raises(ValueError):
        volume_calculator.thickness_statistics(v, 0.0, 0.7, np.ones(3))
    assert "thickness_statistics" not in vars(volume_calculator.VolumeCalculator)


def test_statistics_from_the_level_table():
    assert pipeline._thickness_statistics([], []) == (0.0, 0.0, 0.0)
    assert pipeline._thickness_statistics([1.0, 2.0], [0.0, 0.0]) == (0.0, 0.0, 0.0)
    assert pipeline._thickness_statistics([1.5], [3.0]) == (3.0, 0.0, 3.0)
    mean, std, top = pipeline._thickness_statistics([0.5, 1.5, 4.0], [1.0, 3.0, 0.0])       # diameters 1 and 3, weights 1 and 3
    assert (mean, top) == (2.5, 3.0) and std == np.sqrt((1 * 1.5 ** 2 + 3 * 0.5 ** 2) / 4)


# ------------------------------------------------------------------ the C exports answer bad arguments without a GPU
def test_new_exports_answer_bad_arguments_without_a_gpu():
    L = _lib.lib()
    big = 1 << 20
    assert L.tomo_edt_squared(None, 4, 4, 4, None, None, None, 1, None, None, big, None) == -1
    assert L.tomo_edt_at_least(None, None, 4, 4, 4, 1.0, None, None) == -1
    assert L.tomo_edt_cover(None, None, 4, 4, 4, None, None, None, 1.0, 1, None, None, big, None) == -1
    assert L.tomo_edt_threshold_masked(None, 4, 4, 4, None, None, None, 1, 1.0, 0, None, None, None, big, None) == -1
    assert L.tomo_edt_thickness_finish(None, None, 4, 4, 4, None, 1, None, None) == -1
    buf = np.zeros(256, dtype=np.int64)
    p, q, r, s = (buf.ctypes.data + 512 * i for i in range(4))                   # four distinct host addresses, never read
    assert L.tomo_edt_squared(p, 0, 4, 4, p, p, p, 1, q, r, big, None) == -1
    assert L.tomo_edt_squared(p, 4, 4, 4, p, p, p, 1, p, r, big, None) == -1     # the result is the input
    assert L.tomo_edt_squared(p, 4, 4, 4, p, p, p, 1, q, r, 0, None) == -1
    assert L.tomo_edt_squared(p, 100, 200, 64, p, p, p, 1, q, r, 1000, None) == -4           # less than one word of columns
    assert L.tomo_edt_at_least(p, q, 4, 4, 0, 1.0, r, None) == -1
    assert L.tomo_edt_at_least(p, q, 4, 4, 4, -1.0, r, None) == -1
    assert L.tomo_edt_at_least(p, q, 4, 4, 4, float("nan"), r, None) == -1
    assert L.tomo_edt_at_least(p, q, 4, 4, 4, 1.0, q, None) == -1 and L.tomo_edt_at_least(p, q, 4, 4, 4, 1.0, p, None) == -1
    assert L.tomo_edt_cover(p, q, 4, 4, 4, p, p, p, 1.0, 0, r, s, big, None) == -1           # levels are 1-based
    assert L.tomo_edt_cover(p, q, 4, 4, 4, p, p, p, -1.0, 1, r, s, big, None) == -1
    assert L.tomo_edt_cover(p, None, 4, 4, 4, p, p, p, 1.0, 1, r, s, big, None) == -1
    assert L.tomo_edt_cover(p, q, 4, 4, 4, p, p, p, 1.0, 1, q, s, big, None) == -1           # the map is the volume
    assert L.tomo_edt_cover(p, q, 100, 200, 64, p, p, p, 1.0, 1, r, s, 1000, None) == -4
    assert L.tomo_edt_threshold_masked(p, 4, 4, 4, p, p, p, 1, 1.0, 0, None, r, s, big, None) == -1
    assert L.tomo_edt_threshold_masked(p, 4, 4, 4, p, p, p, 1, 1.0, 0, q, q, s, big, None) == -1
    assert L.tomo_edt_threshold_masked(p, 4, 4, 4, p, p, p, 1, 1.0, 0, p, p, s, big, None) == -1
    assert L.tomo_edt_threshold_masked(p, 4, 4, 4, p, p, p, 0, float("nan"), 1, q, r, s, big, None) == -1
    assert L.tomo_edt_thickness_finish(p, q, 4, 4, 4, None, 1, r, None) == -1    # levels without their values
    assert L.tomo_edt_thickness_finish(p, q, 4, 4, 4, r, -1, s, None) == -1
    assert L.tomo_edt_thickness_finish(p, p, 4, 4, 4, r, 1, s, None) == -1
    assert L.tomo_edt_thickness_finish(p, q, 4, -4, 4, r, 1, s, None) == -1
    assert L.tomo_abi_version() == 9
