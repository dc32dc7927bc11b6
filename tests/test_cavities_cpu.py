"""CPU tier of the cavity calls: the host reference (tests/cavities_reference.py) against SciPy's binary_fill_holes, hand
values and tests/golden/topology.npz; the argument checks of the new pipeline / volume_calculator calls, which need no device;
the ABI additions (tomo_cc_select, tomo_cc_cavity_owners, tomo_cc_fill_map) and the VoxelProcessor switches."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavities_reference as R  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator, voxel_processor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "topology.npz"))
FIXTURES = R.fixtures()
NEW_SYMBOLS = ("tomo_cc_select", "tomo_cc_cavity_owners", "tomo_cc_fill_map")
INT64_MAX = 2 ** 63 - 1


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_fill_without_a_window_is_binary_fill_holes(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    v = FIXTURES[name]
    for k in (6, 26):
        structure = ndimage.generate_binary_structure(3, 1 if k == 26 else 3)        # the BACKGROUND's connectivity
        assert np.array_equal(R.fill(v, k), ndimage.binary_fill_holes(v, structure=structure)), (name, k)
        assert np.array_equal(R.fill(v, k) & ~v, R.cavity_mask(v, k))


def test_the_hand_values_of_pores():
    v = R.pores()
    assert v.shape == (9, 12, 140)
    labels, owners, sizes = R.cavities(v, 6)
    assert T.label(v, 6)[1] == 3 and T.label(v, 26)[1] == 3
    assert sizes.tolist() == [12, 840, 2, 1, 2, 1, 4, 6] and owners.tolist() == [1, 2, 1, 1, 1, 2, 3, 1]
    assert labels.tolist() == list(range(2, 10))                     # label 1 is the outside
    labels, owners, sizes = R.cavities(v, 26)
    assert sizes.tolist() == [12, 840, 1, 1, 2, 1, 1, 4, 6] and len(labels) == 9     # the diagonal pair splits into 1 + 1
    assert owners.tolist() == [1, 2, 1, 1, 1, 1, 2, 3, 1]
    assert not R.cavity_mask(v, 6)[1, 5, 50]                         # the pit open to slice 0
    assert R.cavity_mask(v, 6)[3, 5, 63] and R.cavity_mask(v, 6)[3, 5, 64]           # across the word edge
    assert int(R.fill(v, 6, 0, 2).sum() - v.sum()) == 2 + 1 + 2 + 1
    assert int(R.fill(v, 6, 4, 12).sum() - v.sum()) == 12 + 4 + 6
    assert np.array_equal(R.fill(v, 6, 5, 4), v) and np.array_equal(R.fill(v, 6, 0, 0), v)
    t = R.table(v, 6)
    assert t["index_box"][1].tolist() == [2, 6, 3, 8, 100, 131] and t["volume_mm3"].tolist() == [12.0, 840.0, 2.0, 1.0, 2.0, 1.0, 4.0, 6.0]


def test_the_hand_values_of_the_noise_volume():
    v = R.big_noise()
    assert v.shape == (16, 24, 140)
    for k, n_bg, n_cav in ((6, 1290, 779), (26, 3016, 2330)):
        assert R.background(v, k)[1] == n_bg > 1024                  # the selection scan crosses a tile
        assert len(R.cavities(v, k)[0]) == n_cav


def test_nested_and_the_island():
    v = T.nested()
    for k in (6, 26):
        labels, owners, sizes = R.cavities(v, k)
        assert owners.tolist() == [1, 2] and sizes.tolist() == [7 ** 3 - 3 ** 3, 1]       # the island is no part of the shell's void
        assert int(R.fill(v, k, 0, 1).sum() - v.sum()) == 1


@pytest.mark.parametrize("name", list(T.fixtures()))
def test_owners_add_up_to_the_cavities_column_of_the_topology_golden(name):
    v = FIXTURES[name]
    for k in (6, 26):
        tab = GOLDEN["topo%d_%s" % (k, name)]
        labels, owners, _ = R.cavities(v, k)
        assert np.array_equal(np.bincount(owners, minlength=len(tab) + 1)[1:], tab[:, 1]), (name, k)
        assert (owners > 0).all()
        assert np.array_equal(R.all_owners(v, k)[labels - 1], owners)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert _lib.lib().tomo_abi_version() == 9                        # additions only
    for k in ("components_fill", "components_cavity_owners"):
        assert pipeline.COUNTERS[k] >= 0


def test_argument_checks_of_the_entry_points_do_not_need_a_gpu():
    L = _lib.lib()
    one, two, three = ctypes.c_void_p(8), ctypes.c_void_p(16), ctypes.c_void_p(24)   # never dereferenced
    sel = L.tomo_cc_select
    tail = (one, one, one, one, None)
    assert sel(None, 8, one, 0, INT64_MAX, 0, 0, 4, 4, 4, *tail) == -1
    assert sel(one, 8, one, -1, INT64_MAX, 0, 0, 4, 4, 4, *tail) == -1 and sel(one, 8, one, 0, -1, 0, 0, 4, 4, 4, *tail) == -1
    assert sel(one, 0, one, 0, INT64_MAX, 0, 0, 4, 4, 4, *tail) == -1
    assert sel(one, 8, one, 0, INT64_MAX, 1, 1, 4, 4, 4, *tail) == -1                 # largest with enclosed
    assert sel(one, 8, one, 0, 5, 1, 0, 4, 4, 4, *tail) == -1                         # largest with a finite max_voxels
    assert sel(one, 8, one, 0, INT64_MAX, 0, 1, 4, 0, 4, *tail) == -1                 # the face test needs the stack
    assert sel(one, 8, one, 0, INT64_MAX, 0, 0, 4, 4, 4, one, one, one, None, None) == -1
    assert sel(one, 1 << 31, one, 0, INT64_MAX, 0, 0, 4, 4, 4, *tail) == -3
    own = L.tomo_cc_cavity_owners
    fg = (one, 4, 4, 4, one, 8, one, one, one, 4)
    bg = (one, one, 8, one, one, one, one, 4)
    assert own(*fg, *bg, None, None) == -1
    assert own(one, 4, 4, 4, one, 8, one, one, None, 4, *bg, one, None) == -1
    assert own(one, 4, 4, 4, one, 8, one, one, one, 0, *bg, one, None) == -1
    assert own(*fg, one, one, -1, one, one, one, one, 4, one, None) == -1
    assert own(*fg, one, one, 8, one, one, one, None, 4, one, None) == -1             # background runs without their table
    assert own(*fg, one, one, 1 << 31, one, one, one, one, 4, one, None) == -3
    assert own(*fg, None, None, 0, None, None, None, None, 0, None, None) == 0        # a full volume: nothing to do, nothing launched
    fill = L.tomo_cc_fill_map
    assert fill(one, 4, 4, 4, one, 8, one, one, one, one, 3, None, one, None) == -1   # out == bits
    assert fill(one, 4, 4, 4, one, 8, one, one, one, one, 3, two, two, None) == -1    # out == solid
    assert fill(one, 4, 4, 4, one, 8, one, one, one, None, 3, two, three, None) == -1
    assert fill(one, 4, 4, 4, one, 8, one, one, one, one, 9, two, three, None) == -1  # more components than runs
    assert fill(one, 4, 4, 0, one, 8, one, one, one, one, 3, two, three, None) == -1
    assert fill(one, 1 << 15, 1 << 15, 128, one, 8, one, one, one, one, 3, two, three, None) == -3


def test_the_keep_rule_is_normalised_and_checked_before_any_launch():
    assert pipeline._keep_rule() == (0, False, None, False) and pipeline._keep_rule(-5, 1) == (0, True, None, False)
    assert pipeline._keep_rule(27.0, 0, 40, 1) == (27, False, 40, True)
    assert pipeline._keep_rule(7, max_voxels=3) == (7, False, 3, False)              # min > max: no error, nothing selected
    for kw in ({"max_voxels": 5}, {"enclosed": True}, {"max_voxels": 0, "enclosed": True}):
        with pytest.raises(ValueError):
            pipeline._keep_rule(0, True, **kw)
    with pytest.raises(ValueError):
        pipeline._keep_rule(0, False, -1)
    runs = pipeline.ComponentRuns.__new__(pipeline.ComponentRuns)    # no device behind it: the checks come first
    runs._rule = runs._picked = runs._table = runs._topology = None
    tables = np.ones(2)
    for call in (lambda: runs.select(0, True, enclosed=True), lambda: runs.select(0, True, max_voxels=4),
                 lambda: runs.properties(tables, 1.0, 1.0, 0, True, enclosed=True),
                 lambda: runs.moments(tables, 1.0, 1.0, 0, True, max_voxels=4),
                 lambda: runs.surface(tables, 13, 0, True, enclosed=True),
                 lambda: runs.topology_rows(0, True, max_voxels=4), lambda: runs.select(0, max_voxels=-2)):
        with pytest.raises(ValueError):
            call()


def test_pipeline_rejects_bad_arguments_before_it_touches_the_device():
    vol = pipeline.BitVolume(None, (3, 4, 5))
    for fn in (pipeline.cavity_volume, pipeline.fill_cavities):
        with pytest.raises(ValueError):
            fn(vol, connectivity=18)
        for kw in ({"min_voxels": -1}, {"max_voxels": -1}, {"min_voxels": 2.5}, {"max_voxels": 2.5}, {"min_voxels": None},
                   {"max_voxels": "3"}):
            with pytest.raises(ValueError):
                fn(vol, **kw)
    with pytest.raises(ValueError):
        pipeline.cavity_table(vol, connectivity=18)
    for kw in ({"min_voxels": -1}, {"max_voxels": -1}, {"max_voxels": 0.5}, {"slice_depths": np.ones(4)}, {"slice_depths": [1, 0, 1]},
               {"mm_per_pixel_x": 0.0}):
        with pytest.raises(ValueError):
            pipeline.cavity_table(vol, **kw)
    assert pipeline._check_size_window(0, None) == (0, None) and pipeline._check_size_window(4.0, np.int64(7)) == (4, 7)
    assert pipeline._check_size_window(9, 3) == (9, 3)


def test_volume_calculator_rejects_bad_arguments_before_it_touches_the_device():
    ok = np.ones((3, 4, 5), dtype=bool)
    for bad in (np.ones((3, 4, 5), np.uint8), np.ones((4, 5), bool), [[[True]]]):
        with pytest.raises(TypeError):
            volume_calculator.closed_porosity(bad, 1.0, 1.0, np.ones(3))
    with pytest.raises(TypeError):
        volume_calculator.component_properties(np.ones((3, 4, 5), np.uint8), 1.0, 1.0, np.ones(3), porosity=True)
    for kw in ({"connectivity": 18}, {"min_voxels": -1}, {"max_voxels": -3}, {"max_voxels": 1.5}):
        with pytest.raises(ValueError):
            volume_calculator.closed_porosity(ok, 1.0, 1.0, np.ones(3), **kw)
    with pytest.raises(ValueError):
        volume_calculator.closed_porosity(ok, 1.0, 1.0, np.ones(2))
    assert "closed_porosity" not in vars(volume_calculator.VolumeCalculator)


def test_volume_calculator_class_gains_nothing():
    public = sorted(k for k in vars(volume_calculator.VolumeCalculator) if not k.startswith("_"))
    assert public == ["analyze_object_properties", "calculate_bounding_box", "calculate_bounding_box_variable_depth",
                      "calculate_density", "calculate_voxel_volume", "calculate_voxel_volume_variable_depth"]
    assert callable(volume_calculator.closed_porosity)


def test_voxel_processor_switches(monkeypatch):
    for k in ("TOMO_FILL_CAVITIES", "TOMO_MAX_CAVITY_VOXELS", "TOMO_MIN_COMPONENT_VOXELS", "TOMO_KEEP_LARGEST"):
        monkeypatch.delenv(k, raising=False)
    vp = voxel_processor.VoxelProcessor()
    assert vp.fill_cavities is False and vp.max_cavity_voxels == 0 and vp._fill_options() is None and vp._component_options() is None
    marker = object()
    assert vp._keep_components(marker) is marker                     # both off: the volume itself, nothing is launched
    monkeypatch.setenv("TOMO_FILL_CAVITIES", "1")
    monkeypatch.setenv("TOMO_MAX_CAVITY_VOXELS", " 40 ")
    vp2 = voxel_processor.VoxelProcessor()
    assert vp2.fill_cavities is True and vp2.max_cavity_voxels == 40 and vp2._fill_options() == (6, 40)
    vp2.component_connectivity = 26
    vp2.max_cavity_voxels = 0
    assert vp2._fill_options() == (26, None)
    vp2.component_connectivity = 18
    with pytest.raises(ValueError):
        vp2._fill_options()
    vp2.component_connectivity, vp2.max_cavity_voxels = 6, -1
    with pytest.raises(ValueError):
        vp2._fill_options()
    monkeypatch.setenv("TOMO_FILL_CAVITIES", "0")
    assert voxel_processor.VoxelProcessor().fill_cavities is False
    monkeypatch.setenv("TOMO_MAX_CAVITY_VOXELS", "-3")
    with pytest.raises(ValueError):
        voxel_processor.VoxelProcessor()
    monkeypatch.setenv("TOMO_MAX_CAVITY_VOXELS", "many")
    with pytest.raises(ValueError):
        voxel_processor.VoxelProcessor()


def test_empty_rows_have_the_declared_dtypes():
    p = pipeline._component_properties_from(*pipeline._PROPERTIES.empty(), 1.0, 1.0)
    runs = pipeline.ComponentRuns.__new__(pipeline.ComponentRuns)
    c = pipeline._cavities_from(runs, p)
    assert len(c) == 0
    for k, dtype, shape in (("labels", np.int64, (0,)), ("owner", np.int64, (0,)), ("voxels", np.int64, (0,)),
                            ("index_box", np.int64, (0, 6)), ("volume_mm3", np.float64, (0,)), ("centroid_mm", np.float64, (0, 3)),
                            ("centroid_index", np.float64, (0, 3))):
        a = getattr(c, k)
        assert a.dtype == dtype and a.shape == shape, (k, a.dtype, a.shape)
