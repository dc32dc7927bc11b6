"""CPU tier of the connected-component work: the NumPy helper the GPU tests compare with reproduces SciPy's answers (the
golden file everywhere, SciPy itself where it imports), the golden file says what the issue lists, the VoxelProcessor options
parse, and the new entry points are declared, bound, exported and check their arguments without a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.voxel_processor import VoxelProcessor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "components.npz"))
FIXTURES = C.fixtures()
NEW_SYMBOLS = ("tomo_cc_scan_blocks", "tomo_cc_count_runs", "tomo_cc_label_runs", "tomo_cc_expand", "tomo_cc_filter")


@pytest.mark.parametrize("name", list(FIXTURES))
def test_golden_file_holds_the_fixture_volumes(name):
    vol = FIXTURES[name]
    assert tuple(GOLDEN["shape_" + name]) == vol.shape
    assert np.array_equal(GOLDEN["bits_" + name], C.pack(vol))
    assert np.array_equal(C.unpack(GOLDEN["bits_" + name], vol.shape), vol)


def test_golden_counts_are_the_listed_ones():
    for (name, conn), n in C.KNOWN_COUNTS.items():
        assert int(GOLDEN["n%d_%s" % (conn, name)]) == n, (name, conn)
    assert int(FIXTURES["serpentine"].sum()) == 2124 and GOLDEN["sizes6_serpentine"].tolist() == [2124]
    assert GOLDEN["sizes6_comb"].tolist() == [int(FIXTURES["comb"].sum())]


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_helper_reproduces_the_golden_file(name, conn):
    vol = FIXTURES[name]
    labels, n = C.label(vol, conn)
    assert labels.dtype == np.int32 and n == int(GOLDEN["n%d_%s" % (conn, name)])
    assert np.array_equal(C.sizes(labels, n), GOLDEN["sizes%d_%s" % (conn, name)])
    key = "labels%d_%s" % (conn, name)
    assert (key in GOLDEN.files) == (vol.size <= C.LABELLED)
    if key in GOLDEN.files:
        assert np.array_equal(labels, GOLDEN[key])
    # numbered in raster order of the first voxel, which makes the labelling unique
    flat = labels.reshape(-1)
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    assert np.all(np.diff(first[1:]) > 0)


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_helper_reproduces_scipy(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)
    rng = np.random.default_rng(conn)
    vols = [FIXTURES[k] for k in ("checkerboard", "noise_big", "snake3d", "words_130")]
    vols += [rng.random(shape) < d for shape, d in [((7, 8, 9), 0.3), ((2, 3, 200), 0.6), ((9, 1, 5), 0.5), ((4, 33, 65), 0.2)]]
    for vol in vols:
        exp, n = ndimage.label(vol, structure)
        got, m = C.label(vol, conn)
        assert m == n and np.array_equal(got, exp)


def test_helper_keep_rule():
    vol = FIXTURES["tie"]
    labels, n = C.label(vol, 6)
    assert n == 3 and C.sizes(labels, n).tolist() == [1, 27, 27]      # the speck comes first in raster order
    sz = C.sizes(labels, n)
    first_cube = int(np.flatnonzero(sz == 27)[0]) + 1
    assert np.array_equal(C.keep(vol, largest=True), labels == first_cube)
    assert np.array_equal(C.keep(vol, 2), (labels > 0) & (sz[np.maximum(labels, 1) - 1] >= 2))
    assert np.array_equal(C.keep(vol, 0), vol) and np.array_equal(C.keep(vol, 1), vol)
    assert not C.keep(vol, 28).any() and not C.keep(vol, 28, largest=True).any()
    assert not C.keep(np.zeros((2, 2, 2), bool), largest=True).any()
    with pytest.raises(ValueError):
        C.label(vol, 18)


def test_option_defaults_and_environment(monkeypatch):
    for k in ("TOMO_MIN_COMPONENT_VOXELS", "TOMO_KEEP_LARGEST"):
        monkeypatch.delenv(k, raising=False)
    vp = VoxelProcessor()
    assert (vp.min_component_voxels, vp.keep_largest_component, vp.component_connectivity) == (0, False, 6)
    assert vp._component_options() is None
    monkeypatch.setenv("TOMO_MIN_COMPONENT_VOXELS", "28")
    monkeypatch.setenv("TOMO_KEEP_LARGEST", "0")
    vp2 = VoxelProcessor()
    assert (vp2.min_component_voxels, vp2.keep_largest_component) == (28, False) and vp2._component_options() == (28, False, 6)
    assert vp.min_component_voxels == 0                           # read when the object is made, not later
    monkeypatch.setenv("TOMO_MIN_COMPONENT_VOXELS", "")
    monkeypatch.setenv("TOMO_KEEP_LARGEST", "1")
    vp3 = VoxelProcessor()
    assert (vp3.min_component_voxels, vp3.keep_largest_component) == (0, True) and vp3._component_options() == (0, True, 6)
    vp3.component_connectivity = 26
    assert vp3._component_options() == (0, True, 26)
    vp3.component_connectivity = 18
    with pytest.raises(ValueError):
        vp3._component_options()
    for bad in ("-1", "many"):
        monkeypatch.setenv("TOMO_MIN_COMPONENT_VOXELS", bad)
        with pytest.raises(ValueError):
            VoxelProcessor()


def test_zero_size_masks_pass_through_with_an_option_set(capsys):
    vp = VoxelProcessor()
    vp.min_component_voxels = 5
    out = vp.create_voxel_data([np.zeros((0, 4), bool)] * 3)
    assert out.shape == (3, 0, 4) and "active: 0" in capsys.readouterr().out


def test_an_option_without_a_gpu_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vp = VoxelProcessor()
    vp.keep_largest_component = True
    masks = [np.ones((4, 16), bool)] * 3
    for close_ends in (True, False):
        with pytest.raises(_lib.TomoUnavailable):
            vp.create_voxel_data(masks, close_ends)
    with pytest.raises(_lib.TomoUnavailable):
        vp.smooth_voxel_data(np.ones((3, 4, 16), bool))


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert _lib.lib().tomo_abi_version() == 9                      # these were additive (7); 8 and 9 since exports without a caller left
    for k in ("components_label", "components_expand", "components_filter"):
        assert pipeline.COUNTERS[k] >= 0


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    one = ctypes.c_void_p(8)                                      # never dereferenced: every call below fails its checks first
    assert L.tomo_cc_scan_blocks(0) == -1 and L.tomo_cc_scan_blocks(1) == 2 and L.tomo_cc_scan_blocks(1025) == 3
    assert L.tomo_cc_count_runs(None, 4, 4, 4, one, one, one, None) == -1
    assert L.tomo_cc_count_runs(one, 4, 0, 4, one, one, one, None) == -1
    assert L.tomo_cc_count_runs(one, 4, 4, 4, None, one, one, None) == -1
    assert L.tomo_cc_count_runs(one, 1 << 15, 1 << 15, 128, one, one, one, None) == -3       # 2^31 words
    assert L.tomo_cc_label_runs(one, 4, 4, 4, 18, one, 8, one, one, one, one, one, None) == -1   # neither 6 nor 26
    assert L.tomo_cc_label_runs(one, 4, 4, 4, 6, one, 0, one, one, one, one, one, None) == -1
    assert L.tomo_cc_label_runs(one, 4, 4, 4, 26, one, 8, one, None, one, one, one, None) == -1
    assert L.tomo_cc_label_runs(one, 4, 4, 4, 6, one, 1 << 31, one, one, one, one, one, None) == -3
    assert L.tomo_cc_expand(one, 4, 4, 4, one, 8, one, one, one, None, None) == -1
    assert L.tomo_cc_expand(one, 4, 4, -1, one, 8, one, one, one, one, None) == -1
    assert L.tomo_cc_filter(one, 4, 4, 4, one, 8, one, one, one, one, 0, 0, one, None) == -1     # out == bits
    assert L.tomo_cc_filter(one, 4, 4, 4, one, 8, one, one, one, one, -1, 0, ctypes.c_void_p(16), None) == -1
    assert L.tomo_cc_filter(one, 4, 4, 4, one, 8, one, one, None, one, 0, 1, ctypes.c_void_p(16), None) == -1


def test_pipeline_rejects_other_connectivities():
    vol = pipeline.BitVolume(None, (1, 1, 1))
    for fn in (pipeline.label_components, pipeline.component_sizes, pipeline.keep_components):
        with pytest.raises(ValueError):
            fn(vol, connectivity=18)
