"""CPU tier of the components-across-slabs work: the numbering rule (label every slab, ids base_r + c, unite across the cuts,
number the roots) reproduces the labelling of the whole volume in a NumPy model, and the new entry points are declared,
bound, exported and check their arguments without a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import slab_components_reference as S  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "components.npz"))
FIXTURES = {k: v for k, v in C.fixtures().items() if v.shape[0] >= 2}
SHAPES = S.shapes()
NEW_SYMBOLS = ("tomo_cc_slice_components", "tomo_cc_seam_union", "tomo_cc_merge_tables", "tomo_cc_local_maps", "tomo_cc_filter_map",
               "tomo_cc_expand_map")


def check_model(vol, cuts, conn, whole):
    labels, n = whole
    m = S.model(vol, cuts, conn)
    assert m["n"] == n and np.array_equal(m["sizes"], C.sizes(labels, n)), cuts
    assert np.array_equal(m["labels"], labels), cuts
    assert int(m["bases"][-1]) == sum(m["ns"]) >= n and m["sizes"].sum() == int(np.asarray(vol).sum())
    assert np.all(m["parent"] <= np.arange(len(m["parent"])))     # a root is the smallest id of its component


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_model_reproduces_the_whole_volume_on_the_fixtures(name, conn):
    vol = FIXTURES[name]
    whole = C.label(vol, conn)
    assert whole[1] == int(GOLDEN["n%d_%s" % (conn, name)])
    assert np.array_equal(C.sizes(*whole), GOLDEN["sizes%d_%s" % (conn, name)])
    for cuts in S.cut_sets(vol.shape[0]):
        check_model(vol, cuts, conn, whole)


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_model_reproduces_the_whole_volume_on_the_built_shapes(name, conn):
    vol, cuts = SHAPES[name]
    whole = C.label(vol, conn)
    for c in [cuts] + S.cut_sets(vol.shape[0]):
        check_model(vol, c, conn, whole)


def test_the_built_shapes_are_what_they_are_meant_to_be():
    n = {(k, conn): C.label(SHAPES[k][0], conn)[1] for k in SHAPES for conn in C.CONNECTIVITIES}
    assert n[("pillars", 6)] == 2 and n[("w", 6)] == 2
    v, cuts = SHAPES["pillars"]
    assert S.model(v, cuts, 6)["ns"] == [3, 2, 1]                 # two pieces of one component in the middle slab
    v, cuts = SHAPES["w"]
    m = S.model(v, cuts, 6)
    assert m["ns"] == [2, 3] and len(m["pairs"]) == 3             # the same seam crossed three times
    assert (n[("corner_cut", 6)], n[("corner_cut", 26)]) == (2, 1)
    assert (n[("diagonal_rows", 6)], n[("diagonal_rows", 26)]) == (6, 3)
    v, cuts = SHAPES["empty_middle"]
    assert not v[cuts[1]:cuts[2]].any() and v[:cuts[1]].any() and v[cuts[2]:].any()
    v, cuts = SHAPES["empty_seam_slice"]
    assert not v[cuts[1] - 1].any() and v[cuts[1]].any()
    v, cuts = SHAPES["summed_tie"]
    labels, k = C.label(v, 6)
    assert C.sizes(labels, k).tolist() == [15, 20] and S.model(v, cuts, 6)["local_sizes"][0].tolist() == [15, 10]
    assert np.array_equal(C.keep(v, largest=True), labels == 2)
    v, cuts = SHAPES["tie_cut"]
    m = S.model(v, cuts, 6)
    assert m["sizes"].tolist() == [1, 27, 27] and m["ns"] == [2, 1]


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert _lib.lib().tomo_abi_version() == 9                      # these were additive (7); 8 and 9 since exports without a caller left
    for k in ("slab_components_label", "slab_components_seam", "slab_components_merge", "slab_components_expand",
              "slab_components_filter"):
        assert pipeline.COUNTERS[k] >= 0


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    one, two = ctypes.c_void_p(8), ctypes.c_void_p(16)            # never dereferenced: every call below fails its checks first
    assert L.tomo_cc_slice_components(4, 4, 4, one, 8, one, one, one, one, 8, None) == -1        # z == nz
    assert L.tomo_cc_slice_components(4, 4, -1, one, 8, one, one, one, one, 8, None) == -1
    assert L.tomo_cc_slice_components(4, 4, 3, one, 8, one, one, one, None, 8, None) == -1
    assert L.tomo_cc_slice_components(4, 4, 3, one, 8, one, one, one, one, 0, None) == -1
    assert L.tomo_cc_slice_components(4, 4, 3, one, 1 << 31, one, one, one, one, 8, None) == -3
    seam = [one, 4, 4, 6, one, 8, one, one, one, one, one, one, 3, 2, 2, one, one, None]
    for at, bad in ((0, None), (1, 0), (3, 18), (5, 0), (9, None), (11, None), (12, 0), (13, 0), (14, 0), (15, None), (16, None)):
        args = list(seam)
        args[at] = bad
        assert L.tomo_cc_seam_union(*args) == -1, at
    args = list(seam)
    args[13] = args[14] = 1 << 30
    assert L.tomo_cc_seam_union(*args) == -3
    merge = [one, 2, 5, 3, one, 4, 2, 4, one, one, one, one, one, None]
    for at, bad in ((0, None), (1, 0), (2, 4), (3, 2), (4, None), (5, 0), (6, 0), (6, 5), (7, -1), (7, 5), (8, None), (12, None)):
        args = list(merge)
        args[at] = bad
        assert L.tomo_cc_merge_tables(*args) == -1, at
    assert L.tomo_cc_merge_tables(one, 2, (1 << 31) + 5, (1 << 31) + 1, one, 1 << 31, 1 << 31, 0, one, one, one, one, one, None) == -3
    maps = [one, one, one, one, 4, 1, 3, 0, 0, one, one, None]
    for at, bad in ((0, None), (3, None), (4, 0), (5, -1), (5, 2), (6, 0), (7, -1)):
        args = list(maps)
        args[at] = bad
        assert L.tomo_cc_local_maps(*args) == -1, at
    assert L.tomo_cc_local_maps(one, one, one, one, 4, 1, 3, 0, 0, None, None, None) == -1       # neither map
    assert L.tomo_cc_filter_map(one, 4, 4, 4, one, 8, one, one, one, one, 3, one, None) == -1    # out == bits
    assert L.tomo_cc_filter_map(one, 4, 4, 4, one, 8, one, one, one, None, 3, two, None) == -1
    assert L.tomo_cc_filter_map(one, 4, 4, 4, one, 8, one, one, one, one, 9, two, None) == -1    # more components than runs
    assert L.tomo_cc_filter_map(one, 1 << 15, 1 << 15, 128, one, 8, one, one, one, one, 3, two, None) == -3
    assert L.tomo_cc_expand_map(one, 4, 4, 4, one, 8, one, one, one, None, 3, one, None) == -1
    assert L.tomo_cc_expand_map(one, 4, 4, 4, one, 8, one, one, one, one, 0, one, None) == -1
    assert L.tomo_cc_expand_map(one, 4, 0, 4, one, 8, one, one, one, one, 3, one, None) == -1


class _NoComm:
    rank, world = 0, 1


def test_bad_inputs_raise_without_a_gpu(monkeypatch):
    import torch
    from tomography_3d_reconstructor_amd.slab_components import SlabComponents
    vol = pipeline.BitVolume(torch.zeros((2, 3, 1), dtype=torch.int64), (2, 3, 40))
    with pytest.raises(ValueError):
        SlabComponents(vol, _NoComm(), connectivity=18)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.TomoUnavailable):
        SlabComponents(vol, _NoComm())
    with pytest.raises(ValueError):
        SlabComponents(vol, _NoComm(), connectivity=18)
