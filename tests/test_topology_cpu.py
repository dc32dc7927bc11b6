"""CPU tier of the topology measurements: the NumPy / SciPy helper the GPU tests compare with (topology_reference) gives the
hand values of the textbook bodies, its per-component Euler numbers add up to the volume's, the golden file is what the
helper writes, and the new entry points are declared, bound, exported and check their arguments without a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import components_reference as C  # noqa: E402
import make_topology_golden as G  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = np.load(G.PATH)
FIXTURES = T.fixtures()
NEW_SYMBOLS = ("tomo_cc_euler", "tomo_cc_complement", "tomo_cc_cavities", "tomo_cc_topology_rows")


def rows(name, k):
    return T.components(FIXTURES[name], k)[2].tolist()


@pytest.mark.parametrize("k", C.CONNECTIVITIES)
def test_ball_shell_and_torus(k):
    assert rows("ball", k) == [[1, 0, 0]]
    assert rows("shell", k) == [[2, 1, 0]]
    assert rows("torus", k) == [[0, 0, 1]]
    assert T.euler(FIXTURES["ball"], k) == 1 and T.euler(FIXTURES["shell"], k) == 2 and T.euler(FIXTURES["torus"], k) == 0


def test_voxels_that_meet_at_corners():
    assert rows("corner_pair", 6) == [[1, 0, 0]] * 2            # two components
    assert rows("corner_pair", 26) == [[1, 0, 0]]               # one
    assert rows("diamond", 6) == [[1, 0, 0]] * 4                # four components
    assert rows("diamond", 26) == [[0, 0, 1]]                   # one ring
    assert T.cell_counts(FIXTURES["diamond"], 26) == (24, 44, 24, 4)      # four cubes; each of the four inner edges is shared by two
    assert T.cell_counts(FIXTURES["diamond"], 6) == (4, 0, 0, 0)


def test_cube_without_centre_and_corner():
    """Under 6 the centre drains through the missing corner (the background is 26-connected); under 26 it is sealed."""
    assert rows("pierced_cube", 6) == [[1, 0, 0]]
    assert rows("pierced_cube", 26) == [[2, 1, 0]]


@pytest.mark.parametrize("k", C.CONNECTIVITIES)
def test_nesting_borders_and_trivial_volumes(k):
    assert rows("nested", k) == [[2, 1, 0]] * 2                 # the island's void is the island's, the shell's void is one
    assert rows("open_void", k) == [[1, 0, 0]]                  # a void that reaches a face of the stack is no cavity
    assert rows("full", k) == [[1, 0, 0]] and rows("one_voxel", k) == [[1, 0, 0]] and rows("empty", k) == []
    assert rows("cavity_at_64", k) == [[2, 1, 0]]
    assert T.volume(np.zeros((0, 3))) == {"components": 0, "cavities": 0, "handles": 0, "euler": 0}


def test_the_noise_the_issue_counts():
    v = FIXTURES["noise_080"]
    assert v.shape == (6, 9, 70) and np.array_equal(v, np.random.default_rng(7).random((6, 9, 70)) < 0.8)
    assert T.volume(T.components(v, 6)[2])["handles"] == 232
    t26 = T.volume(T.components(v, 26)[2])
    assert (t26["cavities"], t26["handles"]) == (133, 11)


@pytest.mark.parametrize("k", C.CONNECTIVITIES)
def test_component_euler_numbers_add_up_to_the_volumes(k):
    rng = np.random.default_rng(19)
    vols = [FIXTURES[n] for n in ("noise_030", "noise_050", "noise_080", "straddle", "nested")]
    vols += [rng.random(shape) < d for shape, d in [((5, 6, 7), 0.4), ((3, 4, 66), 0.6), ((7, 1, 9), 0.5), ((1, 8, 8), 0.7)]]
    for v in vols:
        labels, n, tab = T.components(v, k)
        assert int(tab[:, 0].sum()) == T.euler(v, k)
        assert n == 0 or int(tab[:, 2].min()) >= 0
        for c in range(min(n, 5)):                              # the cut to the box changes nothing
            mask = labels == c + 1
            assert (T.euler(mask, k), T.cavities(mask, k)) == tuple(tab[c, :2])
    with pytest.raises(ValueError):
        T.euler(vols[0], 18)


def test_labelling_without_scipy_is_the_same(monkeypatch):
    before = T.components(FIXTURES["noise_050"], 6)[2], T.components(FIXTURES["straddle"], 26)[2]
    monkeypatch.setattr(T, "ndimage", None)
    assert np.array_equal(T.components(FIXTURES["noise_050"], 6)[2], before[0])
    assert np.array_equal(T.components(FIXTURES["straddle"], 26)[2], before[1])


def test_golden_file_regenerates_byte_for_byte():
    named = G.arrays()
    assert sorted(named) == sorted(GOLDEN.files)
    for key, value in named.items():
        assert np.array_equal(GOLDEN[key], value) and GOLDEN[key].dtype == np.asarray(value).dtype, key
    assert G.encode(named) == open(G.PATH, "rb").read()
    assert os.path.getsize(G.PATH) < 100000
    for name, vol in FIXTURES.items():
        assert np.array_equal(C.unpack(GOLDEN["bits_" + name], vol.shape), vol)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert _lib.lib().tomo_abi_version() == 9                      # additions only
    for k in ("components_euler", "components_cavities"):
        assert pipeline.COUNTERS[k] >= 0


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    one, two = ctypes.c_void_p(8), ctypes.c_void_p(16)              # never dereferenced: every call below fails its checks first
    eu, cav, rows_ = L.tomo_cc_euler, L.tomo_cc_cavities, L.tomo_cc_topology_rows
    assert eu(None, 4, 4, 4, 6, one, 8, one, one, one, one, 4, None) == -1
    assert eu(one, 4, 4, 4, 18, one, 8, one, one, one, one, 4, None) == -1                # neither 6 nor 26
    assert eu(one, 4, 4, 4, 6, one, 8, one, one, one, None, 4, None) == -1
    assert eu(one, 4, 4, 4, 6, one, 8, one, one, one, one, 0, None) == -1
    assert eu(one, 4, 0, 4, 26, None, 0, None, None, None, one, 1, None) == -1
    assert eu(one, 4, 4, 4, 26, None, 8, one, one, one, one, 4, None) == -1               # tables without their row offsets
    assert eu(one, 4, 4, 4, 26, one, 0, one, one, one, one, 4, None) == -1
    assert eu(one, 4, 4, 4, 6, one, 8, one, one, one, one, 1 << 31, None) == -3
    assert eu(one, 4, 4, 4, 6, one, 1 << 31, one, one, one, one, 4, None) == -3
    assert eu(one, 1 << 15, 1 << 15, 128, 6, None, 0, None, None, None, one, 1, None) == -3   # 2^31 words
    assert L.tomo_cc_complement(None, 4, 4, 4, two, None) == -1 and L.tomo_cc_complement(one, 4, 4, 4, None, None) == -1
    assert L.tomo_cc_complement(one, 4, 4, 4, one, None) == -1                            # out == bits
    assert L.tomo_cc_complement(one, 4, 4, 0, two, None) == -1
    fg = (one, 4, 4, 4, one, 8, one, one, one, 4)
    bg = (one, one, 8, one, one, one, one, 4)
    assert cav(*fg, *bg, None, one, None) == -1 and cav(*fg, *bg, one, None, None) == -1
    assert cav(one, 4, 4, 4, one, 8, one, one, None, 4, *bg, one, one, None) == -1
    assert cav(one, 4, 4, 4, one, 8, one, one, one, 0, *bg, one, one, None) == -1
    assert cav(*fg, one, one, -1, one, one, one, one, 4, one, one, None) == -1
    assert cav(*fg, one, one, 8, one, one, one, None, 4, one, one, None) == -1          # background runs without their table
    assert cav(*fg, one, one, 8, one, one, one, one, 0, one, one, None) == -1
    assert cav(*fg, one, one, 1 << 31, one, one, one, one, 4, one, one, None) == -3
    assert cav(one, 4, 4, 4, one, 8, one, one, one, 1 << 31, *bg, one, one, None) == -3
    assert rows_(None, one, 4, one, one, one, one, 4, None) == -1 and rows_(one, one, 4, one, one, one, None, 4, None) == -1
    assert rows_(one, one, 0, one, one, one, one, 4, None) == -1 and rows_(one, one, 4, one, one, one, one, 0, None) == -1
    assert rows_(one, one, 1 << 31, one, one, one, one, 4, None) == -3 and rows_(one, one, 4, one, one, one, one, 1 << 31, None) == -3


def test_pipeline_rejects_bad_arguments_before_it_touches_the_device():
    vol = pipeline.BitVolume(None, (1, 1, 1))
    for fn in (pipeline.euler_number, pipeline.component_topology, pipeline.volume_topology):
        with pytest.raises(ValueError):
            fn(vol, connectivity=18)
    with pytest.raises(TypeError):
        volume_calculator.component_properties(np.ones((3, 4, 5), np.uint8), 1.0, 1.0, np.ones(3), topology=True)


def test_host_side_of_the_rows():
    """_component_topology_from: the five columns of tomo_cc_topology_rows to the dataclass."""
    t = pipeline._component_topology_from(np.array([[2, 27, 0, 0, 1], [5, 9, 2, 1, 0]]))
    assert len(t) == 2 and t.labels.tolist() == [2, 5] and t.voxels.tolist() == [27, 9]
    assert t.euler.tolist() == [0, 2] and t.cavities.tolist() == [0, 1] and t.handles.tolist() == [1, 0]
    assert all(getattr(t, k).dtype == np.int64 for k in ("labels", "voxels", "euler", "cavities", "handles"))
    e = pipeline._component_topology_from(np.zeros((0, 5), np.int64))
    assert len(e) == 0 and e.euler.shape == (0,) and e.handles.dtype == np.int64
