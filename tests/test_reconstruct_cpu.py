"""CPU tier of the grey reconstruction, the h-maxima and the separation by height: the reference
(tests/reconstruct_reference.py) against itself computed another way -- the claim the tiled sweep rests on: the operator is
monotone, so every order ends at the same bytes --, the "float just below" rule against the plateau definition, the scene no
fixed erosion radius splits, and the plumbing (exports, argument checks before any device use, signatures).  None of it needs
a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import reconstruct_reference as R  # noqa: E402
import test_abi  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

NEW_SYMBOLS = ("tomo_recon_seed", "tomo_recon_sweep", "tomo_recon_below")
SHAPE = (9, 17, 70)
MAPS = ("five", "levels256", "float", "zeros", "negative")
_cache = {}


def make_map(kind, seed):
    if kind == "five":
        return R.level_map(SHAPE, 5, seed)
    if kind == "levels256":
        return R.level_map(SHAPE, 256, seed, lo=-3.0, step=0.125)
    if kind == "float":
        return R.float_map(SHAPE, seed)
    if kind == "zeros":
        return R.zero_map(SHAPE, seed)
    return R.level_map(SHAPE, 7, seed, lo=-9.5, step=1.5)                             # all but one level negative


def scene_maxima(h):
    """The extended maxima of the scene's distance map under connectivity 6, computed once and shared, read-only."""
    if h not in _cache:
        v = R.scene()
        _cache[h] = R.extended_maxima(v, R.unit_distance(v), h, 6)
    return _cache[h]


# ------------------------------------------------------------------ the fixed point
@pytest.mark.parametrize("density", (0.3, 0.7))
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("kind", MAPS)
def test_two_reconstructions_agree_byte_for_byte(kind, conn, density):
    v = R.noise(SHAPE, density, 11)
    f = make_map(kind, 1)
    for marker in (make_map(kind, 2), R.h_marker(f, 1.0), R.below(f)):
        a, n = R.sweeps(v, f, marker, conn)
        b = R.flood(v, f, marker, conn)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), (kind, conn, density)
        assert (a[~v] == 0).all()
        assert not (np.signbit(a) & (a == 0)).any()                                  # -0.0 never comes back
        lo = np.minimum(R.canon(marker), R.canon(f))
        assert (a[v] >= lo[v]).all() and (a[v] <= R.canon(f)[v]).all()
        # a fixed point: one more application of the operator changes nothing
        assert R.sweeps(v, f, a, conn)[0].tobytes() == a.tobytes() and n >= 1


@pytest.mark.parametrize("density", (0.3, 0.7))
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("kind", MAPS)
def test_the_float_just_below_gives_the_plateau_maxima(kind, conn, density):
    v = R.noise(SHAPE, density, 12)
    f = make_map(kind, 3)
    want = R.plateau_maxima(v, f, conn)
    assert np.array_equal(R.regional_maxima(v, f, conn), want), (kind, conn, density)
    assert np.array_equal(R.regional_maxima(v, f, conn, how=R.flood), want)
    assert want.any() and (want <= v).all()
    if kind == "five":                                                               # plateaus, not single voxels
        labels = R.plateaus(v, f, conn)
        assert np.bincount(labels[v]).max() >= 4


def test_the_keys_order_the_floats_and_step_by_one():
    a = np.array([-np.inf, -3.4e38, -1.0, -1.2e-38, -1e-45, -0.0, 0.0, 1e-45, 1.2e-38, 1.0, 3.4e38, np.inf], dtype=np.float32)
    k = R.keys(a)
    assert k[5] == k[6] == 1 << 31 and (np.diff(k[[0, 1, 2, 3, 4, 5]]) > 0).all() and (np.diff(k[6:]) > 0).all()
    assert k[0] == 0x00800000 and k[-1] == 0xff800000                                # key 0 lies below every value
    assert R.values(k).tobytes() == R.canon(a).tobytes()
    rng = np.random.default_rng(4)
    b = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    b = b[np.isfinite(b)]
    assert R.values(R.keys(b) - 1).tobytes() == R.below(b).tobytes()                 # "the float just below" is the key minus one
    assert R.values(R.keys(np.float32([0.0])) - 1)[0] == np.float32(-1e-45)
    order = np.argsort(b, kind="stable")
    assert (np.diff(R.keys(b)[order]) >= 0).all()


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_idempotent_and_monotone_in_the_marker(conn):
    v = R.noise(SHAPE, 0.7, 13)
    f = make_map("levels256", 5)
    m = make_map("levels256", 6)
    g = R.reconstruct(v, f, m, conn)
    assert R.reconstruct(v, f, g, conn).tobytes() == g.tobytes()
    raised = (m + np.float32(0.5) * (np.random.default_rng(7).random(SHAPE) < 0.1)).astype(np.float32)
    assert (R.reconstruct(v, f, raised, conn)[v] >= g[v]).all()
    assert (R.reconstruct(v, f, raised, conn) != g).any()


# ------------------------------------------------------------------ the scene
def test_no_erosion_radius_leaves_six_cores():
    v = R.scene()
    assert v.shape == (20, 40, 70) and C.label(v, 6)[1] == 4
    d = R.unit_distance(v)
    cores = {r: C.label(v & (d > r), 6)[1] for r in np.arange(0.5, 8.01, 0.5)}
    assert len(cores) == 16 and 6 not in cores.values(), cores
    assert max(cores.values()) == 5 and cores[0.5] == 4 and cores[3.0] == 5 and cores[4.5] < 4 and cores[5.5] < 4
    print("cores per radius:", cores)


def test_the_extended_maxima_mark_the_six_grains():
    v = R.scene()
    labels, n = C.label(v, 6)
    m = scene_maxima(1.0)
    ml, count = C.label(m, 6)
    assert n == 4 and count == 6 and (m <= v).all()
    per = [len(np.unique(ml[(labels == c) & m])) for c in range(1, n + 1)]
    assert tuple(per) == R.SCENE_MARKERS, per
    for (cz, cy, cx), _ in R.SCENE_BALLS:                                             # every ball holds a marker near its centre
        assert m[cz - 1:cz + 2, cy - 1:cy + 2, cx - 1:cx + 2].any()
    assert np.array_equal(m, R.plateau_maxima(v, R.h_maxima(v, R.unit_distance(v), 1.0, 6), 6))


def test_the_marker_count_falls_with_h():
    counts = [C.label(scene_maxima(h), 6)[1] for h in (0.25, 1.0, 1.5, 3.0)]
    assert all(a >= b for a, b in zip(counts, counts[1:])) and counts[0] == 6 and counts[-1] >= 4, counts
    print("markers over h = 0.25, 1, 1.5, 3:", counts)


def test_the_corridor_visits_every_tile():
    v, path = R.corridor()
    assert v.sum() == len(path) == len(set(path)) and C.label(v, 26)[1] == 1
    tiles = {(z // 8, y // 8, x // 64) for z, y, x in path}
    assert len(tiles) == 3 * 3 * 3
    for a, b in zip(path, path[1:]):
        assert sum(abs(p - q) for p, q in zip(a, b)) == 1                             # a 6-connected walk


# ------------------------------------------------------------------ the plumbing
def test_exports_and_signatures():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert [s for s in syms if s.startswith("tomo_recon_")] == sorted(NEW_SYMBOLS)
    assert {"recon_calls", "recon_sweeps"} <= set(pipeline.COUNTERS)


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(7)]
    a, b, c, d, e, f, g = (ctypes.addressof(x) for x in bufs)                         # distinct host buffers, never dereferenced
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        assert L.tomo_recon_seed(a, b, c, 0, 1.0, *bad, d, e, None) == -1
        assert L.tomo_recon_sweep(a, *bad, 6, b, c, d, e, f, None) == -1
        assert L.tomo_recon_below(a, b, c, *bad, d, None) == -1
    big = (1 << 12, 1 << 13, 1 << 12)                                                 # 2^31 words
    assert L.tomo_recon_seed(a, b, c, 0, 1.0, *big, d, e, None) == -3
    assert L.tomo_recon_sweep(a, *big, 6, b, c, d, e, f, None) == -3
    assert L.tomo_recon_below(a, b, c, *big, d, None) == -3
    assert L.tomo_recon_sweep(a, 1 << 15, 1 << 15, 1 << 15, 26, b, c, d, e, f, None) == -3      # 2^31 tiles and more
    good = [a, b, c, 0, 1.0, 4, 4, 4, d, e]
    for k in (0, 1, 2, 8, 9):
        args = list(good)
        args[k] = None
        assert L.tomo_recon_seed(*args, None) == -1
    for mode in (-1, 3, 7):
        assert L.tomo_recon_seed(a, b, c, mode, 1.0, 4, 4, 4, d, e, None) == -1
    for h in (0.0, -1.0, float("nan"), float("inf"), 1e-50):                          # 1e-50 is 0.0 as a float32
        assert L.tomo_recon_seed(a, b, None, 1, h, 4, 4, 4, d, e, None) == -1
    assert L.tomo_recon_seed(a, b, c, 0, 1.0, 4, 4, 4, b, e, None) == -1              # g over the mask
    assert L.tomo_recon_seed(a, b, c, 0, 1.0, 4, 4, 4, c, e, None) == -1              # g over the marker
    assert L.tomo_recon_seed(a, b, c, 0, 1.0, 4, 4, 4, a, e, None) == -1              # g over the bits
    good = [a, 4, 4, 4, 26, b, c, d, e, f]
    for k in (0, 5, 6, 7, 8, 9):
        args = list(good)
        args[k] = None
        assert L.tomo_recon_sweep(*args, None) == -1
    for conn in (0, 4, 8, 18, 27, -6):
        assert L.tomo_recon_sweep(a, 4, 4, 4, conn, b, c, d, e, f, None) == -1
    assert L.tomo_recon_sweep(a, 4, 4, 4, 6, b, c, d, d, f, None) == -1               # one array for both sets of flags
    assert L.tomo_recon_sweep(a, 4, 4, 4, 6, b, b, d, e, f, None) == -1               # g over the mask
    for k in (0, 1, 2, 6):
        args = [a, b, c, 4, 4, 4, d]
        args[k] = None
        assert L.tomo_recon_below(*args, None) == -1
    for out in (a, b, c):                                                             # in place
        assert L.tomo_recon_below(a, b, c, 4, 4, 4, out, None) == -1
    assert L.tomo_recon_below(a, b, b, 4, 4, 4, d, None) == -1


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(pipeline._lib, "lib", boom)
    monkeypatch.setattr(volume_calculator, "to_device_volume", boom)


def host_volume(shape=(3, 4, 70)):
    return pipeline.BitVolume(torch.zeros((shape[0], shape[1], (shape[2] + 63) // 64), dtype=torch.int64), shape)


BAD_DEPTHS = (np.ones(4), np.ones(2), [], [1.0, 0.0, 1.0], [1.0, np.nan, 1.0])
BAD_PIXELS = (0.0, -0.5, np.nan, np.inf)
BAD_HEIGHTS = (0.0, -1.0, np.nan, np.inf, 1e-50, 1e39, None, "3", True)


def test_argument_errors(no_device):
    vol = host_volume()
    ok = torch.zeros(vol.shape, dtype=torch.float32)
    calls = {"reconstruct": lambda m, **k: pipeline.reconstruct(vol, m, ok, **k),
             "reconstruct marker": lambda m, **k: pipeline.reconstruct(vol, ok, m, **k),
             "h_maxima": lambda m, **k: pipeline.h_maxima(vol, m, k.pop("h", 1.0), **k),
             "regional_maxima": lambda m, **k: pipeline.regional_maxima(vol, m, **k),
             "extended_maxima": lambda m, **k: pipeline.extended_maxima(vol, m, k.pop("h", 1.0), **k)}
    for name, call in calls.items():
        for bad in (torch.zeros(vol.shape, dtype=torch.float64), torch.zeros(vol.shape, dtype=torch.int32), np.zeros(vol.shape, dtype=np.float32),
                    None, "map"):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (torch.zeros((3, 4, 71), dtype=torch.float32), torch.zeros((4, 70), dtype=torch.float32)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in (0, 18, 7, None):
            with pytest.raises(ValueError, match="connectivity"):
                call(ok, connectivity=bad)
        with pytest.raises(AssertionError, match="device"):                           # good arguments reach the device
            call(ok, connectivity=6)
    for bad in BAD_HEIGHTS:
        with pytest.raises(ValueError, match="h must be"):
            pipeline.h_maxima(vol, ok, bad)
        with pytest.raises(ValueError, match="h must be"):
            pipeline.extended_maxima(vol, ok, bad)
        with pytest.raises(ValueError, match="h_mm"):
            pipeline.separate_by_height(vol, bad)
        with pytest.raises(ValueError, match="h_mm"):
            pipeline.separate_by_height_with_contacts(vol, bad)
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in BAD_HEIGHTS:
        with pytest.raises(ValueError, match="h_mm"):
            volume_calculator.separate_grains_by_height(v, 0.9, 0.7, np.ones(3), bad)
        with pytest.raises(ValueError, match="h_mm"):
            volume_calculator.grain_contacts_by_height(v, 0.9, 0.7, np.ones(3), bad)
        if bad is not None:
            with pytest.raises(ValueError, match="h_mm"):
                volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), separate_h_mm=bad)
    for call in (lambda **k: pipeline.separate_by_height(vol, 1.0, **k), lambda **k: pipeline.separate_by_height_with_contacts(vol, 1.0, **k)):
        for bad in BAD_DEPTHS:
            with pytest.raises(ValueError):
                call(slice_depths=bad)
        for bad in BAD_PIXELS:
            with pytest.raises(ValueError):
                call(mm_per_pixel_y=bad)
            with pytest.raises(ValueError):
                call(mm_per_pixel_x=bad)
        for bad in (0, 18, None):
            with pytest.raises(ValueError, match="connectivity"):
                call(connectivity=bad)
        for bad in (-1, 2.5, np.nan, "3", True):
            with pytest.raises(ValueError, match="min_marker_voxels"):
                call(min_marker_voxels=bad)
        for bad in (-0.5, np.nan, np.inf, None, "1", True):
            with pytest.raises(ValueError, match="min_radius_mm"):
                call(min_radius_mm=bad)
        with pytest.raises(AssertionError, match="device"):
            call(slice_depths=[0.5, 1.0, 2.0], mm_per_pixel_y=0.7, min_radius_mm=0.5)
    for bad in (4, 12):
        with pytest.raises(ValueError):
            pipeline.separate_by_height_with_contacts(vol, 1.0, directions=bad)
    with pytest.raises(ValueError, match="separate_mm and separate_h_mm"):
        volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), separate_mm=1.0, separate_h_mm=1.0)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool)):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.separate_grains_by_height(bad, 0.9, 0.7, np.ones(3), 1.0)
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.grain_contacts_by_height(bad, 0.9, 0.7, np.ones(3), 1.0)
    with pytest.raises(ValueError, match="min_radius_mm"):
        volume_calculator.separate_grains_by_height(v, 0.9, 0.7, np.ones(3), 1.0, min_radius_mm=-1.0)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.separate_grains_by_height(v, 0.9, 0.7, np.ones(3), 1.0)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.grain_contacts_by_height(v, 0.9, 0.7, np.ones(3), 1.0)
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.component_properties(v, 0.9, 0.7, np.ones(3), separate_h_mm=1.0)


def test_the_volume_budget_raises_before_anything_is_allocated(no_device, monkeypatch):
    """extended_maxima and reconstruct hold three maps, regional_maxima and h_maxima two; a separation by height both budgets."""
    vol = host_volume()
    ok = torch.zeros(vol.shape, dtype=torch.float32)
    voxels = 3 * 4 * 70
    three = (lambda: pipeline.extended_maxima(vol, ok, 1.0), lambda: pipeline.reconstruct(vol, ok, ok.clone()),
             lambda: pipeline.separate_by_height(vol, 1.0))
    two = (lambda: pipeline.regional_maxima(vol, ok), lambda: pipeline.h_maxima(vol, ok, 1.0))
    for calls, nbytes in ((three, 12 * voxels), (two, 8 * voxels)):
        for call in calls:
            monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", nbytes - 1)
            with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET"):
                call()
            monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", nbytes)
            with pytest.raises(AssertionError, match="device"):
                call()


def test_signatures_and_defaults():
    def names(fn):
        return list(inspect.signature(fn).parameters)

    def default(fn, name):
        return inspect.signature(fn).parameters[name].default
    assert names(pipeline.reconstruct) == ["vol", "mask", "marker", "connectivity"]
    assert names(pipeline.h_maxima) == ["vol", "values", "h", "connectivity"]
    assert names(pipeline.regional_maxima) == ["vol", "values", "connectivity"]
    assert names(pipeline.extended_maxima) == ["vol", "values", "h", "connectivity"]
    for fn in (pipeline.reconstruct, pipeline.h_maxima, pipeline.regional_maxima, pipeline.extended_maxima):
        assert default(fn, "connectivity") == 26
    base = ["vol", "h_mm", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "min_marker_voxels", "min_radius_mm"]
    assert names(pipeline.separate_by_height) == base
    assert names(pipeline.separate_by_height_with_contacts) == base + ["directions"]
    assert default(pipeline.separate_by_height_with_contacts, "directions") == 13
    for fn in (pipeline.separate_by_height, pipeline.separate_by_height_with_contacts):
        assert [default(fn, n) for n in base[2:]] == [None, 1.0, 1.0, 6, 1, 0.0]
    grains = ["voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "h_mm", "connectivity", "min_marker_voxels", "min_radius_mm"]
    for fn in (volume_calculator.separate_grains_by_height, volume_calculator.grain_contacts_by_height):
        assert names(fn) == grains and [default(fn, n) for n in grains[5:]] == [6, 1, 0.0]
    p = names(volume_calculator.component_properties)
    assert default(volume_calculator.component_properties, "separate_h_mm") is None
    assert p[p.index("separate_mm") + 1] == "separate_h_mm"
    assert [f.name for f in pipeline.Separation.__dataclass_fields__.values()] == ["volume", "markers", "cut_voxels", "zones", "sweeps"]
    # the fixed-radius pair keeps its signatures
    assert names(pipeline.separate_components) == base[:1] + ["radius_mm"] + base[2:7]
    assert names(pipeline.separate_with_contacts) == base[:1] + ["radius_mm"] + base[2:7] + ["directions"]
