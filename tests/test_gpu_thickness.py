"""GPU tier: local thickness and ball openings of the resident bit volume in millimetres (csrc/distance.hip ->
pipeline.local_thickness / opening_volume -> volume_calculator.thickness_statistics).

Every expected value comes from tests/thickness_reference.py (NumPy; held against the all-pairs brute force by
tests/test_thickness_cpu.py) -- never from a second run of the code under test.  The volumes are uploaded as bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as E  # noqa: E402
import fenced as F  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, pipeline, volume_calculator  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = T.fixtures()
NAMES = list(FIXTURES)
# sided: the last radius is above every ball, so it is never launched and counts 0.  unit: D2 == r^2 and |pq|^2 == r^2 are hit
# exactly (every squared distance is an integer), which pins `>=` and `<`
RADII = {"sided": (0.6, 1.1, 1.7, 2.2, 9.0), "unit": (1.0, 1.5, 2.0, 3.0)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def resident(name, dev):
    v = FIXTURES[name]
    return v, pipeline.BitVolume(torch.from_numpy(E.pack(v)).to(dev), v.shape)


_cache = {}


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def base(name, kind):
    """(tables, inside D2) of the helper, computed once per case and left unchanged."""
    key = ("base", name, kind)
    if key not in _cache:
        v = FIXTURES[name]
        tabs = T.tables(v.shape, kind)
        d2 = E.edt_squared(v, *tabs, True)
        d2.setflags(write=False)
        _cache[key] = (tabs, d2)
    return _cache[key]


def expected_exact(name, kind):
    key = ("exact", name, kind)
    if key not in _cache:
        v = FIXTURES[name]
        tabs, d2 = base(name, kind)
        r2s = T.distinct_levels(v, d2)
        _cache[key] = frozen(T.expected(v, T.by_levels(v, d2, tabs, r2s), np.sqrt(r2s), T.slice_weights(v.shape, kind)))
    return _cache[key]


def expected_radii(name, kind, radii):
    key = ("radii", name, kind, tuple(radii))
    if key not in _cache:
        v = FIXTURES[name]
        tabs, d2 = base(name, kind)
        r = np.asarray(radii, dtype=np.float64)
        _cache[key] = frozen(T.expected(v, T.by_levels(v, d2, tabs, r * r), r, T.slice_weights(v.shape, kind)))
    return _cache[key]


def check_inputs_off_the_radii(name, kind, radii):
    """A condition on the INPUTS, not a tolerance on the result: no reference D2 of a set voxel and no outside squared distance
    to an eroded set lies within 1e-9 r^2 of an r^2, so the 1 ulp the transform is free in cannot move a decision."""
    v = FIXTURES[name]
    tabs, d2 = base(name, kind)
    for r in radii:
        r2 = r * r
        assert not (np.abs(d2[v] - r2) <= 1e-9 * r2).any(), "pick another radius: a D2 sits on r^2 (%s, %s, %r)" % (name, kind, r)
        out = T.cover(v, d2, tabs, r2)[1]
        if out is not None:
            fin = out[np.isfinite(out)]
            assert not (np.abs(fin - r2) <= 1e-9 * r2).any(), "pick another radius: an outside d2 sits on r^2 (%s, %s, %r)" % (name, kind, r)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_result(got, exp, v):
    assert isinstance(got, pipeline.LocalThickness)
    assert got.thickness.dtype == torch.float32 and tuple(got.thickness.shape) == v.shape and got.thickness.is_cuda
    th = got.thickness.cpu().numpy()
    assert same_bits(th, exp["thickness"])                                       # bit for bit: +0.0 at every unset voxel too
    assert not th[~v].any() and not np.signbit(th[~v]).any()
    assert got.radii_mm.dtype == np.float64 and same_bits(got.radii_mm, exp["radii_mm"])
    assert got.level_voxels.dtype == np.int64 and np.array_equal(got.level_voxels, exp["level_voxels"])
    assert got.level_volume_mm3.dtype == np.float64 and same_bits(got.level_volume_mm3, exp["level_volume_mm3"])
    assert type(got.uncovered_voxels) is int and got.uncovered_voxels == exp["uncovered_voxels"]
    assert got.uncovered_voxels + int(got.level_voxels.sum()) == int(v.sum())
    for key in ("mean_mm", "std_mm", "max_mm"):
        assert type(getattr(got, key)) is float and getattr(got, key) == exp[key], key


@pytest.mark.parametrize("kind", ["unit", "dyadic"])
@pytest.mark.parametrize("name", NAMES)
def test_exact_mode(dev, name, kind):
    v, vol = resident(name, dev)
    args = T.spacing(kind, v.shape[0])
    exp = expected_exact(name, kind)
    before = vol.bits.clone()
    c0 = pipeline.COUNTERS["local_thickness"]
    got = pipeline.local_thickness(vol, *args)
    assert pipeline.COUNTERS["local_thickness"] == c0 + 1
    print("%s/%s: %d levels, %d set voxels" % (name, kind, len(got.radii_mm), int(v.sum())))
    check_result(got, exp, v)
    assert got.uncovered_voxels == 0 and len(got.radii_mm) <= pipeline.LOCAL_THICKNESS_MAX_LEVELS
    th = got.thickness.cpu().numpy()
    own = pipeline.distance_transform(vol, *args).cpu().numpy()
    assert (th[v] >= 2 * own[v]).all()                                           # every set voxel lies in its own ball
    sphere = pipeline.inscribed_sphere(vol, *args)
    if sphere is None:
        assert name == "empty" and len(got.radii_mm) == 0 and (got.mean_mm, got.std_mm, got.max_mm) == (0.0, 0.0, 0.0)
        assert not th.any()
    else:
        top = np.float32(2 * sphere[0])
        assert abs(got.max_mm - float(top)) <= float(np.spacing(top)) and th.max() == np.float32(got.max_mm)
    assert torch.equal(vol.bits, before), "the input volume was modified"


@pytest.mark.parametrize("kind", ["sided", "unit"])
@pytest.mark.parametrize("name", NAMES)
def test_radii_mode(dev, name, kind):
    v, vol = resident(name, dev)
    radii = RADII[kind]
    if kind == "sided":
        check_inputs_off_the_radii(name, kind, radii)
    else:
        tabs, d2 = base(name, kind)
        assert np.array_equal(d2, np.rint(d2))                                   # integers: the ties below are exact
        if name in ("dumbbell", "edge"):
            assert (d2[v] == 4.0).any() and (T.cover(v, d2, tabs, 4.0)[1] == 4.0).any()
    exp = expected_radii(name, kind, radii)
    before = vol.bits.clone()
    got = pipeline.local_thickness(vol, *T.spacing(kind, v.shape[0]), radii_mm=list(radii))
    check_result(got, exp, v)
    assert len(got.radii_mm) == len(radii)
    if kind == "sided":
        assert got.level_voxels[-1] == 0 and got.level_volume_mm3[-1] == 0.0     # 9 mm: above every ball here
    assert torch.equal(vol.bits, before), "the input volume was modified"


@pytest.mark.parametrize("kind", ["sided", "unit"])
@pytest.mark.parametrize("name", NAMES)
def test_opening_volume(dev, name, kind):
    v, vol = resident(name, dev)
    args = T.spacing(kind, v.shape[0])
    tabs, d2 = base(name, kind)
    before = vol.bits.clone()
    c0 = pipeline.COUNTERS["opening_volume"]
    radii = RADII[kind][:4]
    if kind == "sided":
        check_inputs_off_the_radii(name, kind, radii)
    for r in radii:
        opened = T.cover(v, d2, tabs, r * r)[0]
        got = pipeline.opening_volume(vol, r, *args)
        assert got.shape == vol.shape and got.bits.dtype == torch.int64 and got.bits.data_ptr() != vol.bits.data_ptr()
        assert np.array_equal(got.bits.cpu().numpy(), E.pack(opened)), (name, kind, r)      # whole words: the tail bits too
        one = pipeline.local_thickness(vol, *args, radii_mm=[r])
        assert np.array_equal(one.thickness.cpu().numpy() > 0, opened), (name, kind, r)
    same = pipeline.opening_volume(vol, 0, *args)
    assert same.bits.data_ptr() != vol.bits.data_ptr() and torch.equal(same.bits, vol.bits)
    assert pipeline.COUNTERS["opening_volume"] == c0 + len(radii) + 1
    assert torch.equal(vol.bits, before), "the input volume was modified"


@pytest.mark.parametrize("words", [0, 2])
@pytest.mark.parametrize("name", ["edge", "dumbbell"])
def test_chunked_workspace(dev, monkeypatch, name, words):
    """The same answers when every transform of the call goes through the workspace in several chunks of 64-column words."""
    v, vol = resident(name, dev)
    nz, ny, nx = v.shape
    L = pipeline._lib.lib()
    budget = words * L.tomo_edt_workspace_bytes(nz, ny, nx, 0)
    monkeypatch.setattr(pipeline, "EDT_WORKSPACE_BUDGET", budget)
    cw = L.tomo_edt_chunk_columns(nz, ny, nx, L.tomo_edt_workspace_bytes(nz, ny, nx, budget))
    assert cw == 64 * max(words, 1) and -(-nx // cw) == {("edge", 0): 3, ("edge", 2): 2, ("dumbbell", 0): 2, ("dumbbell", 2): 1}[name, words]
    check_result(pipeline.local_thickness(vol, *T.spacing("unit", nz)), expected_exact(name, "unit"), v)
    radii = RADII["sided"]
    check_inputs_off_the_radii(name, "sided", radii)
    args = T.spacing("sided", nz)
    check_result(pipeline.local_thickness(vol, *args, radii_mm=radii), expected_radii(name, "sided", radii), v)
    tabs, d2 = base(name, "sided")
    got = pipeline.opening_volume(vol, radii[1], *args)
    assert np.array_equal(got.bits.cpu().numpy(), E.pack(T.cover(v, d2, tabs, radii[1] * radii[1])[0]))


def test_too_many_levels_names_radii_mm(dev):
    v, vol = resident("dumbbell", dev)
    assert len(expected_exact("dumbbell", "unit")["radii_mm"]) > 1
    with pytest.raises(ValueError, match="radii_mm"):
        pipeline.local_thickness(vol, max_levels=1)
    n = len(expected_exact("dumbbell", "unit")["radii_mm"])
    with pytest.raises(ValueError, match="radii_mm"):
        pipeline.local_thickness(vol, max_levels=n - 1)
    check_result(pipeline.local_thickness(vol, max_levels=n), expected_exact("dumbbell", "unit"), v)


def test_volume_budget_is_checked_before_any_allocation(dev, monkeypatch):
    v, vol = resident("plate", dev)
    monkeypatch.setattr(pipeline, "LOCAL_THICKNESS_VOLUME_BUDGET", 1)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    c0 = pipeline.COUNTERS["local_thickness"]
    with F.fenced("zero", F.package_modules()) as fz:
        with pytest.raises(ValueError, match="LOCAL_THICKNESS_VOLUME_BUDGET"):
            pipeline.local_thickness(vol)
        with pytest.raises(ValueError, match="LOCAL_THICKNESS_VOLUME_BUDGET"):
            pipeline.local_thickness(vol, radii_mm=[1.0])
        assert fz.total == 0
    assert torch.cuda.memory_allocated() == held and pipeline.COUNTERS["local_thickness"] == c0


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
@pytest.mark.parametrize("name", ["edge", "shell"])
def test_fenced(dev, poison, name):
    v, vol = resident(name, dev)
    nz = v.shape[0]
    radii = RADII["sided"]
    check_inputs_off_the_radii(name, "sided", radii)
    sided, unit = T.spacing("sided", nz), T.spacing("unit", nz)
    exp_exact, exp_radii = expected_exact(name, "unit"), expected_radii(name, "sided", radii)
    tabs, d2 = base(name, "sided")
    exp_open = E.pack(T.cover(v, d2, tabs, radii[1] * radii[1])[0])

    def once(p):
        with F.fenced(p, F.package_modules(), seed=11) as fz:
            with fz.unchanged(vol.bits):
                check_result(pipeline.local_thickness(vol, *unit), exp_exact, v)
                check_result(pipeline.local_thickness(vol, *sided, radii_mm=radii), exp_radii, v)
                assert np.array_equal(pipeline.opening_volume(vol, radii[1], *sided).bits.cpu().numpy(), exp_open)
            fz.check()
            assert fz.ran("__init__") >= 3 and fz.ran("local_thickness") >= 8 and fz.ran("opening_volume") == 2
    try:
        once(poison)
    except AssertionError as e:
        try:
            once("zero")
            control = "the zero control PASSES: the failure is a read of memory nobody wrote"
        except AssertionError as z:
            control = "the zero control fails too (%s): not a matter of the poison" % (str(z).splitlines() or [""])[0][:200]
        raise AssertionError("%s\n[%s] %s (%s)" % (e, poison, control, name)) from e


# ------------------------------------------------------------------ the drop-in layer
@pytest.mark.parametrize("name", ["dumbbell", "shell", "empty"])
def test_thickness_statistics(dev, name):
    v = np.ascontiguousarray(FIXTURES[name])
    nz = v.shape[0]
    for kind, radii in (("dyadic", None), ("sided", RADII["sided"])):
        depths, mm_y, mm_x = T.spacing(kind, nz)
        if radii is not None:
            check_inputs_off_the_radii(name, kind, radii)
        exp = expected_exact(name, kind) if radii is None else expected_radii(name, kind, radii)
        _devcache.clear()
        got = volume_calculator.thickness_statistics(v, mm_x, mm_y, depths, radii_mm=radii)
        _devcache.clear()
        assert set(got) == {'mean_mm', 'std_mm', 'max_mm', 'uncovered_voxels', 'histogram'}
        assert (got['mean_mm'], got['std_mm'], got['max_mm']) == (exp["mean_mm"], exp["std_mm"], exp["max_mm"])
        assert got['uncovered_voxels'] == exp["uncovered_voxels"]
        hist = [(2.0 * float(r), int(n), float(w)) for r, n, w in zip(exp["radii_mm"], exp["level_voxels"], exp["level_volume_mm3"])]
        assert got['histogram'] == hist and all(type(a) is float and type(b) is int and type(c) is float for a, b, c in got['histogram'])
        if name == "empty":
            assert (got['mean_mm'], got['std_mm'], got['max_mm'], got['uncovered_voxels']) == (0.0, 0.0, 0.0, 0)
            assert got['histogram'] == ([] if radii is None else [(2.0 * r, 0, 0.0) for r in radii])
