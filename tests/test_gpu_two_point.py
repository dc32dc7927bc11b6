"""GPU tier: the two-point covariance of the resident bit volume over a box of integer lags (csrc/two_point.hip: tomo_two_point
-> pipeline.two_point -> volume_calculator.two_point_report).

The table is compared with == against tests/two_point_reference.py -- shifted slices and np.count_nonzero, held to the float64
FFT autocorrelation, to a loop over all voxel pairs and to hand values by tests/test_two_point_cpu.py -- never with a second run
of the code under test.  The floats are compared bit for bit: they come from the same host functions
(pipeline.two_point_from_table and the methods of TwoPoint) on the reference's integers.  Both phases: the background equals the
object of the inverted volume."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chords_reference as CH  # noqa: E402
import components_reference as C  # noqa: E402
import fenced as F  # noqa: E402
import two_point_reference as R  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
KEY = "two_point"
SHAPE = (19, 21, 150)                                            # x crosses 63|64 and 127|128 and has a 22-bit tail
PHASES = ("object", "background")
# every RX variant (8, 16, 32, 63) at its full width and narrower than it (Rx = 7, 15, 31 and 0: only the columns |hx| <= Rx are
# flushed), ints
BOXES = ((4, 5, 63), (0, 0, 0), (18, 20, 7), (2, 0, 31), (0, 3, 15), 1, 16, (1, 2, 32), (3, 1, 8))
LARGER = (41, 30, 63)                                            # reaches past (5, 7, 150) and the narrow shapes on every axis it can
ODD = np.array([0.5, 0.5, 1.0, 0.25, 2.0, 0.3, 0.75])


def _set(shape, *at):
    v = np.zeros(shape, dtype=bool)
    for p in at:
        v[p] = True
    return v


def add(p, o, t=1):
    return tuple(int(a + t * b) for a, b in zip(p, o))


def pair_at_the_seams(step):
    """Two voxels one step apart in (2, 3, 66): across x = 63|64 where the step has an x part, into the last row where it goes up
    in y, into the top slice where it goes up in z (the seam pair of tests/test_gpu_chords.py)."""
    p = (0, 1, 64 if step[2] < 0 else 63)
    return _set((2, 3, 66), p, add(p, step))


def bar_at_the_seams(step):
    """Five voxels along the step in (6, 7, 130): across x = 63|64, into the last row (dy > 0) or the first (dy < 0), into the top
    slice (dz > 0) (the seam bar of tests/test_gpu_chords.py)."""
    p = (1 if step[0] else 2, {1: 2, -1: 4, 0: 3}[step[1]], {1: 61, -1: 66, 0: 63}[step[2]])
    return _set((6, 7, 130), *[add(p, step, t) for t in range(5)])


NARROW = ((23, 5, 70), (5, 23, 3), (40, 3, 2), (1, 9, 70), (9, 1, 130), (5, 6, 64), (5, 6, 65))


def fixtures():
    out = {}
    for d in (10, 30, 50, 90):
        out["noise_%03d" % d] = R.noise(d / 100.0, SHAPE, seed=d)
    out["full"] = np.ones((5, 7, 150), dtype=bool)
    out["empty"] = np.zeros((5, 7, 150), dtype=bool)
    out["one_voxel"] = np.ones((1, 1, 1), dtype=bool)
    nz, ny, nx = 3, 4, 150
    out["corners"] = _set((nz, ny, nx), *[(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)])
    for step in CH.FORWARD:
        out["pair_%d_%d_%d" % step] = pair_at_the_seams(step)
        out["bar_%d_%d_%d" % step] = bar_at_the_seams(step)
    for shape in NARROW:
        out["narrow_%d_%d_%d" % shape] = R.noise(0.5, shape, seed=shape[0])
    return out


FIXTURES = fixtures()
SMALL = [n for n in FIXTURES if n.startswith(("pair_", "bar_", "one_voxel", "corners"))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def upload(v, dev):
    return pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


_ref = {}


def reference(name, box, phase):
    """The reference's table of a fixture, computed once per (case, box, phase) and left unchanged."""
    key = (name, R.box(box), phase)
    if key not in _ref:
        v = FIXTURES[name] if phase == "object" else ~FIXTURES[name]
        _ref[key] = R.pairs(v, *R.box(box))
        _ref[key].setflags(write=False)
    return _ref[key]


def same_bytes(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same(got, v, N, box, spacing, depths, phase, what):
    """A TwoPoint of the device against the reference's table N of the bool volume v (the phase already applied)."""
    box = R.box(box)
    assert got.pairs.dtype == np.int64 and got.pairs.shape == N.shape, (what, got.pairs.shape)
    assert np.array_equal(got.pairs, N), (what, np.argwhere(got.pairs != N)[:6].tolist())
    assert got.max_lag == box and got.shape == v.shape and got.voxels == int(v.sum()) and got.phase == phase, what
    assert np.array_equal(got.pairs[0], got.pairs[0, ::-1, ::-1]), (what, "the plane hz = 0 is not point-symmetric")
    exp = pipeline.two_point_from_table(N, box, v.shape, spacing, phase, depths)
    assert got.spacing == exp.spacing
    same_bytes(got.inside(), R.inside(v.shape, box), what)
    for name in ("s2", "covariance", "correlation", "lag_mm", "directional", "correlation_length_mm"):
        same_bytes(getattr(got, name)(), getattr(exp, name)(), (what, name))
    for a, b in zip(got.radial(max(spacing)), exp.radial(max(spacing))):
        same_bytes(a, b, (what, "radial"))
    if min(box) >= 1:
        same_bytes(got.specific_surface_per_mm(), exp.specific_surface_per_mm(), what)
    assert got.s2()[0, box[1], box[2]] == v.sum() / v.size


def check_case(name, dev, boxes, phases=PHASES, odd=False):
    v = FIXTURES[name]
    vol = upload(v, dev)
    before = vol.bits.clone()
    nz = v.shape[0]
    depths, mm_y, mm_x = (np.resize(ODD, nz).copy(), 0.45, 0.7) if odd else (None, 1.0, 1.0)
    spacing = (1.0 if depths is None else float(np.mean(depths)), mm_y, mm_x)
    for box in boxes:
        for phase in phases:
            c0 = pipeline.COUNTERS[KEY]
            got = pipeline.two_point(vol, box, depths, mm_y, mm_x, phase)
            assert pipeline.COUNTERS[KEY] == c0 + 1
            same(got, v if phase == "object" else ~v, reference(name, box, phase), box, spacing, depths, phase, (name, box, phase))
    assert torch.equal(vol.bits, before), "the input volume was modified"
    return vol


@pytest.mark.parametrize("name", [n for n in FIXTURES if n not in SMALL])
def test_table_equals_the_reference(dev, name):
    """Noise, full, empty and the narrow shapes over every box, both phases: every RX variant, both truncations, lags beyond the
    axes -- (18, 20, 7) and 16 reach the last slice and row of the noise, LARGER goes past every axis of the others."""
    check_case(name, dev, BOXES if name.startswith("noise_") else BOXES + (LARGER,), odd=name == "noise_030")


@pytest.mark.parametrize("name", SMALL)
def test_seams_and_corners(dev, name):
    check_case(name, dev, ((4, 5, 63), 1, (2, 0, 31), (7, 8, 15)))


def test_the_hand_values(dev):
    one = pipeline.two_point(upload(FIXTURES["one_voxel"], dev), (2, 2, 2))
    assert one.pairs.sum() == 1 and one.pairs[0, 2, 2] == 1 and one.voxels == 1
    assert not pipeline.two_point(upload(FIXTURES["one_voxel"], dev), 3, phase="background").pairs.any()
    for s in CH.FORWARD:
        got = pipeline.two_point(upload(FIXTURES["pair_%d_%d_%d" % s], dev), 1).pairs
        exp = np.zeros((2, 3, 3), dtype=np.int64)
        exp[0, 1, 1] = 2
        exp[s[0], s[1] + 1, s[2] + 1] = 1
        if s[0] == 0:
            exp[0, 1 - s[1], 1 - s[2]] = 1
        assert np.array_equal(got, exp), s
    full = pipeline.two_point(upload(FIXTURES["full"], dev), (6, 8, 63))
    assert np.array_equal(full.pairs, full.inside()) and np.array_equal(full.pairs, R.inside((5, 7, 150), (6, 8, 63)))
    assert not full.pairs[5:].any() and not full.pairs[:, :1].any()                      # hz >= nz, |hy| >= ny read 0


def test_background_is_the_object_of_the_inverted_volume(dev):
    v = FIXTURES["noise_030"]
    a = pipeline.two_point(upload(v, dev), (4, 5, 63), phase="background")
    b = pipeline.two_point(upload(~v, dev), (4, 5, 63), phase="object")
    same_bytes(a.pairs, b.pairs, "inverted")
    again = pipeline.two_point(upload(v, dev), (4, 5, 63), phase="background")           # the same bytes on every run
    same_bytes(a.pairs, again.pairs, "second run")
    assert np.array_equal(a.pairs, reference("noise_030", (4, 5, 63), "background"))


def test_set_tail_bits_are_not_trusted(dev):
    """The same volume uploaded with every bit past nx SET in each row's last word, built from raw words."""
    for name in ("noise_030", "narrow_5_6_65", "narrow_5_23_3"):
        v = FIXTURES[name]
        words = C.pack(v).copy().view(np.uint64)
        tail = v.shape[2] % 64
        assert tail
        words[..., -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(tail)
        vol = pipeline.BitVolume(torch.from_numpy(words.view(np.int64)).to(dev), v.shape)
        before = vol.bits.clone()
        for box in ((4, 5, 63), (2, 0, 31), 1):
            for phase in PHASES:
                got = pipeline.two_point(vol, box, phase=phase)
                assert np.array_equal(got.pairs, reference(name, box, phase)), (name, box, phase)
        assert torch.equal(vol.bits, before)


def test_chords_and_pairs_agree_on_the_device(dev):
    """sum (n - 1) counts[m][n] of chord_lengths == N(s_m) of two_point, both from the device."""
    vol = upload(FIXTURES["noise_030"], dev)
    c = pipeline.chord_lengths(vol)
    t = pipeline.two_point(vol, 1)
    n = np.arange(c.counts.shape[1])
    for m, s in enumerate(CH.FORWARD):
        assert int(((n - 1) * c.counts[m])[1:].sum()) == int(t.pairs[s[0], s[1] + 1, s[2] + 1]), s
    same_bytes(t.directional()[:, 1], c.lineal_path()[:, 2], "the lineal path at r = 2 is S2 at the step")


def test_scale(dev):
    """(6, 520, 1030) at (2, 3, 63): 17 words a row, 53 040 words in 208 chunks for each of 21 planes -- 4368 workgroups, more
    than the card keeps resident.  Against the FFT reference, and against the shifted slices at (1, 1, 63)."""
    v = R.noise(0.3, (6, 520, 1030), seed=42)
    vol = upload(v, dev)
    got = pipeline.two_point(vol, (2, 3, 63))
    exp, off = R.pairs_fft(v, 2, 3, 63)
    assert off < 0.25, off
    assert np.array_equal(got.pairs, exp), np.argwhere(got.pairs != exp)[:6].tolist()
    assert got.voxels == int(v.sum()) and np.array_equal(got.pairs[0], got.pairs[0, ::-1, ::-1])
    small = pipeline.two_point(vol, (1, 1, 63))
    assert np.array_equal(small.pairs, R.pairs(v, 1, 1, 63))
    assert np.array_equal(small.pairs, got.pairs[:2, 2:5])


# ------------------------------------------------------------------ the raw entry point
def test_raw_abi(dev):
    v = FIXTURES["noise_010"]
    vol = upload(v, dev)
    L, st = _lib.lib(), _stream()
    nz, ny, nx = v.shape
    rz, ry, rx = 4, 5, 63
    out = torch.full(((rz + 1) * (2 * ry + 1) * (2 * rx + 1),), 77, dtype=torch.int64, device=dev)
    args = [_p(vol.bits), nz, ny, nx, rz, ry, rx, _p(out), st]
    for hole in (0, 7):
        assert L.tomo_two_point(*[None if i == hole else a for i, a in enumerate(args)]) == -1
    for i, value in ((1, 0), (2, -3), (3, 0), (4, -1), (5, -1), (6, -1), (6, 64)):
        assert L.tomo_two_point(*[value if j == i else a for j, a in enumerate(args)]) == -1
    assert L.tomo_two_point(_p(vol.bits), 1 << 20, 1 << 11, 64, rz, ry, rx, _p(out), st) == -3
    assert L.tomo_two_point(_p(vol.bits), nz, ny, nx, 1 << 15, 1 << 15, 0, _p(out), st) == -3
    torch.cuda.synchronize()
    assert out.eq(77).all(), "a refused call wrote to the table"
    _lib.check(L.tomo_two_point(*args), "tomo_two_point")        # ... and the table is zeroed by the call itself
    got = out.cpu().numpy().reshape(rz + 1, 2 * ry + 1, 2 * rx + 1)
    assert np.array_equal(got, reference("noise_010", (rz, ry, rx), "object"))


def test_argument_errors(dev):
    vol = upload(FIXTURES["noise_010"], dev)
    c0 = pipeline.COUNTERS[KEY]
    for bad in ({"phase": "pores"}, {"max_lag": -1}, {"max_lag": (1, 1, 64)}, {"max_lag": 1.5}, {"slice_depths": np.ones(3)},
                {"mm_per_pixel_y": 0.0}):
        with pytest.raises(ValueError):
            pipeline.two_point(vol, **bad)
    assert pipeline.COUNTERS[KEY] == c0, "a refused call reached the kernel"


# ------------------------------------------------------------------ the report
def test_two_point_report(dev):
    v = FIXTURES["noise_030"]
    nz = v.shape[0]
    d, mm_y, mm_x = np.resize(ODD, nz).copy(), 0.45, 0.7
    box = (4, 5, 63)
    c0 = pipeline.COUNTERS[KEY]
    got = volume_calculator.two_point_report(v, d, mm_y, mm_x, max_lag=box)
    assert pipeline.COUNTERS[KEY] == c0 + 2
    assert list(got) == ["max_lag", "object", "background", "cross"] and got["max_lag"] == box
    tables = {}
    for phase in PHASES:
        N = reference("noise_030", box, phase)
        t = tables[phase] = pipeline.two_point_from_table(N, box, v.shape, (float(np.mean(d)), mm_y, mm_x), phase, d)
        r = got[phase]
        assert list(r) == ["volume_fraction", "specific_surface_per_mm", "correlation_length_mm", "directional", "radial"]
        assert r["volume_fraction"] == t.volume_fraction() == t.voxels / v.size
        assert r["specific_surface_per_mm"] == t.specific_surface_per_mm() and r["specific_surface_per_mm"] > 0
        assert type(r["correlation_length_mm"]) is list and len(r["correlation_length_mm"]) == 13
        same_bytes(np.array(r["correlation_length_mm"]), t.correlation_length_mm(), phase)
        same_bytes(r["directional"], t.directional(), phase)
        assert list(r["radial"]) == ["bin_mm", "centres_mm", "values", "lags"] and r["radial"]["bin_mm"] == max(t.spacing)
        for a, b in zip((r["radial"]["centres_mm"], r["radial"]["values"], r["radial"]["lags"]), t.radial(max(t.spacing))):
            same_bytes(a, b, phase)
    P = R.inside(v.shape, box)
    cross = (P - tables["object"].pairs - tables["background"].pairs).astype(np.float64) / (2 * P).astype(np.float64)
    same_bytes(got["cross"], cross, "cross")
    assert got["cross"][0, box[1], box[2]] == 0.0 and (got["cross"] >= 0).all() and (got["cross"] <= 0.5).all()
    only = volume_calculator.two_point_report(v, d, mm_y, mm_x, max_lag=box, background=False)
    assert list(only) == ["max_lag", "object", "background", "cross"] and only["background"] is None and only["cross"] is None
    assert only["object"]["correlation_length_mm"] == got["object"]["correlation_length_mm"]
    flat = volume_calculator.two_point_report(v, d, mm_y, mm_x, max_lag=(0, 2, 2), background=False)
    assert flat["object"]["specific_surface_per_mm"] is None and flat["max_lag"] == (0, 2, 2)
    nothing = volume_calculator.two_point_report(FIXTURES["empty"], np.ones(5), 1.0, 1.0, max_lag=(6, 2, 7))     # NaNs, no exception
    assert nothing["object"]["volume_fraction"] == 0.0 and np.isnan(nothing["object"]["correlation_length_mm"]).all()
    assert nothing["object"]["specific_surface_per_mm"] == 0.0 and nothing["background"]["volume_fraction"] == 1.0
    assert np.isnan(nothing["cross"][5:]).all() and not nothing["cross"][:5].any()
    assert np.isnan(nothing["object"]["directional"][8:, 5:]).all()                      # hz >= nz: P = 0
    with pytest.raises(TypeError):
        volume_calculator.two_point_report(v.astype(np.uint8), d, mm_y, mm_x)
    with pytest.raises(ValueError):
        volume_calculator.two_point_report(v, np.ones(3), mm_y, mm_x)
    _devcache.clear()
    _memo.clear()


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_fenced(dev, poison):
    """Noise, the narrow shapes and the set tail bits inside fenced, poisoned buffers: the same integers, clean fences."""
    names = ["noise_030", "noise_090"] + [n for n in FIXTURES if n.startswith("narrow_")]
    vols = {name: upload(FIXTURES[name], dev) for name in names}
    v = FIXTURES["noise_030"]
    words = C.pack(v).copy().view(np.uint64)
    words[..., -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(v.shape[2] % 64)
    dirty = pipeline.BitVolume(torch.from_numpy(words.view(np.int64)).to(dev), v.shape)
    boxes = ((4, 5, 63), (2, 3, 15))

    def once(p):
        with F.fenced(p, F.package_modules(), seed=7) as fz:
            for name in names + ["tail_bits"]:
                vol = dirty if name == "tail_bits" else vols[name]
                ref = "noise_030" if name == "tail_bits" else name
                with fz.unchanged(vol.bits):
                    for box in boxes:
                        for phase in PHASES:
                            got = pipeline.two_point(vol, box, phase=phase)
                            assert np.array_equal(got.pairs, reference(ref, box, phase)), ("fenced", name, box, phase)
            fz.check()
            assert fz.ran("two_point") >= 3 * len(boxes) * (len(names) + 1)                # the table twice, the complement once
    try:
        once(poison)
    except AssertionError as e:
        try:
            once("zero")
            control = "the zero control PASSES: the failure is a read of memory nobody wrote"
        except AssertionError as z:
            control = "the zero control fails too (%s): not a matter of the poison" % (str(z).splitlines() or [""])[0][:200]
        raise AssertionError("%s\n[%s] %s" % (e, poison, control)) from e
