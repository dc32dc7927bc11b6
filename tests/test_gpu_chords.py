"""GPU tier: chord lengths of the resident bit volume along the 13 lattice directions (csrc/chords.hip: tomo_chord_hist ->
pipeline.chord_lengths -> volume_calculator.chord_report).

counts, border and sum_q are compared with == against tests/chords_reference.py -- running lengths carried from slab to slab
in NumPy, held to a walk over every voxel and to hand values by tests/test_chords_cpu.py -- never with a second run of the code
under test.  The floats are compared bit for bit: they come from the same host functions (pipeline.chord_lengths_from_tables and
the methods of ChordLengths) on the same integers.  Both phases: the background equals the object of the inverted volume."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chords_reference as R  # noqa: E402
import components_reference as C  # noqa: E402
import fenced as F  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
KEY = "chord_lengths"
SHAPE = (19, 21, 150)                                            # x crosses 63|64 and 127|128 and has a 22-bit tail
SPACINGS = ("unit", "dyadic", "odd")
PHASES = ("object", "background")


def spacing(kind, nz):
    """The spacings of tests/test_gpu_breadth.py -> (slice_depths, mm_y, mm_x): unit, dyadic (2, 1, 0.5), odd with varying depths."""
    if kind == "unit":
        return None, 1.0, 1.0
    if kind == "dyadic":
        return np.full(nz, 2.0), 1.0, 0.5
    return np.resize(np.array([0.5, 0.5, 1.0, 0.25, 2.0, 0.3, 0.75]), nz).copy(), 0.45, 0.7


def _set(shape, *at):
    v = np.zeros(shape, dtype=bool)
    for p in at:
        v[p] = True
    return v


def add(p, o, t=1):
    return tuple(int(a + t * b) for a, b in zip(p, o))


def pair_at_the_seams(step):
    """Two voxels one step apart in (2, 3, 66): across x = 63|64 where the step has an x part, into the last row where it goes up
    in y, into the top slice where it goes up in z."""
    p = (0, 1, 64 if step[2] < 0 else 63)
    return _set((2, 3, 66), p, add(p, step))


def bar_at_the_seams(step):
    """Five voxels along the step in (6, 7, 130): across x = 63|64, into the last row (dy > 0) or the first (dy < 0), into the top
    slice (dz > 0)."""
    p = (1 if step[0] else 2, {1: 2, -1: 4, 0: 3}[step[1]], {1: 61, -1: 66, 0: 63}[step[2]])
    return _set((6, 7, 130), *[add(p, step, t) for t in range(5)])


WRAPS = ((23, 5, 70), (5, 23, 3), (40, 3, 2), (1, 9, 70), (9, 1, 130), (5, 6, 64), (5, 6, 65))


def fixtures():
    out = {}
    for d in (10, 30, 50, 90):
        out["noise_%03d" % d] = R.noise(d / 100.0, SHAPE, seed=d)
    out["full"] = np.ones((5, 7, 150), dtype=bool)
    out["empty"] = np.zeros((5, 7, 150), dtype=bool)
    out["one_voxel"] = np.ones((1, 1, 1), dtype=bool)
    nz, ny, nx = 3, 4, 150
    out["corners"] = _set((nz, ny, nx), *[(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)])
    for step in R.FORWARD:
        out["pair_%d_%d_%d" % step] = pair_at_the_seams(step)
        out["bar_%d_%d_%d" % step] = bar_at_the_seams(step)
    out["diagonals"] = _set((9, 9, 130), *([(t, t, 60 + t) for t in range(9)] + [(t, 8 - t, 129 - t) for t in range(9)]))
    for shape in WRAPS:
        out["wrap_noise_%d_%d_%d" % shape] = R.noise(0.5, shape, seed=shape[0])
        out["wrap_full_%d_%d_%d" % shape] = np.ones(shape, dtype=bool)
    out["long_x"] = np.ones((3, 4, 1100), dtype=bool)             # chords past the bins a workgroup keeps
    out["long_z"] = np.ones((1100, 3, 4), dtype=bool)
    for axis in range(3):                                        # four lines of one workgroup along each axis, their lengths 256 apart
        shape = tuple(600 if a == axis else 2 for a in range(3))  # in pairs: both want one slot of the bins for long chords
        v = np.zeros(shape, dtype=bool)
        for line, length in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (300, 556, 600, 344)):
            at = [slice(0, length) if a == axis else None for a in range(3)]
            at[[a for a in range(3) if a != axis][0]], at[[a for a in range(3) if a != axis][1]] = line
            v[tuple(at)] = True
        out["slots_%s" % "zyx"[axis]] = v
    return out


FIXTURES = fixtures()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def upload(v, dev):
    return pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


_ref = {}


def reference(name, kind, phase):
    """The reference's tables of a fixture, computed once per (case, spacing, phase) and left unchanged."""
    if (name, kind, phase) not in _ref:
        v = FIXTURES[name] if phase == "object" else ~FIXTURES[name]
        d, mm_y, mm_x = spacing(kind, v.shape[0])
        t = R.tables(v, R.steps_q(R.steps(d, v.shape[0], mm_y, mm_x)))
        for a in t:
            a.setflags(write=False)
        _ref[(name, kind, phase)] = t
    return _ref[(name, kind, phase)]


def same_bytes(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same(got, v, tables, kind, what):
    """A ChordLengths of the device against the reference's tables of the bool volume v (the phase already applied)."""
    nz = v.shape[0]
    d, mm_y, mm_x = spacing(kind, nz)
    L = max(v.shape)
    for name, a, b in zip(("counts", "border", "sum_q"), (got.counts, got.border, got.sum_q), tables):
        assert a.dtype == np.int64 and a.shape == (13, L + 1), (what, name, a.shape)
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:6].tolist())
    steps = R.steps(d, nz, mm_y, mm_x)
    same_bytes(got.steps, steps, what)
    exp = pipeline.chord_lengths_from_tables(tables, v.sum(axis=(1, 2)), steps, v.shape,
                                             (1.0 if d is None else float(np.mean(d)), mm_y, mm_x))
    assert got.voxels == int(v.sum()) and got.shape == v.shape and got.spacing == exp.spacing
    assert ((got.counts * np.arange(L + 1)).sum(axis=1) == v.sum()).all(), what          # the invariant
    same_bytes(got.directions, np.array(R.FORWARD, dtype=np.int64), what)
    same_bytes(got.chords, tables[0].sum(axis=1), what)
    total = np.zeros(13)
    for k in range(nz):                                          # the sequential sum of the definition, written out
        total = total + float(v[k].sum()) * steps[k]
    same_bytes(got.total_length_mm, total, what)
    same_bytes(got.mean_chord_mm, exp.mean_chord_mm, what)
    assert np.isnan(got.mean_chord_mm[got.chords == 0]).all()
    same_bytes(got.mean_length_mm(), exp.mean_length_mm(), what)
    for interior in (False, True):
        same_bytes(got.lineal_path(interior), exp.lineal_path(interior), what)
    same_bytes(got.quantiles_mm(), exp.quantiles_mm(), what)
    assert (got.lineal_path()[:, 1] == v.sum() / v.size).all()


def check_case(name, dev, kinds=SPACINGS, phases=PHASES):
    v = FIXTURES[name]
    vol = upload(v, dev)
    before = vol.bits.clone()
    for kind in kinds:
        d, mm_y, mm_x = spacing(kind, v.shape[0])
        for phase in phases:
            c0 = pipeline.COUNTERS[KEY]
            got = pipeline.chord_lengths(vol, d, mm_y, mm_x, phase)
            assert pipeline.COUNTERS[KEY] == c0 + 1
            same(got, v if phase == "object" else ~v, reference(name, kind, phase), kind, (name, kind, phase))
    assert torch.equal(vol.bits, before), "the input volume was modified"
    return vol


@pytest.mark.parametrize("name", list(FIXTURES))
def test_tables_equal_the_reference(dev, name):
    """Every fixture under the three spacings and both phases (the long lines under the varying depths alone: the reference
    carries its running lengths along them step by step)."""
    check_case(name, dev, kinds=("odd",) if name in ("long_z", "slots_z", "slots_y", "slots_x") else SPACINGS)


def test_the_hand_values(dev):
    got = pipeline.chord_lengths(upload(np.ones((4, 5, 6), dtype=bool), dev))
    m = R.FORWARD.index((1, 1, 1))
    assert got.counts[m].tolist() == [0, 24, 18, 12, 6, 0, 0] and got.border[m].tolist() == got.counts[m].tolist()
    assert got.counts[0].tolist() == [0, 0, 0, 0, 0, 0, 20] and got.chords.tolist() == got.counts.sum(axis=1).tolist()
    one = pipeline.chord_lengths(upload(FIXTURES["one_voxel"], dev), [0.3], 0.45, 0.7)
    assert one.counts.tolist() == [[0, 1]] * 13 and one.border.tolist() == [[0, 1]] * 13
    assert one.sum_q[:, 1].tolist() == R.steps_q(R.steps([0.3], 1, 0.45, 0.7))[0].tolist()
    empty = pipeline.chord_lengths(upload(FIXTURES["one_voxel"], dev), phase="background")
    assert not empty.counts.any() and empty.voxels == 0 and np.isnan(empty.mean_chord_mm).all()
    bar = pipeline.chord_lengths(upload(FIXTURES["bar_0_0_1"], dev))
    assert bar.counts[0, 5] == 1 and bar.counts[0].sum() == 1 and (bar.counts[1:, 1] == 5).all() and not bar.border.any()


def test_background_is_the_object_of_the_inverted_volume(dev):
    v = FIXTURES["noise_030"]
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    a = pipeline.chord_lengths(upload(v, dev), d, mm_y, mm_x, "background")
    b = pipeline.chord_lengths(upload(~v, dev), d, mm_y, mm_x, "object")
    for x, y in ((a.counts, b.counts), (a.border, b.border), (a.sum_q, b.sum_q), (a.total_length_mm, b.total_length_mm)):
        same_bytes(x, y, "inverted")
    again = pipeline.chord_lengths(upload(v, dev), d, mm_y, mm_x, "background")          # the same bytes on every run
    for x, y in ((a.counts, again.counts), (a.border, again.border), (a.sum_q, again.sum_q)):
        same_bytes(x, y, "second run")


def test_a_diagonal_of_600_voxels(dev):
    """Only the line (t, t, t), t < 600, of a (600, 600, 640) stack is set: one chord of (1, 1, 1) past every bin a workgroup
    keeps, 600 chords of one voxel in every other direction.  The reference walks the points alone."""
    shape, n = (600, 600, 640), 600
    words = np.zeros((shape[0], shape[1], 10), dtype=np.uint64)
    t = np.arange(n)
    words[t, t, t >> 6] = np.uint64(1) << (t & 63).astype(np.uint64)
    vol = pipeline.BitVolume(torch.from_numpy(words.view(np.int64)).to(dev), shape)
    d = np.resize(np.array([0.5, 0.5, 1.0, 0.25, 2.0, 0.3, 0.75]), n).copy()
    q = R.steps_q(R.steps(d, n, 0.45, 0.7))
    exp = R.walk_points([(i, i, i) for i in range(n)], shape, q)
    got = pipeline.chord_lengths(vol, d, 0.45, 0.7)
    for name, a, b in zip(("counts", "border", "sum_q"), (got.counts, got.border, got.sum_q), exp):
        assert a.shape == (13, 641) and np.array_equal(a, b), name
    m = R.FORWARD.index((1, 1, 1))
    assert got.counts[m, n] == 1 and got.border[m, n] == 1 and got.sum_q[m, n] == int(q[:, m].sum()) and got.voxels == n
    assert (got.counts[:m, 1] == n).all() and (got.border[:m, 1] >= 1).all()              # (0, 0, 0) lies on three faces


def test_scale(dev):
    """More lines in the slice plane (535 600) than lanes resident on the card (524 288), 17 words a row."""
    shape = (6, 520, 1030)
    FIXTURES["scale"] = R.noise(0.3, shape, seed=41)
    try:
        check_case("scale", dev, kinds=("odd",))
    finally:
        del FIXTURES["scale"]
        for key in [k for k in _ref if k[0] == "scale"]:
            del _ref[key]


# ------------------------------------------------------------------ the report
def test_chord_report(dev):
    v = FIXTURES["noise_030"]
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    c0 = pipeline.COUNTERS[KEY]
    got = volume_calculator.chord_report(v, d, mm_y, mm_x)
    assert pipeline.COUNTERS[KEY] == c0 + 2
    assert list(got) == ["directions", "object", "background"] and got["directions"] == list(R.FORWARD)
    vol = upload(v, dev)
    for phase in PHASES:
        c = pipeline.chord_lengths(vol, d, mm_y, mm_x, phase)
        same(c, v if phase == "object" else ~v, reference("noise_030", "odd", phase), "odd", ("report", phase))
        r = got[phase]
        assert list(r) == ["voxels", "chords", "mil_mm", "mean_chord_mm", "fabric", "lineal_path", "quantiles_mm"]
        assert r["voxels"] == c.voxels and r["chords"] == c.chords.tolist() and r["mil_mm"] == c.mean_chord_mm.tolist()
        assert type(r["mean_chord_mm"]) is float and r["mean_chord_mm"] == float(np.sum(c.total_length_mm) / int(c.chords.sum()))
        f = c.fabric()
        assert list(r["fabric"]) == ["tensor", "principal_mil_mm", "axes", "degree_of_anisotropy"]
        assert r["fabric"]["tensor"] == f["tensor"].tolist() and r["fabric"]["principal_mil_mm"] == f["principal_mil_mm"].tolist()
        assert r["fabric"]["axes"] == f["axes"].tolist() and r["fabric"]["degree_of_anisotropy"] == f["degree_of_anisotropy"]
        assert 0.0 <= f["degree_of_anisotropy"] < 1.0 and (np.diff(f["principal_mil_mm"]) <= 0).all()
        same_bytes(r["lineal_path"], c.lineal_path(), phase)
        assert r["quantiles_mm"]["fractions"] == (0.1, 0.5, 0.9)
        same_bytes(r["quantiles_mm"]["values"], c.quantiles_mm((0.1, 0.5, 0.9)), phase)
        assert (np.diff(r["quantiles_mm"]["values"], axis=1) >= 0).all()
    only = volume_calculator.chord_report(v, d, mm_y, mm_x, background=False)
    assert list(only) == ["directions", "object", "background"] and only["background"] is None
    assert only["object"]["chords"] == got["object"]["chords"]
    nothing = volume_calculator.chord_report(FIXTURES["empty"], np.ones(5), 1.0, 1.0)
    assert nothing["object"]["fabric"] is None and np.isnan(nothing["object"]["mean_chord_mm"]) and nothing["object"]["voxels"] == 0
    assert nothing["background"]["voxels"] == FIXTURES["empty"].size
    _devcache.clear()
    _memo.clear()


# ------------------------------------------------------------------ arguments
def test_argument_errors(dev):
    v = FIXTURES["noise_010"]
    vol = upload(v, dev)
    c0 = pipeline.COUNTERS[KEY]
    for phase in ("pores", "", None, 0):
        with pytest.raises(ValueError):
            pipeline.chord_lengths(vol, phase=phase)
    for bad in ((np.ones(3), 1.0, 1.0), (np.zeros(v.shape[0]), 1.0, 1.0), (None, 0.0, 1.0), (None, 1.0, float("nan"))):
        with pytest.raises(ValueError):
            pipeline.chord_lengths(vol, *bad)
        with pytest.raises(ValueError):
            volume_calculator.chord_report(v, np.ones(v.shape[0]) if bad[0] is None else bad[0], bad[1], bad[2])
    with pytest.raises(TypeError):
        volume_calculator.chord_report(v.astype(np.uint8), np.ones(v.shape[0]), 1.0, 1.0)
    assert pipeline.COUNTERS[KEY] == c0, "a refused call reached the kernel"
    L, st = _lib.lib(), _stream()
    nz, ny, nx = v.shape
    lmax = max(v.shape)
    tab = torch.from_numpy(pipeline.chord_steps_q(pipeline.chord_steps(None, nz))).to(dev)
    out = torch.full((3, 13 * (lmax + 1)), 77, dtype=torch.int64, device=dev)
    args = [_p(vol.bits), nz, ny, nx, _p(tab), lmax, _p(out[0]), _p(out[1]), _p(out[2]), st]
    for hole in (0, 4, 6, 7, 8):
        assert L.tomo_chord_hist(*[None if i == hole else a for i, a in enumerate(args)]) == -1
    for i, value in ((1, 0), (2, -3), (3, 0), (5, lmax - 1), (5, 0)):
        assert L.tomo_chord_hist(*[value if j == i else a for j, a in enumerate(args)]) == -1
    torch.cuda.synchronize()
    assert out.eq(77).all(), "a refused call wrote to the tables"
    _lib.check(L.tomo_chord_hist(*args), "tomo_chord_hist")      # ... and the tables are zeroed by the call itself
    got = out.cpu().numpy().reshape(3, 13, lmax + 1)
    for a, b in zip(got, reference("noise_010", "unit", "object")):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_fenced(dev, poison):
    """Noise, the wrap shapes and the long chords inside fenced, poisoned buffers: the same integers, clean fences."""
    names = ["noise_030", "noise_090", "long_x", "slots_x"] + [n for n in FIXTURES if n.startswith("wrap_")]
    vols = {name: upload(FIXTURES[name], dev) for name in names}

    def once(p):
        with F.fenced(p, F.package_modules(), seed=7) as fz:
            for name in names:
                v, vol = FIXTURES[name], vols[name]
                d, mm_y, mm_x = spacing("odd", v.shape[0])
                with fz.unchanged(vol.bits):
                    for phase in PHASES:
                        got = pipeline.chord_lengths(vol, d, mm_y, mm_x, phase)
                        same(got, v if phase == "object" else ~v, reference(name, "odd", phase), "odd", ("fenced", name, phase))
            fz.check()
            assert fz.ran("chord_lengths") >= 3 * len(names)     # the tables twice, the complement once
    try:
        once(poison)
    except AssertionError as e:
        try:
            once("zero")
            control = "the zero control PASSES: the failure is a read of memory nobody wrote"
        except AssertionError as z:
            control = "the zero control fails too (%s): not a matter of the poison" % (str(z).splitlines() or [""])[0][:200]
        raise AssertionError("%s\n[%s] %s" % (e, poison, control)) from e
