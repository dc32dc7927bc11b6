"""CPU tier of the chord lengths: tests/chords_reference.py against a walk over every voxel and direction and against hand
values, then the pure NumPy half of pipeline.chord_lengths (chord_lengths_from_tables and the methods of ChordLengths) on the
reference's integers: the invariant, the lineal path, the fabric tensor of a ball and of an ellipsoid, the fixed-point bound.
Nothing here needs a GPU; the argument checks of tomo_chord_hist return before anything is launched."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chords_reference as R  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

ODD = np.array([0.5, 0.5, 1.0, 0.25, 2.0, 0.3, 0.75])


def spacing(kind, nz):
    """The three spacings of tests/test_gpu_breadth.py -> (slice_depths, mm_y, mm_x)."""
    if kind == "unit":
        return None, 1.0, 1.0
    if kind == "dyadic":
        return np.full(nz, 2.0), 1.0, 0.5
    return np.resize(ODD, nz).copy(), 0.45, 0.7


def lengths(v, kind="unit"):
    """The ChordLengths of the package's host functions on the reference's tables."""
    nz = v.shape[0]
    d, mm_y, mm_x = spacing(kind, nz)
    steps = pipeline.chord_steps(d, nz, mm_y, mm_x)
    d_mean = 1.0 if d is None else float(np.mean(d))
    return pipeline.chord_lengths_from_tables(R.tables(v, pipeline.chord_steps_q(steps)), v.sum(axis=(1, 2)), steps, v.shape,
                                              (d_mean, mm_y, mm_x))


# ------------------------------------------------------------------ the reference against the walk
def test_directions_and_steps():
    assert pipeline.chord_directions().dtype == np.int64 and pipeline.chord_directions().tolist() == [list(s) for s in R.FORWARD]
    assert np.array_equal(pipeline.chord_directions(), pipeline.breadth_normals())
    assert len(R.FORWARD) == 13 and R.FORWARD[0] == (0, 0, 1) and R.FORWARD[12] == (1, 1, 1) and list(R.FORWARD) == sorted(R.FORWARD)
    for kind in ("unit", "dyadic", "odd"):
        d, mm_y, mm_x = spacing(kind, 9)
        got = pipeline.chord_steps(d, 9, mm_y, mm_x)
        assert got.dtype == np.float64 and got.shape == (9, 13) and got.tobytes() == R.steps(d, 9, mm_y, mm_x).tobytes()
        q = pipeline.chord_steps_q(got)
        assert q.dtype == np.int64 and np.array_equal(q, R.steps_q(got))
    assert pipeline.chord_steps(None, 2)[0].tolist() == [np.sqrt(float(sum(abs(a) for a in s))) for s in R.FORWARD]
    assert pipeline.chord_steps_q(np.array([[0.5 / 65536, 1.5 / 65536, 2.5 / 65536]])).tolist() == [[0, 2, 2]]     # half to even
    for bad in (([1.0, 2.0], 3, 1.0, 1.0), ([1.0, -1.0], 2, 1.0, 1.0), (None, 0, 1.0, 1.0), (None, 2, 0.0, 1.0), (None, 2, 1.0, float("inf"))):
        with pytest.raises(ValueError):
            pipeline.chord_steps(*bad)


@pytest.mark.parametrize("shape,density", [((4, 5, 6), 1.0), ((7, 3, 5), 0.5), ((3, 7, 2), 0.6), ((1, 1, 1), 1.0), ((5, 4, 6), 0.85)])
def test_reference_equals_the_walk(shape, density):
    v = np.ones(shape, dtype=bool) if density == 1.0 else R.noise(density, shape, seed=shape[0])
    for kind in ("unit", "odd"):
        d, mm_y, mm_x = spacing(kind, shape[0])
        q = R.steps_q(R.steps(d, shape[0], mm_y, mm_x))
        got, exp = R.tables(v, q), R.walk(v, q)
        for name, a, b in zip(("counts", "border", "sum_q"), got, exp):
            assert a.dtype == np.int64 and a.shape == (13, max(shape) + 1) and np.array_equal(a, b), (name, kind)
        assert not got[0][:, 0].any() and not got[1][:, 0].any() and not got[2][:, 0].any()
        assert (got[1] <= got[0]).all()


def test_hand_values():
    q = R.steps_q(R.steps(None, 4))
    counts, border, sum_q = R.tables(np.ones((4, 5, 6), dtype=bool), q)
    m = R.FORWARD.index((1, 1, 1))
    assert counts[m].tolist() == [0, 24, 18, 12, 6, 0, 0] and border[m].tolist() == counts[m].tolist()
    assert sum_q[m].tolist() == [n * c * int(q[0, m]) for n, c in enumerate(counts[m])]
    assert counts[R.FORWARD.index((0, 0, 1))].tolist() == [0, 0, 0, 0, 0, 0, 20]
    assert counts[R.FORWARD.index((1, 0, 0))].tolist() == [0, 0, 0, 0, 30, 0, 0]
    assert np.array_equal(counts, border)                        # a full box: every chord runs from face to face
    one = R.tables(np.ones((1, 1, 1), dtype=bool), R.steps_q(R.steps([0.3], 1, 0.45, 0.7)))
    assert one[0].tolist() == [[0, 1]] * 13 and one[1].tolist() == [[0, 1]] * 13
    assert one[2][:, 1].tolist() == R.steps_q(R.steps([0.3], 1, 0.45, 0.7))[0].tolist()
    v = np.zeros((3, 3, 9), dtype=bool)
    v[1, 1, 2:7] = True                                          # a bar of five voxels inside: one chord along x, five across
    counts, border, _ = R.tables(v, R.steps_q(R.steps(None, 3)))
    assert counts[0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0] and not border.any()
    assert all(counts[m].tolist() == [0, 5] + [0] * 8 for m in range(1, 13))
    # the walk over points alone, for a line too long to build the volume of
    pts = [(t, t, t) for t in range(7)]
    line = np.zeros((7, 8, 9), dtype=bool)
    for p in pts:
        line[p] = True
    q = R.steps_q(R.steps(None, 7))
    for a, b in zip(R.walk_points(pts, line.shape, q), R.tables(line, q)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ the pure functions
@pytest.mark.parametrize("kind", ["unit", "dyadic", "odd"])
def test_invariant_and_lineal_path(kind):
    v = R.noise(0.6, (7, 9, 11), seed=3)
    c = lengths(v, kind)
    n = np.arange(c.counts.shape[1])
    assert c.voxels == int(v.sum()) and ((c.counts * n).sum(axis=1) == v.sum()).all()                # the invariant
    assert np.array_equal(c.chords, c.counts.sum(axis=1)) and c.directions.tolist() == [list(s) for s in R.FORWARD]
    lp = c.lineal_path()
    assert lp.dtype == np.float64 and lp.shape == c.counts.shape and not lp[:, 0].any()
    assert (lp[:, 1] == v.sum() / v.size).all()                  # L(1) is the volume fraction
    assert (lp >= 0).all() and (lp <= 1).all()
    inner = c.lineal_path(interior=True)
    assert (inner <= lp).all() and (inner[:, 1] < lp[:, 1]).all()
    P = c.segments()
    for m, s in enumerate(R.FORWARD):                            # ... against a count of the segments themselves
        for r in (1, 2, 3, 7, 8, 11):
            total = hit = 0
            for z in range(7):
                for y in range(9):
                    for x in range(11):
                        e = (z + (r - 1) * s[0], y + (r - 1) * s[1], x + (r - 1) * s[2])
                        if 0 <= e[0] < 7 and 0 <= e[1] < 9 and 0 <= e[2] < 11:
                            total += 1
                            hit += all(v[z + t * s[0], y + t * s[1], x + t * s[2]] for t in range(r))
            assert P[m, r] == total and lp[m, r] == (hit / total if total else 0.0), (s, r)
    # total_length_mm comes from the slice counts, sum_q from the chords: one checks the other
    assert np.abs(c.sum_q.sum(axis=1) / 65536.0 - c.total_length_mm).max() <= v.sum() * 2.0 ** -17
    assert np.array_equal(c.mean_chord_mm, c.total_length_mm / c.chords)
    mean = c.mean_length_mm()
    assert np.isnan(mean[c.counts == 0]).all() and (mean[c.counts > 0] > 0).all()
    if kind != "odd":                                            # constant depth: the mean length of a bin is n fixed-point steps
        step = pipeline.chord_steps_q(c.steps)[0] / 65536.0
        assert np.array_equal(mean[c.counts > 0], (n[None, :] * step[:, None])[c.counts > 0])


def test_lineal_path_of_a_full_box_is_one():
    c = lengths(np.ones((4, 5, 6), dtype=bool), "odd")
    lp, P = c.lineal_path(), c.segments()
    assert (lp[P > 0] == 1.0).all() and not lp[P == 0].any() and (P[:, 1] == 120).all()
    assert P[12].tolist() == [0, 120, 60, 24, 6, 0, 0] and P[0].tolist() == [0, 120, 100, 80, 60, 40, 20]
    assert not c.lineal_path(interior=True).any()                # every chord of a full box is cut by the stack
    empty = lengths(np.zeros((4, 5, 6), dtype=bool))
    assert empty.voxels == 0 and not empty.chords.any() and np.isnan(empty.mean_chord_mm).all() and not empty.lineal_path().any()
    with pytest.raises(ValueError):
        empty.fabric()
    with pytest.raises(ValueError):                              # no chord that the stack does not cut
        lengths(np.ones((1, 1, 1), dtype=bool)).fabric(interior=True)


def test_fabric_of_a_ball():
    """R = 16 in 37^3: by symmetry the 13 MILs fall into three classes, the fit is a sphere; 0.995 .. 1.006 of 4 R / 3."""
    c = lengths(R.ellipsoid((37, 37, 37), (16, 16, 16)))
    f = c.fabric()
    assert list(f) == ["tensor", "principal_mil_mm", "axes", "degree_of_anisotropy", "directions_used"] and f["directions_used"] == 13
    assert abs(f["degree_of_anisotropy"]) < 1e-12
    ratio = c.mean_chord_mm / (4.0 * 16.0 / 3.0)
    assert 0.995 <= ratio.min() and ratio.max() <= 1.0063
    assert np.abs(f["principal_mil_mm"] / (64.0 / 3.0) - 1.002428405350478).max() < 1e-9
    assert np.abs(f["axes"] @ f["axes"].T - np.eye(3)).max() < 1e-12
    assert not c.border.any() and abs(c.fabric(interior=True)["degree_of_anisotropy"]) < 1e-12


# semi-axes (10, 16, 28) voxels in (27, 39, 63): measured with tests/chords_reference.py, deterministic float64 from integers.
# Per spacing: principal MIL over 4 / 3 of the continuum semi-axes in mm (descending), degree of anisotropy, continuum value.
ELLIPSOID = {
    "unit": ([1.00598876555794, 1.004954426797634, 0.9989044969272279], 0.8742391070462915, 0.8724489795918368),
    "dyadic": ([0.9987926725413292, 1.0024897159969897, 1.0129643651673355], 0.49599630515718707, 0.51),
    "odd": ([1.0703523903471885, 1.0367311841574014, 1.0124377033735927], 0.8792642446273985, 0.8650562265722616),
}


@pytest.mark.parametrize("kind", list(ELLIPSOID))
def test_fabric_of_an_ellipsoid(kind):
    v = R.ellipsoid((27, 39, 63), (10, 16, 28))
    c = lengths(v, kind)
    f = c.fabric()
    d, mm_y, mm_x = spacing(kind, 27)
    d_mean = 1.0 if d is None else float(np.mean(d))
    semi = np.array([10 * d_mean, 16 * mm_y, 28 * mm_x])
    order = np.argsort(-semi)
    ratios, da, da_continuum = ELLIPSOID[kind]
    assert np.abs(f["principal_mil_mm"] / (semi[order] * 4.0 / 3.0) - np.array(ratios)).max() < 1e-9
    assert abs(f["degree_of_anisotropy"] - da) < 1e-9 and abs(1.0 - (semi.min() / semi.max()) ** 2 - da_continuum) < 1e-12
    assert np.abs(np.abs(f["axes"]) - np.eye(3)[order]).max() < 1e-9 and (f["axes"][np.arange(3), order] > 0).all()
    assert np.abs(f["tensor"] - f["tensor"].T).max() == 0.0
    if kind == "unit":                                           # the values of the README
        assert np.abs(f["principal_mil_mm"] * 0.75 - [28.167685435622325, 16.07927082876214, 9.98904496927228]).max() < 1e-9
        assert round(f["degree_of_anisotropy"], 3) == 0.874
    assert not c.border.any()                                    # the body lies inside the stack: nothing is cut


def test_fabric_needs_six_directions():
    v = np.zeros((3, 3, 9), dtype=bool)
    v[1, 1, 2:7] = True
    c = lengths(v)
    c.mean_chord_mm[5:] = np.nan                                 # five directions left
    with pytest.raises(ValueError):
        c.fabric()


def test_quantiles():
    v = np.zeros((1, 4, 12), dtype=bool)
    v[0, 0, 0:1] = v[0, 1, 0:2] = v[0, 2, 0:3] = v[0, 3, 0:10] = True      # x chords of 1, 2, 3 and 10 voxels
    c = lengths(v, "dyadic")
    qs = c.quantiles_mm((0.1, 0.25, 0.5, 0.75, 0.9, 1.0))
    assert qs.shape == (13, 6) and qs[0].tolist() == [0.5, 0.5, 1.0, 1.5, 5.0, 5.0]
    assert np.isnan(lengths(np.zeros((2, 2, 2), dtype=bool)).quantiles_mm()).all()


@pytest.mark.parametrize("kind", ["dyadic", "odd"])
def test_sum_q_is_within_half_a_unit_per_voxel(kind):
    """|sum_q / 65536 - exact| <= n * 2^-17 per chord (every step is rounded once, by at most half a unit of 2^-16), so per bin
    at most counts * n * 2^-17: in exact rational arithmetic on the float64 steps."""
    v = R.noise(0.7, (7, 5, 6), seed=11)
    d, mm_y, mm_x = spacing(kind, 7)
    steps = pipeline.chord_steps(d, 7, mm_y, mm_x)
    q = pipeline.chord_steps_q(steps)
    counts, _, sum_q = R.tables(v, q)
    pts = [tuple(p) for p in np.argwhere(v)]
    c2, _, exact = R.walk_points(pts, v.shape, [[Fraction(float(x)) for x in row] for row in steps])
    assert np.array_equal(counts, c2)
    worst = Fraction(0)
    for m in range(13):
        for n in range(1, counts.shape[1]):
            err = abs(Fraction(int(sum_q[m, n]), 65536) - exact[m, n])
            assert err <= Fraction(int(counts[m, n]) * n, 2 ** 17), (m, n)
            worst = max(worst, err)
    assert worst > 0                                             # the diagonal steps are irrational: something was rounded


# ------------------------------------------------------------------ the entry point and the report without a GPU
def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    a = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(a)
    assert L.tomo_chord_hist(None, 2, 2, 2, p, 2, p, p, p, None) == -1
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert L.tomo_chord_hist(p, 2, 2, 2, args[0], 2, args[1], args[2], args[3], None) == -1
    for nz, ny, nx in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert L.tomo_chord_hist(p, nz, ny, nx, p, 8, p, p, p, None) == -1
    for nz, ny, nx in ((3, 2, 2), (2, 3, 2), (2, 2, 3)):         # lmax below the longest side
        assert L.tomo_chord_hist(p, nz, ny, nx, p, 2, p, p, p, None) == -1
    assert L.tomo_chord_hist(p, 1 << 20, 1 << 11, 64, p, 1 << 20, p, p, p, None) == -3
    assert "chord_lengths" in pipeline.COUNTERS and pipeline.CHORD_LDS_BINS == 256
    text = open(os.path.join(_lib.CSRC, "chords.hip")).read()
    assert "#define CHORD_BINS %d" % pipeline.CHORD_LDS_BINS in text


def test_report_and_phase_arguments():
    with pytest.raises(TypeError):
        volume_calculator.chord_report(np.zeros((2, 2, 2), dtype=np.uint8), [1.0, 1.0], 1.0, 1.0)
    with pytest.raises(ValueError):
        volume_calculator.chord_report(np.zeros((2, 2, 2), dtype=bool), [1.0], 1.0, 1.0)
    with pytest.raises(ValueError):
        pipeline.chord_lengths(pipeline.BitVolume(None, (2, 2, 2)), phase="pores")
