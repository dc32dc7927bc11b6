"""GPU tier: mean breadth per component by the discretised Crofton formula on the resident bit volume
(csrc/component_measures.hip: tomo_cc_breadth_hist, tomo_cc_breadth -> pipeline.mean_breadth / component_breadth /
cavity_breadth -> volume_calculator.mean_breadth / component_properties(..., breadth=True) / minkowski_functionals).

Every result is compared with tests/breadth_reference.py -- shifted ANDs in NumPy on SciPy's labelling, held to a walk over the
lattice planes, to SciPy's 2-D labelling and to hand values by tests/test_breadth_cpu.py -- never with a second run of the code
under test.  section_euler is compared with ==; mean_breadth_mm is bit for bit the sequential float64 sum of the reference's
integers times pipeline.breadth_factors, and within 1e-11 of the scale of the sum with the reference's own factors (SciPy's
Voronoi cells: the two weight computations agree to 1e-14)."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breadth_reference as R  # noqa: E402
import component_props_reference as P  # noqa: E402
import components_reference as C  # noqa: E402
import fenced as F  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
KEY = "components_breadth"
SHAPE = (19, 21, 150)                                            # x crosses 63|64 and 127|128 and has a 22-bit tail


def spacing(kind, nz):
    """-> (slice_depths, mm_y, mm_x): unit, dyadic (2, 1, 0.5), odd with varying depths (an FMA would show)."""
    if kind == "unit":
        return None, 1.0, 1.0
    if kind == "dyadic":
        return np.full(nz, 2.0), 1.0, 0.5
    return np.resize(np.array([0.5, 0.5, 1.0, 0.25, 2.0, 0.3, 0.75]), nz).copy(), 0.45, 0.7


SPACINGS = ("unit", "dyadic", "odd")


def _set(shape, *at):
    v = np.zeros(shape, dtype=bool)
    for p in at:
        v[p] = True
    return v


def add(p, o):
    return tuple(int(a + b) for a, b in zip(p, o))


def pair_at_the_seams(step):
    """Two voxels one forward step apart in a (2, 3, 66) stack: across x = 63|64 where the step has an x part, into the last row
    where it goes up in y, into the top slice where it goes up in z."""
    p = (0, 1, 64 if step[2] < 0 else 63)
    return _set((2, 3, 66), p, add(p, step))


def fixtures():
    out = {}
    for d in (10, 30, 50, 90):
        out["noise_%03d" % d] = T.noise(d / 100.0, SHAPE, seed=d)
    out["sponge"] = T.sponge()
    out["full"] = np.ones((5, 7, 150), dtype=bool)
    out["empty"] = np.zeros((5, 7, 150), dtype=bool)
    nz, ny, nx = 3, 4, 150
    out["corners"] = _set((nz, ny, nx), *[(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)])
    out["one_voxel"] = np.ones((1, 1, 1), dtype=bool)
    for step in R.FORWARD:
        out["pair_%d_%d_%d" % step] = pair_at_the_seams(step)
    out["triangle"] = _set((2, 3, 66), (0, 1, 64), (0, 2, 63), (1, 1, 63))       # a face of (1, 1, 1) across the seam
    out["corner_pair"] = T.corner_pair()                         # diagonal contacts: two components under 6, one under 26
    out["diamond"] = T.diamond()
    out["edge_pair_z"] = _set((2, 1, 66), (0, 0, 63), (1, 0, 64))
    out["straddle"] = T.straddle()                               # ny = 5: a wave's rows lie in 13 slices
    return out


FIXTURES = fixtures()
CASES = [(name, conn) for name in FIXTURES for conn in C.CONNECTIVITIES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def upload(v, dev):
    return pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


def resident(name, dev):
    """The BitVolume of a case, uploaded as bits: the kernels under test are the only ones that run."""
    return FIXTURES[name], upload(FIXTURES[name], dev)


_ref = {}


def reference(name, conn):
    """(n, sizes, chi int64 (n, nz, 26)) of the helper, computed once per case and left unchanged."""
    if (name, conn) not in _ref:
        v = FIXTURES[name]
        labels, n = T.label(v, conn)
        per = R.chi(labels, n)
        assert np.array_equal(per.sum(axis=0), R.chi_whole(v))   # the components add up to the unlabelled volume
        per.setflags(write=False)
        _ref[(name, conn)] = (n, C.sizes(labels, n), per)
    return _ref[(name, conn)]


def sums(per, B, directions):
    """R.breadth of every row at once: the same float64 operations in the same order, a vector of components wide
    -> (the sums, the sums of the absolute terms: the scale of the rounding)."""
    per = np.asarray(per).reshape(-1, per.shape[-2], 26)
    s, scale = np.zeros(len(per)), np.zeros(len(per))
    for k in range(per.shape[1]):
        for col in range(26):
            if directions == 13 or col % 13 in R.AXES:
                term = per[:, k, col].astype(np.float64) * float(B[k, col])
                s = s + term
                scale = scale + np.abs(term)
    return s, scale


def same_breadth(got, per, d, mm_y, mm_x, directions, what):
    """Breadths of the device against the reference's integers per (rows, nz, 26)."""
    nz = per.shape[-2]
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    exact, scale = sums(per, pipeline.breadth_factors(d, nz, mm_y, mm_x, directions), directions)
    free, _ = sums(per, R.factors(d, nz, mm_y, mm_x, directions), directions)
    assert got.tobytes() == exact.tobytes(), (what, got[:4], exact[:4])
    assert (np.abs(got - free) <= 1e-11 * scale).all(), (what, got[:4], free[:4])


def same(got, pick, sizes, per, d, mm_y, mm_x, directions, what):
    """A ComponentBreadth against the helper's rows for the labels `pick` (1-based, ascending)."""
    pick = np.asarray(pick, dtype=np.int64)
    assert got.labels.dtype == np.int64 and np.array_equal(got.labels, pick), (what, got.labels[:8], pick[:8])
    assert got.voxels.dtype == np.int64 and np.array_equal(got.voxels, sizes[pick - 1]), what
    exp = R.section_euler(per[pick - 1]).reshape(-1, 13)
    assert got.section_euler.dtype == np.int64 and got.section_euler.shape == exp.shape, (what, got.section_euler.shape)
    assert np.array_equal(got.section_euler, exp), (what, got.section_euler[:4].tolist(), exp[:4].tolist())
    assert got.mean_breadth_mm.dtype == np.float64 and got.mean_breadth_mm.shape == (len(pick),)
    same_breadth(got.mean_breadth_mm, per[pick - 1], d, mm_y, mm_x, directions, what)


@pytest.mark.parametrize("name,conn", CASES)
def test_rows_and_breadth_equal_the_reference(dev, name, conn):
    """Every fixture under both connectivities, the three spacings and both direction sets: the rows of all components, and
    the unlabelled call, which equals their sum."""
    v, vol = resident(name, dev)
    n, sizes, per = reference(name, conn)
    whole_ref = R.chi_whole(v)
    before = vol.bits.clone()
    runs = pipeline.ComponentRuns(vol, conn)                     # one labelling serves every setting
    for kind in SPACINGS:
        d, mm_y, mm_x = spacing(kind, v.shape[0])
        for directions in (13, 3):
            what = (name, conn, kind, directions)
            got = runs.breadth(pipeline.breadth_factors(d, v.shape[0], mm_y, mm_x, directions), directions)
            same(got, np.arange(1, n + 1), sizes, per, d, mm_y, mm_x, directions, what)
            whole = pipeline.mean_breadth(vol, d, mm_y, mm_x, directions)
            assert whole.section_euler.dtype == np.int64 and whole.section_euler.shape == (13,)
            assert np.array_equal(whole.section_euler, R.section_euler(whole_ref))
            assert np.array_equal(got.section_euler.sum(axis=0), whole.section_euler)      # without tables: the sum of the rows
            assert isinstance(whole.mean_breadth_mm, float)
            same_breadth(whole.mean_breadth_mm, whole_ref[None], d, mm_y, mm_x, directions, what)
            if not v.any():
                assert whole.mean_breadth_mm == 0.0 and len(got) == 0
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    same(pipeline.component_breadth(vol, d, mm_y, mm_x, conn), np.arange(1, n + 1), sizes, per, d, mm_y, mm_x, 13, name)
    assert torch.equal(vol.bits, before), "the input volume was modified"


def test_the_hand_values(dev):
    _, vol = resident("one_voxel", dev)
    one = pipeline.mean_breadth(vol)
    assert abs(one.mean_breadth_mm - 0.75102007697) < 1e-10 and one.section_euler.tolist() == [1] * 13
    assert pipeline.mean_breadth(vol, directions=3).mean_breadth_mm == 1.0
    assert abs(pipeline.mean_breadth(vol, [2.0], 1.0, 0.5).mean_breadth_mm - 0.91061687050) < 1e-10
    box = np.zeros((7, 10, 70), dtype=bool)
    box[1:6, 1:9, 58:69] = True                                  # 5 x 8 x 11 voxels across x = 63|64
    got = pipeline.component_breadth(upload(box, dev))
    assert got.section_euler.tolist() == [[sum(abs(a) * (s - 1) for a, s in zip(m, (5, 8, 11))) + 1 for m in R.NORMALS]]
    assert abs(got.mean_breadth_mm[0] - 10.4805616018) < 1e-9
    assert abs(pipeline.mean_breadth(upload(box, dev), directions=3).mean_breadth_mm - 8.0) < 1e-12 * 8.0
    _, vol = resident("corner_pair", dev)
    f = R.NORMALS.index((1, -1, -1))
    assert [r[f] for r in pipeline.component_breadth(vol, connectivity=6).section_euler.tolist()] == [1, 1]
    assert pipeline.component_breadth(vol, connectivity=26).section_euler.tolist() == [[2] * 13]
    for directions in (0, 4, 26):
        with pytest.raises(ValueError):
            pipeline.mean_breadth(vol, directions=directions)
        with pytest.raises(ValueError):
            pipeline.component_breadth(vol, directions=directions)
        with pytest.raises(ValueError):
            pipeline.cavity_breadth(vol, directions=directions)
    with pytest.raises(ValueError):
        pipeline.component_breadth(vol, connectivity=18)


def test_an_empty_volume_gives_empty_arrays(dev):
    v, vol = resident("empty", dev)
    c0 = pipeline.COUNTERS[KEY]
    for got in (pipeline.component_breadth(vol, None, 0.45, 0.7, 26), pipeline.cavity_breadth(vol),
                pipeline.cavity_breadth(resident("full", dev)[1]), pipeline.component_breadth(resident("full", dev)[1], min_voxels=10 ** 6)):
        assert len(got) == 0 and got.labels.shape == (0,) and got.voxels.shape == (0,) and got.mean_breadth_mm.shape == (0,)
        assert got.section_euler.shape == (0, 13) and got.section_euler.dtype == np.int64 and got.mean_breadth_mm.dtype == np.float64
    assert pipeline.COUNTERS[KEY] == c0                          # nothing was launched beyond the labelling and the selection
    assert volume_calculator.component_properties(v, 0.7, 0.45, np.ones(v.shape[0]), breadth=True) == []
    _devcache.clear()


@pytest.mark.parametrize("name,conn", [("noise_030", 6), ("noise_010", 26), ("straddle", 26), ("sponge", 6)])
def test_selected_rows_are_those_of_component_properties(dev, name, conn):
    v, vol = resident(name, dev)
    n, sizes, per = reference(name, conn)
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    B = pipeline.breadth_factors(d, v.shape[0], mm_y, mm_x)
    for min_voxels, largest in [(0, False), (int(np.median(sizes)), False), (2, False), (int(sizes.max()) + 1, False), (0, True), (2, True)]:
        pick = P.selected(sizes, min_voxels, largest).astype(np.int64) + 1
        props = pipeline.component_properties(vol, d, mm_y, mm_x, conn, min_voxels, largest)
        got = pipeline.component_breadth(vol, d, mm_y, mm_x, conn, min_voxels, largest)
        assert np.array_equal(got.labels, props.labels) and np.array_equal(got.voxels, props.voxels)
        same(got, pick, sizes, per, d, mm_y, mm_x, 13, (name, conn, min_voxels, largest))
    runs = pipeline.ComponentRuns(vol, conn)
    for lo, hi in ((0, 3), (2, int(np.median(sizes)) + 1), (2, 1)):
        pick = np.nonzero((sizes >= lo) & (sizes <= hi))[0].astype(np.int64) + 1
        same(runs.breadth(B, 13, lo, max_voxels=hi), pick, sizes, per, d, mm_y, mm_x, 13, (name, conn, lo, hi))


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_cavity_breadth_on_a_shell_with_two_pores(dev, conn):
    v = np.zeros((12, 13, 80), dtype=bool)
    v[1:11, 1:12, 50:78] = True
    v[3:6, 3:7, 60:68] = False                                   # a pore of 3 x 4 x 8 voxels across x = 63|64
    v[8, 9, 75] = False                                          # a pore of one voxel
    v[4:9, 6, 52] = False
    v[0:5, 6, 52] = False                                        # a channel that reaches the face z = 0: no cavity
    vol = upload(v, dev)
    labels, n = T.label(~v, 32 - conn)
    enclosed = [c for c in range(1, n + 1) if all(lo > 0 and hi < s - 1 for (lo, hi), s in
                                                  zip([(a.min(), a.max()) for a in np.nonzero(labels == c)], v.shape))]
    assert len(enclosed) == 2
    sizes = C.sizes(labels, n)
    per = R.chi(labels, n)
    for kind in SPACINGS:
        d, mm_y, mm_x = spacing(kind, v.shape[0])
        got = pipeline.cavity_breadth(vol, d, mm_y, mm_x, conn)
        same(got, enclosed, sizes, per, d, mm_y, mm_x, 13, ("pores", conn, kind))
        cav = pipeline.cavity_table(vol, d, mm_y, mm_x, conn)
        assert np.array_equal(cav.labels, got.labels) and np.array_equal(cav.voxels, got.voxels)
    assert sorted(got.voxels.tolist()) == [1, 96]
    big = int(np.argmax(got.voxels))
    assert got.section_euler[big].tolist() == [sum(abs(a) * (s - 1) for a, s in zip(m, (3, 4, 8))) + 1 for m in R.NORMALS]
    only = pipeline.cavity_breadth(vol, connectivity=conn, min_voxels=2, directions=3)
    assert only.voxels.tolist() == [96] and abs(only.mean_breadth_mm[0] - 5.0) < 1e-12 * 5.0
    assert len(pipeline.cavity_breadth(vol, connectivity=conn, min_voxels=2, max_voxels=95)) == 0


def test_volume_calculator_dicts(dev):
    name, conn = "noise_010", 6
    v = FIXTURES[name]
    n, sizes, per = reference(name, conn)
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    c0 = pipeline.COUNTERS[KEY]
    plain = volume_calculator.component_properties(v, mm_x, mm_y, d, conn)
    assert volume_calculator.component_properties(v, mm_x, mm_y, d, conn, breadth=False) == plain
    assert pipeline.COUNTERS[KEY] == c0, "breadth=False launched the breadth kernels"
    assert all(not {"mean_breadth_mm", "mean_curvature_integral_mm"} & set(g) for g in plain)
    assert list(plain[0]) == ["label", "voxels", "voxel_volume_mm3", "bounding_box", "dimensions", "centroid_mm", "centroid_index"]
    got = volume_calculator.component_properties(v, mm_x, mm_y, d, conn, breadth=True)
    assert pipeline.COUNTERS[KEY] == c0 + 1
    assert [g["label"] for g in got] == list(range(1, n + 1))
    for g, p in zip(got, plain):
        assert list(g) == list(p) + ["mean_breadth_mm", "mean_curvature_integral_mm"] and all(g[k] == p[k] for k in p)
        assert type(g["mean_breadth_mm"]) is float and type(g["mean_curvature_integral_mm"]) is float
        assert g["mean_curvature_integral_mm"] == 2.0 * math.pi * g["mean_breadth_mm"]
    same_breadth([g["mean_breadth_mm"] for g in got], per, d, mm_y, mm_x, 13, "dicts")
    flags = volume_calculator.component_properties(v, mm_x, mm_y, d, 26, 2, True, topology=True, surface=True, skeleton=True, caliper=True)
    three = volume_calculator.component_properties(v, mm_x, mm_y, d, 26, 2, True, topology=True, surface=True, skeleton=True, breadth=True,
                                                   breadth_directions=3, caliper=True)
    n26, sizes26, per26 = reference(name, 26)
    pick = P.selected(sizes26, 2, True)
    assert [g["label"] for g in three] == (pick + 1).tolist() and len(flags) == len(three)
    for g, p in zip(three, flags):                               # the new keys come last; the others keep their places
        assert list(g) == list(p) + ["mean_breadth_mm", "mean_curvature_integral_mm"] and all(g[k] == p[k] for k in p)
    same_breadth([g["mean_breadth_mm"] for g in three], per26[pick], d, mm_y, mm_x, 3, "dicts, three directions")
    whole = volume_calculator.mean_breadth(v, mm_x, mm_y, d)
    assert type(whole) is float
    same_breadth(whole, R.chi_whole(v)[None], d, mm_y, mm_x, 13, "whole")
    _devcache.clear()
    _memo.clear()


def test_minkowski_functionals_are_the_four_separate_calls(dev):
    v = np.zeros((14, 15, 80), dtype=bool)
    z, y, x = np.indices(v.shape)
    v |= (z - 6) ** 2 + (y - 7) ** 2 + (x - 62) ** 2 <= 36        # a ball across x = 63|64
    v[6, 7, 62] = False                                          # ... with a cavity
    v[2:5, 2:5, 3:9] = True                                      # a box
    d, mm_y, mm_x = spacing("odd", v.shape[0])
    for conn, directions in ((26, 13), (6, 3)):
        got = volume_calculator.minkowski_functionals(v, mm_x, mm_y, d, conn, directions)
        assert list(got) == ["volume_mm3", "surface_area_mm2", "mean_breadth_mm", "mean_curvature_integral_mm", "euler_number",
                             "volume_fraction", "surface_density_per_mm", "mean_curvature_density_per_mm2", "euler_density_per_mm3",
                             "components"]
        vol = volume_calculator.to_device_volume(v)
        assert got["volume_mm3"] == volume_calculator.VolumeCalculator().calculate_voxel_volume_variable_depth(v, mm_x, mm_y, d)
        assert got["surface_area_mm2"] == pipeline.surface_area(vol, d, mm_y, mm_x, directions).surface_area_mm2
        assert got["mean_breadth_mm"] == pipeline.mean_breadth(vol, d, mm_y, mm_x, directions).mean_breadth_mm
        assert got["mean_breadth_mm"] == volume_calculator.mean_breadth(v, mm_x, mm_y, d, directions)
        same_breadth(got["mean_breadth_mm"], R.chi_whole(v)[None], d, mm_y, mm_x, directions, "report")
        assert got["mean_curvature_integral_mm"] == 2.0 * math.pi * got["mean_breadth_mm"]
        assert got["euler_number"] == pipeline.euler_number(vol, conn) == T.euler(v, conn) == 3 and type(got["euler_number"]) is int
        stack = 80 * mm_x * (15 * mm_y) * float(np.sum(d))
        assert abs(got["volume_fraction"] * stack - got["volume_mm3"]) <= 1e-12 * got["volume_mm3"]
        assert abs(got["surface_density_per_mm"] * stack - got["surface_area_mm2"]) <= 1e-12 * got["surface_area_mm2"]
        assert abs(got["mean_curvature_density_per_mm2"] * stack - got["mean_curvature_integral_mm"]) <= 1e-12 * got["mean_curvature_integral_mm"]
        assert abs(got["euler_density_per_mm3"] * stack - 3) <= 1e-12
        assert got["components"] == volume_calculator.component_properties(v, mm_x, mm_y, d, conn, topology=True, surface=True,
                                                                           surface_directions=directions, breadth=True,
                                                                           breadth_directions=directions)
        assert len(got["components"]) == 2 and sum(g["euler_number"] for g in got["components"]) == 3
    _devcache.clear()
    _memo.clear()


def test_the_guards_flag_instead_of_writing_outside_a_table(dev, monkeypatch):
    """A histogram shorter than tot[4]: bit 1 of the flags, the counters stay zero and nothing behind them is touched; the
    finishing kernel then writes no row.  The budget error names min_voxels."""
    L, st = _lib.lib(), _stream()
    W = pipeline.BREADTH_WORDS
    v, vol = resident("noise_030", dev)
    nz = v.shape[0]
    cr = pipeline.ComponentRuns(vol, 6)
    picked = cr.select(0, False)
    n, total, m = picked.table.shape[0], picked.total, picked.m
    assert n == reference("noise_030", 6)[0] and total > m
    hist = torch.full((W * total,), 77, dtype=torch.int64, device=dev)
    _lib.check(L.tomo_cc_breadth_hist(*cr.hist_head(picked), _p(hist), total - 1, st), "tomo_cc_breadth_hist")
    assert pipeline._download(cr.tot)[2] == 2
    assert hist[:W * (total - 1)].eq(0).all() and hist[W * (total - 1):].eq(77).all()
    out = torch.full((m,), 77.0, dtype=torch.float64, device=dev)
    euler = torch.full((m, 13), 77, dtype=torch.int64, device=dev)
    labels = torch.full((m,), 77, dtype=torch.int64, device=dev)
    tab = torch.from_numpy(pipeline.breadth_factors(None, nz)).to(dev)
    _lib.check(L.tomo_cc_breadth(*cr.finish_head(picked), _p(hist), total - 1, _p(tab), nz, 13, _p(out), _p(euler), _p(labels), m, st),
               "tomo_cc_breadth")
    assert out.eq(77.0).all() and euler.eq(77).all() and labels.eq(77).all()
    with pytest.raises(_lib.TomoError):
        cr._checked()

    cr = pipeline.ComponentRuns(vol, 6)                          # ... and one result row short
    picked = cr.select(0, False)
    _lib.check(L.tomo_cc_breadth_hist(*cr.hist_head(picked), _p(hist), total, st), "tomo_cc_breadth_hist")
    assert pipeline._download(cr.tot)[2] == 0
    per = reference("noise_030", 6)[2]
    got = hist.cpu().numpy().reshape(total, W)
    off = picked.off.cpu().numpy()
    box = picked.table.cpu().numpy()[:, 1:3]
    cross = [13 + f for f in range(13) if R.NORMALS[f] != (1, 0, 0)]

    def filed(c, lo, hi):
        """What the entries of component c hold of the reference's slices lo .. hi: the cross parts, and chi^in of (1, 0, 0)
        = voxels - edges x - edges y + squares from the raw counts."""
        e = got[off[c]:off[c + 1]][lo - box[c, 0]:hi + 1 - box[c, 0]]
        assert np.array_equal(e[:, 6:], per[c, lo:hi + 1][:, cross])
        assert np.array_equal(e[:, 0] - e[:, 1] - e[:, 2] + e[:, 5], per[c, lo:hi + 1, R.NORMALS.index((1, 0, 0))])
        assert np.array_equal(e[:, 0] - e[:, 2], per[c, lo:hi + 1, R.NORMALS.index((0, 0, 1))])
        assert np.array_equal(e[:, 0] - e[:, 3], per[c, lo:hi + 1, R.NORMALS.index((0, 1, -1))])
        assert np.array_equal(e[:, 0] - e[:, 4], per[c, lo:hi + 1, R.NORMALS.index((0, 1, 1))])

    for c in (0, 1, n // 2, n - 1):
        filed(c, box[c, 0], box[c, 1])
    _lib.check(L.tomo_cc_breadth(*cr.finish_head(picked), _p(hist), total, _p(tab), nz, 13, _p(out), _p(euler), _p(labels), m - 1, st),
               "tomo_cc_breadth")
    assert pipeline._download(cr.tot)[2] == 2
    assert out.eq(77.0).all() and euler.eq(77).all() and labels.eq(77).all()

    # boxes that do not go with the bits (every box one slice late): bit 2, the voxels in front of a box add nothing and no add
    # leaves the histogram; run tables shorter than the runs: bit 2 for every run and nothing is added at all
    late = picked.table.clone()
    late[:, 1:3] += 1
    for tables, cap_runs in ((late, cr.runs), (picked.table, cr.runs - 1)):
        cr = pipeline.ComponentRuns(vol, 6)
        picked = cr.select(0, False)
        padded = torch.full((W * total + 64,), 77, dtype=torch.int64, device=dev)
        head = list(cr.hist_head(dataclasses.replace(picked, table=tables)))
        assert head[5] == cr.runs
        head[5] = cap_runs                                       # the one argument that is wrong on purpose
        _lib.check(L.tomo_cc_breadth_hist(*head, _p(padded), total, st), "tomo_cc_breadth_hist")
        assert pipeline._download(cr.tot)[2] == 4
        assert padded[W * total:].eq(77).all()
        got = padded[:W * total].cpu().numpy().reshape(total, W)
        if tables is late:
            for c in (0, 1, n // 2, n - 1):                      # what lies inside the late box is filed where it belongs
                if box[c, 1] > box[c, 0]:
                    e = got[off[c]:off[c + 1] - 1]
                    assert np.array_equal(e[:, 6:], per[c, box[c, 0] + 1:box[c, 1] + 1][:, cross])
                assert not got[off[c + 1] - 1].any()
        else:
            assert not got.any()

    monkeypatch.setattr(pipeline, "COMPONENT_HIST_BUDGET", 8 * W * total - 1)
    with pytest.raises(_lib.TomoError, match="min_voxels"):
        pipeline.component_breadth(vol)
    assert len(pipeline.component_breadth(vol, largest=True)) == 1       # one component is always granted
    monkeypatch.setattr(pipeline, "COMPONENT_HIST_BUDGET", 8 * W * total)
    assert len(pipeline.component_breadth(vol)) == n


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_fenced(dev, poison):
    """The noise volume of hundreds of components (every table ends in the middle of a tile) and the sponge (more than one
    workgroup of rows) inside fenced, poisoned buffers: the same integers and sums, clean fences."""
    names = (("noise_030", 6), ("sponge", 26))
    vols = {name: resident(name, dev)[1] for name, _ in names}

    def once(p):
        _devcache.clear()
        with F.fenced(p, F.package_modules(), seed=7) as fz:
            for name, conn in names:
                v, vol = FIXTURES[name], vols[name]
                n, sizes, per = reference(name, conn)
                d, mm_y, mm_x = spacing("odd", v.shape[0])
                with fz.unchanged(vol.bits):
                    same(pipeline.component_breadth(vol, d, mm_y, mm_x, conn), np.arange(1, n + 1), sizes, per, d, mm_y, mm_x, 13, "fenced")
                    same(pipeline.component_breadth(vol, d, mm_y, mm_x, conn, 2, True), P.selected(sizes, 2, True).astype(np.int64) + 1,
                         sizes, per, d, mm_y, mm_x, 13, "fenced largest")
                    whole = pipeline.mean_breadth(vol, d, mm_y, mm_x)
                    assert np.array_equal(whole.section_euler, R.section_euler(R.chi_whole(v)))
                    same_breadth(whole.mean_breadth_mm, R.chi_whole(v)[None], d, mm_y, mm_x, 13, "fenced whole")
            fz.check()
            assert fz.ran("_rows") >= 2 * 2 * 4 and fz.ran("mean_breadth") >= 2 * 2
    try:
        once(poison)
    except AssertionError as e:
        try:
            once("zero")
            control = "the zero control PASSES: the failure is a read of memory nobody wrote"
        except AssertionError as z:
            control = "the zero control fails too (%s): not a matter of the poison" % (str(z).splitlines() or [""])[0][:200]
        raise AssertionError("%s\n[%s] %s" % (e, poison, control)) from e
