"""GPU tier: surface area per component by the discretised Crofton formula on the resident bit volume
(csrc/component_measures.hip: tomo_cc_surface_hist, tomo_cc_surface -> pipeline.surface_area / component_surface ->
volume_calculator.surface_area / component_properties(..., surface=True)).

Every result is compared with tests/surface_reference.py -- the definition in NumPy on SciPy's labelling, its weights from
SciPy's spherical Voronoi cells, held to hand values by tests/test_surface_cpu.py -- never with a second run of the code under
test.  The counts are integers and compared with ==; the area is bit for bit the sequential float64 sum of the reference's
counts times pipeline.surface_factors, and within 1e-11 (relative) of the sum with the reference's own factors: the two
weight computations agree to 1e-14, the sum has a few thousand terms."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import component_props_reference as P  # noqa: E402
import components_reference as C  # noqa: E402
import fenced as F  # noqa: E402
import surface_reference as S  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
MM_X, MM_Y = 0.7, 0.45
KEY = "components_surface"


def _single(shape, at):
    v = np.zeros(shape, dtype=bool)
    v[at] = True
    return v


def _pair(shape, a, b):
    v = _single(shape, a)
    v[b] = True
    return v


def fixtures():
    """The volumes of the topology tests, then the smallest shapes at which the pass can go wrong."""
    out = dict(T.fixtures())
    for nx in (1, 63, 64, 65, 130):                              # runs and shifts across the words of a row
        out["rows_%d" % nx] = T.noise(0.5, (3, 4, nx), seed=nx)
    out["ny_1"] = T.noise(0.5, (4, 1, 70), seed=11)
    out["nz_1"] = T.noise(0.5, (1, 5, 70), seed=12)
    out["full_words"] = np.ones((2, 3, 128), dtype=bool)         # every transition is with the outside
    out["corner_low"] = _single((3, 3, 3), (0, 0, 0))
    out["corner_high"] = _single((2, 3, 66), (1, 2, 65))
    out["edge_pair"] = _pair((1, 2, 2), (0, 0, 0), (0, 1, 1))    # two voxels that touch by an edge only
    out["edge_pair_z"] = _pair((2, 1, 66), (0, 0, 63), (1, 0, 64))     # ... across a word seam and two slices
    for d in (0.1, 0.5, 0.9):
        out["dense_%03d" % round(100 * d)] = T.noise(d, (5, 7, 130), seed=23)
    return out


FIXTURES = fixtures()
CASES = [(name, conn) for name in FIXTURES for conn in C.CONNECTIVITIES]


def depths(nz):
    return S.VARIABLE_DEPTHS[:nz].copy()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def resident(name, dev):
    """The BitVolume of a case, uploaded as bits: the kernels under test are the only ones that run."""
    v = FIXTURES[name]
    return v, pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


_ref = {}


def reference(name, conn):
    """(n, sizes, counts int64 (n, nz, 11)) of the helper, computed once per case."""
    if (name, conn) not in _ref:
        v = FIXTURES[name]
        labels, n = T.label(v, conn)
        per = S.component_counts(labels, n)
        assert np.array_equal(per.sum(axis=0), S.counts(v))      # the components add up to the unlabelled volume
        _ref[(name, conn)] = (n, C.sizes(labels, n), per)
    return _ref[(name, conn)]


def same_area(got, n, d, directions, what):
    """One area of the device against the reference's counts n (nz, 11)."""
    nz = len(n)
    exact = S.area(n, pipeline.surface_factors(d, nz, MM_Y, MM_X, directions))
    free = S.area(n, S.factors(d, nz, MM_Y, MM_X, directions))
    assert float(got) == exact, (what, float(got), exact)
    assert abs(float(got) - free) <= 1e-11 * free, (what, float(got), free)


def same(got, pick, sizes, per, d, directions, what):
    """A ComponentSurface against the helper's rows for the labels `pick` (1-based, ascending)."""
    pick = np.asarray(pick, dtype=np.int64)
    assert got.labels.dtype == np.int64 and np.array_equal(got.labels, pick), (what, got.labels[:8], pick[:8])
    assert got.voxels.dtype == np.int64 and np.array_equal(got.voxels, sizes[pick - 1]), what
    exp = S.fold(per[pick - 1].sum(axis=1)).reshape(-1, 7)
    assert got.pair_counts.dtype == np.int64 and got.pair_counts.shape == exp.shape, (what, got.pair_counts.shape)
    assert np.array_equal(got.pair_counts, exp), (what, got.pair_counts[:4].tolist(), exp[:4].tolist())
    assert got.surface_area_mm2.dtype == np.float64 and got.surface_area_mm2.shape == (len(pick),)
    for i, c in enumerate(pick):
        same_area(got.surface_area_mm2[i], per[c - 1], d, directions, (what, int(c)))


@pytest.mark.parametrize("name,conn", CASES)
def test_counts_and_area_equal_the_reference(dev, name, conn):
    """Every fixture under both connectivities: the rows of all components, and the unlabelled call they add up to."""
    v, vol = resident(name, dev)
    n, sizes, per = reference(name, conn)
    d = depths(v.shape[0])
    before = vol.bits.clone()
    got = pipeline.component_surface(vol, d, MM_Y, MM_X, conn)
    same(got, np.arange(1, n + 1), sizes, per, d, 13, name)
    whole = pipeline.surface_area(vol, d, MM_Y, MM_X)
    n_whole = S.counts(v)
    assert whole.pair_counts.dtype == np.int64 and whole.pair_counts.shape == (7,)
    assert np.array_equal(whole.pair_counts, S.fold(n_whole.sum(axis=0)))
    assert np.array_equal(got.pair_counts.sum(axis=0), whole.pair_counts)
    assert isinstance(whole.surface_area_mm2, float)
    if v.any():
        same_area(whole.surface_area_mm2, n_whole, d, 13, name)
    else:
        assert whole.surface_area_mm2 == 0.0 and len(got) == 0
    assert torch.equal(vol.bits, before), "the input volume was modified"


@pytest.mark.parametrize("name,conn", [("noise_030", 6), ("sponge", 26), ("dense_050", 6), ("one_voxel", 6)])
def test_three_directions_and_unit_spacing(dev, name, conn):
    v, vol = resident(name, dev)
    n, sizes, per = reference(name, conn)
    d = depths(v.shape[0])
    got = pipeline.component_surface(vol, d, MM_Y, MM_X, conn, directions=3)
    same(got, np.arange(1, n + 1), sizes, per, d, 3, name)
    same_area(pipeline.surface_area(vol, d, MM_Y, MM_X, 3).surface_area_mm2, S.counts(v), d, 3, name)
    unit = pipeline.surface_area(vol)                            # slice_depths=None: 1.0 per slice
    exact = S.area(S.counts(v), pipeline.surface_factors(None, v.shape[0]))
    assert unit.surface_area_mm2 == exact and abs(exact - S.surface_area(v)) <= 1e-11 * exact


def test_the_hand_values(dev):
    _, vol = resident("one_voxel", dev)
    assert abs(pipeline.surface_area(vol).surface_area_mm2 - 3.00408) < 1e-5
    assert abs(pipeline.surface_area(vol, directions=3).surface_area_mm2 - 4.0) < 1e-12
    assert pipeline.surface_area(vol).pair_counts.tolist() == [2, 2, 4, 2, 4, 4, 8]
    _, vol = resident("edge_pair", dev)
    assert pipeline.component_surface(vol, connectivity=6).pair_counts.tolist() == [[2, 2, 3, 2, 4, 4, 8]] * 2
    assert pipeline.component_surface(vol, connectivity=26).pair_counts.tolist() == [[4, 4, 6, 4, 8, 8, 16]]
    for directions in (0, 4, 26):
        with pytest.raises(ValueError):
            pipeline.surface_area(vol, directions=directions)
        with pytest.raises(ValueError):
            pipeline.component_surface(vol, directions=directions)
    with pytest.raises(ValueError):
        pipeline.component_surface(vol, connectivity=18)


def test_an_empty_volume_gives_empty_arrays(dev):
    v, vol = resident("empty", dev)
    c0 = pipeline.COUNTERS[KEY]
    got = pipeline.component_surface(vol, None, MM_Y, MM_X, 26)
    assert len(got) == 0 and got.labels.shape == (0,) and got.voxels.shape == (0,) and got.surface_area_mm2.shape == (0,)
    assert got.pair_counts.shape == (0, 7) and got.pair_counts.dtype == np.int64 and got.surface_area_mm2.dtype == np.float64
    assert pipeline.COUNTERS[KEY] == c0                          # nothing was launched beyond the count of the runs
    assert volume_calculator.component_properties(v, MM_X, MM_Y, np.ones(v.shape[0]), surface=True) == []
    _devcache.clear()


def selections(sizes):
    return [(0, False), (int(np.median(sizes)), False), (2, False), (int(sizes.max()) + 1, False), (0, True), (2, True)]


@pytest.mark.parametrize("name,conn", [("noise_030", 6), ("dense_050", 6), ("dense_010", 26), ("straddle", 26), ("nested", 6)])
def test_selected_rows_are_those_of_component_properties(dev, name, conn):
    v, vol = resident(name, dev)
    n, sizes, per = reference(name, conn)
    d = depths(v.shape[0])
    for min_voxels, largest in selections(sizes):
        pick = P.selected(sizes, min_voxels, largest).astype(np.int64) + 1
        props = pipeline.component_properties(vol, d, MM_Y, MM_X, conn, min_voxels, largest)
        got = pipeline.component_surface(vol, d, MM_Y, MM_X, conn, min_voxels, largest)
        assert np.array_equal(got.labels, props.labels) and np.array_equal(got.voxels, props.voxels)
        same(got, pick, sizes, per, d, 13, (name, conn, min_voxels, largest))


def test_volume_calculator_dicts(dev):
    name, conn = "dense_010", 6
    v = FIXTURES[name]
    n, sizes, per = reference(name, conn)
    d = depths(v.shape[0])
    c0 = pipeline.COUNTERS[KEY]
    plain = volume_calculator.component_properties(v, MM_X, MM_Y, d, conn)
    assert volume_calculator.component_properties(v, MM_X, MM_Y, d, conn, surface=False) == plain
    assert pipeline.COUNTERS[KEY] == c0, "surface=False launched the surface kernels"
    assert all(not {"surface_area_mm2", "sphericity"} & set(g) for g in plain)
    got = volume_calculator.component_properties(v, MM_X, MM_Y, d, conn, surface=True)
    assert pipeline.COUNTERS[KEY] == c0 + 1
    assert [g["label"] for g in got] == list(range(1, n + 1))
    for g, p in zip(got, plain):
        assert sorted(g) == sorted(list(p) + ["surface_area_mm2", "sphericity"]) and all(g[k] == p[k] for k in p)
        assert type(g["surface_area_mm2"]) is float and type(g["sphericity"]) is float
        same_area(g["surface_area_mm2"], per[g["label"] - 1], d, 13, g["label"])
        assert g["sphericity"] == math.pi ** (1.0 / 3.0) * (6.0 * g["voxel_volume_mm3"]) ** (2.0 / 3.0) / g["surface_area_mm2"]
    three = volume_calculator.component_properties(v, MM_X, MM_Y, d, conn, 2, True, shape=True, surface=True, surface_directions=3)
    pick = P.selected(sizes, 2, True)
    assert [g["label"] for g in three] == (pick + 1).tolist()
    for g in three:
        assert "principal_axes" in g
        same_area(g["surface_area_mm2"], per[g["label"] - 1], d, 3, g["label"])
    whole = volume_calculator.surface_area(v, MM_X, MM_Y, d)
    assert sorted(whole) == ["sphericity", "surface_area_mm2", "voxel_volume_mm3"]
    same_area(whole["surface_area_mm2"], S.counts(v), d, 13, "whole")
    assert whole["voxel_volume_mm3"] == volume_calculator.VolumeCalculator().calculate_voxel_volume_variable_depth(v, MM_X, MM_Y, d)
    for bad in (v.astype(np.uint8), v[0], list(v)):
        with pytest.raises(TypeError):
            volume_calculator.surface_area(bad, MM_X, MM_Y, d)
    _devcache.clear()
    _memo.clear()


def test_the_ball_is_round(dev):
    """R = 16 at unit spacing: the area within 2 % of 4 pi R^2, the sphericity within 2 % of 1."""
    R, mm_x, mm_y, d, ny, nx = S.BALLS["r16_unit"]
    v = S.ball(R, mm_x, mm_y, d, ny, nx)
    (g,) = volume_calculator.component_properties(v, mm_x, mm_y, d, 6, surface=True)
    print("area / exact = %.5f, sphericity = %.5f" % (g["surface_area_mm2"] / (4 * math.pi * R * R), g["sphericity"]))
    assert g["surface_area_mm2"] == S.area(S.counts(v), pipeline.surface_factors(d, len(d), mm_y, mm_x))
    assert abs(g["surface_area_mm2"] / (4 * math.pi * R * R) - 1.0) < 0.02
    assert abs(g["sphericity"] - 1.0) < 0.02
    whole = volume_calculator.surface_area(v, mm_x, mm_y, d)
    assert whole["surface_area_mm2"] == g["surface_area_mm2"] and whole["sphericity"] == g["sphericity"]
    _devcache.clear()
    _memo.clear()


def test_the_guards_flag_instead_of_writing_outside_a_table(dev, monkeypatch):
    """A histogram shorter than tot[4]: bit 1 of the flags, the counters stay zero and nothing behind them is touched; the
    finishing kernel then writes no row.  The budget error names min_voxels."""
    L, st = _lib.lib(), _stream()
    v, vol = resident("noise_030", dev)
    nz = v.shape[0]
    cr = pipeline.ComponentRuns(vol, 6)
    picked = cr.select(0, False)
    n, total, m = picked.table.shape[0], picked.total, picked.m
    assert n == 293 and total > m
    surf = torch.full((11 * total,), 77, dtype=torch.int64, device=dev)
    _lib.check(L.tomo_cc_surface_hist(*cr.hist_head(picked), _p(surf), total - 1, st), "tomo_cc_surface_hist")
    assert pipeline._download(cr.tot)[2] == 2
    assert surf[:11 * (total - 1)].eq(0).all() and surf[11 * (total - 1):].eq(77).all()
    area = torch.full((m,), 77.0, dtype=torch.float64, device=dev)
    counts = torch.full((m, 7), 77, dtype=torch.int64, device=dev)
    labels = torch.full((m,), 77, dtype=torch.int64, device=dev)
    tab = torch.from_numpy(pipeline.surface_factors(None, nz)).to(dev)
    _lib.check(L.tomo_cc_surface(*cr.finish_head(picked), _p(surf), total - 1, _p(tab), nz, 13, _p(area), _p(counts), _p(labels), m, st),
               "tomo_cc_surface")
    assert area.eq(77.0).all() and counts.eq(77).all() and labels.eq(77).all()
    with pytest.raises(_lib.TomoError):
        cr._checked()

    cr = pipeline.ComponentRuns(vol, 6)                          # ... and one result row short
    picked = cr.select(0, False)
    _lib.check(L.tomo_cc_surface_hist(*cr.hist_head(picked), _p(surf), total, st), "tomo_cc_surface_hist")
    assert pipeline._download(cr.tot)[2] == 0
    per = reference("noise_030", 6)[2]
    got = surf.cpu().numpy().reshape(total, 11)
    off = picked.off.cpu().numpy()
    box = picked.table.cpu().numpy()[:, 1:3]
    for c in (0, 1, n // 2, n - 1):
        assert np.array_equal(got[off[c]:off[c + 1]], per[c, box[c, 0]:box[c, 1] + 1])
    _lib.check(L.tomo_cc_surface(*cr.finish_head(picked), _p(surf), total, _p(tab), nz, 13, _p(area), _p(counts), _p(labels), m - 1, st),
               "tomo_cc_surface")
    assert pipeline._download(cr.tot)[2] == 2
    assert area.eq(77.0).all() and counts.eq(77).all() and labels.eq(77).all()

    # boxes that do not go with the bits (every box one slice late): bit 2, the voxels in front of a box add nothing and no add
    # leaves the histogram; run tables shorter than the runs: bit 2 for every run and nothing is added at all
    late = picked.table.clone()
    late[:, 1:3] += 1
    for tables, cap_runs in ((late, cr.runs), (picked.table, cr.runs - 1)):
        cr = pipeline.ComponentRuns(vol, 6)
        picked = cr.select(0, False)
        padded = torch.full((11 * total + 64,), 77, dtype=torch.int64, device=dev)
        head = list(cr.hist_head(dataclasses.replace(picked, table=tables)))
        assert head[5] == cr.runs
        head[5] = cap_runs                                       # the one argument that is wrong on purpose
        _lib.check(L.tomo_cc_surface_hist(*head, _p(padded), total, st), "tomo_cc_surface_hist")
        assert pipeline._download(cr.tot)[2] == 4
        assert padded[11 * total:].eq(77).all()
        got = padded[:11 * total].cpu().numpy().reshape(total, 11)
        if tables is late:
            for c in (0, 1, n // 2, n - 1):                      # what lies inside the late box is counted where it belongs
                assert np.array_equal(got[off[c]:off[c + 1] - 1], per[c, box[c, 0] + 1:box[c, 1] + 1])
                assert not got[off[c + 1] - 1].any()
        else:
            assert not got.any()

    monkeypatch.setattr(pipeline, "COMPONENT_HIST_BUDGET", 88 * total - 1)
    with pytest.raises(_lib.TomoError, match="min_voxels"):
        pipeline.component_surface(vol)
    assert len(pipeline.component_surface(vol, largest=True)) == 1       # one component is always granted
    monkeypatch.setattr(pipeline, "COMPONENT_HIST_BUDGET", 88 * total)
    assert len(pipeline.component_surface(vol)) == n


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_fenced(dev, poison):
    """The noise volume of hundreds of components (every table ends in the middle of a tile) and the sponge (more than one
    workgroup of rows) inside fenced, poisoned buffers: the same counts, clean fences."""
    names = (("noise_030", 6), ("sponge", 26))
    vols = {name: resident(name, dev)[1] for name, _ in names}

    def once(p):
        _devcache.clear()
        with F.fenced(p, F.package_modules(), seed=7) as fz:
            for name, conn in names:
                v, vol = FIXTURES[name], vols[name]
                n, sizes, per = reference(name, conn)
                d = depths(v.shape[0])
                with fz.unchanged(vol.bits):
                    same(pipeline.component_surface(vol, d, MM_Y, MM_X, conn), np.arange(1, n + 1), sizes, per, d, 13, "fenced")
                    same(pipeline.component_surface(vol, d, MM_Y, MM_X, conn, 2, True), P.selected(sizes, 2, True).astype(np.int64) + 1,
                         sizes, per, d, 13, "fenced largest")
                    whole = pipeline.surface_area(vol, d, MM_Y, MM_X)
                    assert np.array_equal(whole.pair_counts, S.fold(S.counts(v).sum(axis=0)))
                    same_area(whole.surface_area_mm2, S.counts(v), d, 13, "fenced whole")
            fz.check()
            assert fz.ran("_rows") >= 2 * 2 * 4 and fz.ran("surface_area") >= 2 * 2
    try:
        once(poison)
    except AssertionError as e:
        try:
            once("zero")
            control = "the zero control PASSES: the failure is a read of memory nobody wrote"
        except AssertionError as z:
            control = "the zero control fails too (%s): not a matter of the poison" % (str(z).splitlines() or [""])[0][:200]
        raise AssertionError("%s\n[%s] %s" % (e, poison, control)) from e
