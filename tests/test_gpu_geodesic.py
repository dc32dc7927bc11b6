"""GPU tier of the geodesic distance (csrc/geodesic.hip -> pipeline.geodesic_distance / geodesic_reach /
ComponentRuns.geodesic / component_geodesic / cavity_geodesic -> volume_calculator.component_properties(geodesic=True) and
closed_porosity(pore_geodesic=True)).  Every expected value comes from tests/geodesic_reference.py -- Dijkstra with np.float32
additions -- and is compared bit for bit: the relaxation has one fixed point, whatever the order of the tiles."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavities_reference as V  # noqa: E402
import component_thickness_reference as R  # noqa: E402
import components_reference as C  # noqa: E402
import fenced  # noqa: E402
import geodesic_reference as G  # noqa: E402
import thickness_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = G.fixtures()
PORES = R.pore_fixtures()
COMPONENT_CASES = G.COMPONENT_FIXTURES + ("noise_tiles", "weave", "coil", "ring")
FIELDS = ("labels", "voxels", "length_mm", "ends_index", "ends_mm", "chord_mm", "tortuosity")
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def resident(v, dev):
    return pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


def call_spacing(kind, nz):
    """The spacing as the calls take it: unit goes in as the defaults' None."""
    depths, mm_y, mm_x = T.spacing(kind, nz)
    return (None if kind == "unit" else depths), mm_y, mm_x


_cache = {}


def memo(key, fn):
    """A reference computed once and shared, read-only."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def reference_map(name, conn, kind, every=97):
    v = FIXTURES[name]
    return memo(("map", name, conn, kind, every), lambda: G.dijkstra(v, G.default_seeds(v, every), *G.weights(v.shape, kind), conn))


def labelled(name, conn):
    return memo(("labels", name, conn), lambda: C.label(FIXTURES[name], conn))


def delta(c0, key):
    return pipeline.COUNTERS[key] - c0[key]


def same_map(got, ref, what):
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == ref.shape, what
    host = got.cpu().numpy()
    if host.tobytes() != ref.tobytes():
        bad = np.flatnonzero(host.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
        at = np.unravel_index(int(bad[0]), ref.shape)
        raise AssertionError("%s: %d voxels differ, the first at %s: %r here, %r in the reference" % (what, len(bad), at, host[at], ref[at]))


def expected_rows(rows):
    """The reference's dicts as the arrays of pipeline.ComponentGeodesic."""
    m = len(rows)
    return {"labels": np.array([r["label"] for r in rows], dtype=np.int64).reshape(m),
            "voxels": np.array([r["voxels"] for r in rows], dtype=np.int64).reshape(m),
            "length_mm": np.array([r["length_mm"] for r in rows], dtype=np.float64).reshape(m),
            "ends_index": np.array([r["ends_index"] for r in rows], dtype=np.int64).reshape(m, 2, 3),
            "ends_mm": np.array([r["ends_mm"] for r in rows], dtype=np.float64).reshape(m, 2, 3),
            "chord_mm": np.array([r["chord_mm"] for r in rows], dtype=np.float64).reshape(m),
            "tortuosity": np.array([r["tortuosity"] for r in rows], dtype=np.float64).reshape(m)}


def check(got, rows, what):
    ref = expected_rows(rows)
    assert isinstance(got, pipeline.ComponentGeodesic) and len(got) == len(rows), (what, len(got), len(rows))
    for key in FIELDS:
        a, b = getattr(got, key), ref[key]
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, a.shape, b.dtype, b.shape)
        assert a.tobytes() == b.tobytes(), (what, key, a.reshape(-1)[:6], b.reshape(-1)[:6])     # bit for bit


# ------------------------------------------------------------------ the distance map
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_distance(dev, name, conn, kind):
    """Every fixture x connectivity x spacing; the seeds as an index array and as a BitVolume, some of them on unset voxels."""
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    seeds = G.default_seeds(v)
    ref = reference_map(name, conn, kind)
    before = vol.bits.clone()
    c0 = dict(pipeline.COUNTERS)
    got = pipeline.geodesic_distance(vol, seeds, *args, conn)
    same_map(got, ref, (name, conn, kind, "index"))
    mask = G.seeds_mask(v.shape, seeds)
    assert v.all() or (mask & ~v).any()                                             # seeds on unset voxels: ignored
    sbits = resident(mask, dev)
    sbefore = sbits.bits.clone()
    same_map(pipeline.geodesic_distance(vol, sbits, *args, connectivity=conn), ref, (name, conn, kind, "bits"))
    same_map(pipeline.geodesic_distance(vol, torch.from_numpy(seeds).to(dev), *args, conn), ref, (name, conn, kind, "device index"))
    assert delta(c0, "geodesic_calls") == 3
    assert (delta(c0, "geodesic_sweeps") > 0) == bool((mask & v).any())
    assert torch.equal(vol.bits, before) and torch.equal(sbits.bits, sbefore), "an input volume was modified"
    print("%s/%d/%s: %d set voxels, %d reached, %d sweeps for three calls" % (name, conn, kind, int(v.sum()), int(np.isfinite(ref).sum()),
                                                                             delta(c0, "geodesic_sweeps")))


@pytest.mark.parametrize("name", ["noise_tiles", "empty", "one_voxel_clear", "full"])
def test_no_seed_launches_no_sweep(dev, name):
    v = FIXTURES[name]
    vol = resident(v, dev)
    off = np.argwhere(~v)[:3].astype(np.int64).reshape(-1, 3)
    for seeds in (off, np.zeros((0, 3), dtype=np.int64), resident(G.seeds_mask(v.shape, off), dev), resident(np.zeros_like(v), dev)):
        c0 = dict(pipeline.COUNTERS)
        got = pipeline.geodesic_distance(vol, seeds)
        same_map(got, np.full(v.shape, INF, dtype=np.float32), name)
        assert delta(c0, "geodesic_sweeps") == 0 and delta(c0, "geodesic_calls") == 1
        reached = pipeline.geodesic_reach(vol, seeds)
        assert not pipeline.unpack(reached).any() and delta(c0, "geodesic_sweeps") == 0


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_one_seed_on_the_border_of_its_tile(dev, conn):
    """A seed is lowered by nobody: the neighbouring tiles next to it have to be told by the seeding pass.  One seed on a face, an
    edge and a corner of its tile, in a solid block of 2 x 3 x 3 tiles, as an index and as bits."""
    v = np.ones((9, 17, 130), dtype=bool)
    vol = resident(v, dev)
    w = G.weights(v.shape, "sided")
    args = call_spacing("sided", v.shape[0])
    for seed in ((3, 3, 63), (3, 3, 64), (7, 4, 20), (8, 4, 20), (2, 8, 100), (7, 7, 63), (8, 8, 64), (8, 16, 128), (0, 0, 0)):
        seeds = np.array([seed], dtype=np.int64)
        ref = memo(("border", seed, conn), lambda: G.dijkstra(v, seeds, *w, conn))
        assert np.isfinite(ref).all()
        same_map(pipeline.geodesic_distance(vol, seeds, *args, conn), ref, (seed, conn, "index"))
        same_map(pipeline.geodesic_distance(vol, resident(G.seeds_mask(v.shape, seeds), dev), *args, conn), ref, (seed, conn, "bits"))


# ------------------------------------------------------------------ reach
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name,kind", [("noise_031", "sided"), ("noise_tiles", "unit"), ("serpentine", "dyadic"), ("words_130", "sided"),
                                       ("comb", "unit")])
def test_reach(dev, name, kind, conn):
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    seeds = G.default_seeds(v)
    ref = reference_map(name, conn, kind)
    before = vol.bits.clone()
    finite = np.unique(ref[np.isfinite(ref)])
    assert len(finite) >= 3
    on = float(finite[len(finite) // 2])                                              # exactly on a distance: <= keeps it
    between = (float(finite[len(finite) // 3]) + float(finite[len(finite) // 3 + 1])) / 2.0
    for r in (None, on, between, 0.0, float(finite[-1]), 1e30):
        got = pipeline.geodesic_reach(vol, seeds, r, *args, conn)
        assert isinstance(got, pipeline.BitVolume) and got.shape == v.shape and got.bits.dtype == torch.int64
        exp = G.reach(v, ref, r)
        assert np.array_equal(got.bits.cpu().numpy(), C.pack(exp)), (name, conn, kind, r)      # the tail bits are zero as well
    assert G.reach(v, ref, on).sum() > G.reach(v, ref, np.nextafter(np.float32(on), np.float32(0))).sum()
    labels, n = labelled(name, conn)                                                  # None: the components a seed touches
    touched = np.unique(labels[G.seeds_mask(v.shape, seeds) & v])
    assert np.array_equal(pipeline.unpack(pipeline.geodesic_reach(vol, seeds, None, *args, conn)).cpu().numpy(), np.isin(labels, touched) & v)
    assert torch.equal(vol.bits, before)


# ------------------------------------------------------------------ the farthest-point search
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", COMPONENT_CASES)
def test_components(dev, name, conn, kind):
    """ComponentRuns.geodesic / component_geodesic against the reference rows: the three rules x sweeps 2 and 3, on ONE labelling;
    the map of the last search under the selected components, +inf everywhere else."""
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    labels, n = labelled(name, conn)
    before = vol.bits.clone()
    runs = pipeline.ComponentRuns(vol, conn)
    c0 = dict(pipeline.COUNTERS)
    calls = 0
    for min_voxels, largest in R.RULES:
        picked = G.select_labels(labels, n, min_voxels, largest)
        for sweeps in (2, 3):
            rows, dist = memo(("rows", name, conn, kind, min_voxels, largest, sweeps),
                              lambda: G.search(v, labels, n, picked, kind, conn, sweeps))
            what = (name, conn, kind, min_voxels, largest, sweeps)
            got = runs.geodesic(*args, sweeps, min_voxels, largest)
            calls += 1
            check(got, rows, what)
            if len(rows):
                same_map(runs.last_geodesic_map, dist, what)
                assert np.isinf(dist[~np.isin(labels, picked)]).all()                 # an unselected component stays at +inf
            else:
                assert runs.last_geodesic_map is None
    assert delta(c0, "components_label") == 0 and delta(c0, "component_geodesic") == calls
    assert delta(c0, "components_measure") == (1 if n else 0)
    rows, _ = memo(("rows", name, conn, kind, 5, False, 3), lambda: None)
    got = pipeline.component_geodesic(vol, *args, conn, 3, 5)                         # the public call
    check(got, rows, (name, conn, kind, "public"))
    p = pipeline.component_properties(vol, *args, conn, 5)                            # the rows are component_properties'
    assert np.array_equal(p.labels, got.labels) and np.array_equal(p.voxels, got.voxels)
    assert torch.equal(vol.bits, before), "the input volume was modified"
    if name == "coil" and kind == "unit":
        assert got.tortuosity[0] > 2.0 and got.length_mm[0] > 150.0
    if name == "one_voxel":
        assert got.length_mm.tolist() == [] and runs.geodesic(*args).length_mm.tolist() == [0.0] and runs.geodesic(*args).tortuosity.tolist() == [1.0]


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(PORES))
def test_pores(dev, name, conn, kind):
    v = np.ascontiguousarray(PORES[name])
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    for lo, hi in ((0, None), (28, None), (0, 27), (65, None)):
        for sweeps in (2, 3):
            rows, _ = memo(("pores", name, conn, kind, sweeps), lambda: G.enclosed(v, conn, kind, sweeps))
            rows = [r for r in rows if r["voxels"] >= lo and (hi is None or r["voxels"] <= hi)]
            if name == "pore_box":
                assert [r["voxels"] for r in rows] == [s for s in (27, 64) if s >= lo and (hi is None or s <= hi)]
            got = pipeline.cavity_geodesic(vol, *args, conn, sweeps, lo, hi)
            check(got, rows, (name, conn, kind, lo, hi, sweeps))
            cav = pipeline.cavity_table(vol, *args, conn, lo, hi)
            assert np.array_equal(cav.labels, got.labels) and np.array_equal(cav.voxels, got.voxels)
    if name == "pore_box" and kind == "unit":                                         # the crack, 1 x 4 x 16 voxels, corner to corner
        got = pipeline.cavity_geodesic(vol, connectivity=conn)
        assert got.voxels.tolist() == [27, 64] and got.length_mm[1] >= 15.0 and got.chord_mm[1] == np.sqrt(15.0 ** 2 + 3.0 ** 2)


def test_empty_and_nothing_selected(dev):
    for name in ("empty", "one_voxel_clear", "tie"):
        vol = resident(FIXTURES[name], dev)
        c0 = dict(pipeline.COUNTERS)
        got = pipeline.component_geodesic(vol, min_voxels=100)
        check(got, [], name)
        assert delta(c0, "geodesic_sweeps") == 0
        check(pipeline.cavity_geodesic(vol), [], name)


# ------------------------------------------------------------------ sweeps, batches and the limit
def weave_case(dev):
    v = FIXTURES["weave"]
    seeds = np.array([[0, 2, 0]], dtype=np.int64)
    ref = memo("weave", lambda: G.dijkstra(v, seeds, *G.weights(v.shape, "unit"), 6))
    return resident(v, dev), seeds, ref


def test_the_weave_needs_more_than_one_batch(dev):
    vol, seeds, ref = weave_case(dev)
    c0 = dict(pipeline.COUNTERS)
    same_map(pipeline.geodesic_distance(vol, seeds, connectivity=6), ref, "weave")
    assert delta(c0, "geodesic_sweeps") > pipeline.GEODESIC_SWEEP_BATCH
    assert delta(c0, "geodesic_sweeps") % pipeline.GEODESIC_SWEEP_BATCH == 0
    print("weave: %d sweeps" % delta(c0, "geodesic_sweeps"))


def test_the_sweep_limit_names_its_constant(dev, monkeypatch):
    vol, seeds, _ = weave_case(dev)
    monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_LIMIT", 1)
    c0 = dict(pipeline.COUNTERS)
    with pytest.raises(_lib.TomoError, match="GEODESIC_SWEEP_LIMIT"):
        pipeline.geodesic_distance(vol, seeds, connectivity=6)
    assert delta(c0, "geodesic_sweeps") == 1                                          # it returns promptly
    monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_LIMIT", 20)
    with pytest.raises(_lib.TomoError, match="GEODESIC_SWEEP_LIMIT"):
        pipeline.geodesic_distance(vol, seeds, connectivity=6)
    assert delta(c0, "geodesic_sweeps") == 21


@pytest.mark.parametrize("batch", [1, 8, 64])
def test_the_batch_does_not_change_the_bytes(dev, batch, monkeypatch):
    """Speculative clean sweeps and the swapping of the flags: the same bytes for every batch size, and run after run."""
    monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_BATCH", batch)
    vol, seeds, ref = weave_case(dev)
    for _ in range(2):
        c0 = dict(pipeline.COUNTERS)
        same_map(pipeline.geodesic_distance(vol, seeds, connectivity=6), ref, ("weave", batch))
        assert delta(c0, "geodesic_sweeps") % batch == 0
    for name, conn, kind in (("noise_tiles", 26, "sided"), ("snake3d", 6, "dyadic"), ("noise_words", 26, "unit")):
        v = FIXTURES[name]
        for _ in range(2):
            same_map(pipeline.geodesic_distance(resident(v, dev), G.default_seeds(v), *call_spacing(kind, v.shape[0]), conn),
                     reference_map(name, conn, kind), (name, batch))
    v = FIXTURES["coil"]
    rows, _ = memo(("rows", "coil", 26, "sided", 0, False, 3), lambda: G.per_component(v, 26, "sided"))
    check(pipeline.component_geodesic(resident(v, dev), *call_spacing("sided", v.shape[0]), 26), rows, ("coil", batch))


# ------------------------------------------------------------------ fenced, poisoned buffers
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_fenced(dev, poison):
    """One case per entry point inside fenced, poisoned buffers: no fence is touched, no poison is read."""
    name, conn, kind = "noise_tiles", 26, "sided"
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    seeds = G.default_seeds(v)
    sbits = resident(G.seeds_mask(v.shape, seeds), dev)
    ref = reference_map(name, conn, kind)
    labels, n = labelled(name, conn)
    rows, dist = memo(("rows", name, conn, kind, 5, False, 3), lambda: G.search(v, labels, n, G.select_labels(labels, n, 5), kind, conn, 3))
    pv = np.ascontiguousarray(PORES["pore_box"])
    pvol = resident(pv, dev)
    prows, _ = memo(("pores", "pore_box", 6, kind, 3), lambda: G.enclosed(pv, 6, kind, 3))
    with fenced.fenced(poison, modules=fenced.package_modules(), seed=5) as fz:
        with fz.unchanged(vol.bits, sbits.bits, pvol.bits):
            by_bits = pipeline.geodesic_distance(vol, sbits, *args, conn)             # tomo_geo_seed_bits, tomo_geo_sweep
            by_index = pipeline.geodesic_distance(vol, seeds, *args, conn)            # tomo_geo_seed_index
            ball = pipeline.geodesic_reach(vol, seeds, 3.0, *args, conn)              # tomo_geo_reach
            comp = pipeline.component_geodesic(vol, *args, conn, 3, 5)
            pores = pipeline.cavity_geodesic(pvol, *call_spacing(kind, pv.shape[0]), 6)
        fz.check()                                                                    # the fences are intact
        assert fz.total > 0 and fz.ran("_geodesic_map") >= 3 and fz.ran("geodesic") >= 2
    same_map(by_bits, ref, "fenced bits")
    same_map(by_index, ref, "fenced index")
    assert np.array_equal(ball.bits.cpu().numpy(), C.pack(G.reach(v, ref, 3.0)))
    check(comp, rows, "fenced components")
    check(pores, prows, "fenced pores")


# ------------------------------------------------------------------ the drop-in layer
BASE_KEYS = ["label", "voxels", "voxel_volume_mm3", "bounding_box", "dimensions", "centroid_mm", "centroid_index"]


@pytest.mark.parametrize("min_voxels,largest", R.RULES)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_component_properties_session(dev, conn, min_voxels, largest):
    """component_properties(geodesic=True): the reference's numbers from ONE labelling and ONE selection; with the flag off
    nothing new runs and nothing changes."""
    name, kind = "noise_tiles", "sided"
    v = np.ascontiguousarray(FIXTURES[name])
    depths, mm_y, mm_x = T.spacing(kind, v.shape[0])
    labels, n = labelled(name, conn)
    picked = G.select_labels(labels, n, min_voxels, largest)
    assert len(picked)
    new = ["geodesic_length_mm", "geodesic_ends_index", "tortuosity"]
    for sweeps in (2, 3):
        rows, _ = memo(("rows", name, conn, kind, min_voxels, largest, sweeps), lambda: G.search(v, labels, n, picked, kind, conn, sweeps))
        _devcache.clear()
        c0 = dict(pipeline.COUNTERS)
        plain = volume_calculator.component_properties(v, mm_x, mm_y, depths, conn, min_voxels, largest)
        assert {k: x - c0[k] for k, x in pipeline.COUNTERS.items() if x != c0[k]} == {"components_label": 1, "components_measure": 1,
                                                                                    "components_zhist": 1}      # as it was
        assert [list(p) for p in plain] == [BASE_KEYS] * len(picked)
        assert [p["label"] for p in plain] == picked.tolist() and [p["voxels"] for p in plain] == [r["voxels"] for r in rows]
        _devcache.clear()
        c0 = dict(pipeline.COUNTERS)
        with fenced.fenced("zero", fenced.package_modules()) as fz:
            got = volume_calculator.component_properties(v, mm_x, mm_y, depths, conn, min_voxels, largest, geodesic=True,
                                                         geodesic_sweeps=sweeps)
            fz.check()
            assert fz.ran("select") == 4 and fz.ran("_measure") == 1                  # one selection (four allocations), one table
        moved = {k: x - c0[k] for k, x in pipeline.COUNTERS.items() if x != c0[k]}
        assert moved.pop("geodesic_sweeps") > 0
        assert moved == {"components_label": 1, "components_measure": 1, "components_zhist": 1, "component_geodesic": 1,
                         "components_value": sweeps + 1}, moved
        direct = pipeline.component_geodesic(resident(v, dev), depths, mm_y, mm_x, conn, sweeps, min_voxels, largest)
        check(direct, rows, (conn, min_voxels, largest, sweeps))
        for i, (g, p) in enumerate(zip(got, plain)):
            assert list(g) == list(p) + new and {k: g[k] for k in p} == p             # the other keys: unchanged, in their order
            assert g["geodesic_length_mm"] == rows[i]["length_mm"] == direct.length_mm[i]
            assert g["geodesic_ends_index"] == tuple(rows[i]["ends_index"]) and g["tortuosity"] == rows[i]["tortuosity"]
            assert [type(g[k]) for k in new] == [float, tuple, float]
            assert all(type(x) is int for end in g["geodesic_ends_index"] for x in end)
    _devcache.clear()
    _memo.clear()


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_closed_porosity_session(dev, conn):
    v = np.ascontiguousarray(PORES["pore_box"])
    kind = "sided"
    depths, mm_y, mm_x = T.spacing(kind, v.shape[0])
    rows_all, _ = memo(("pores", "pore_box", conn, kind, 3), lambda: G.enclosed(v, conn, kind, 3))
    for lo, hi in ((0, None), (28, None), (0, 27), (65, None)):
        rows = [r for r in rows_all if r["voxels"] >= lo and (hi is None or r["voxels"] <= hi)]
        for pore_size in (False, True):
            _devcache.clear()
            c0 = dict(pipeline.COUNTERS)
            plain = volume_calculator.closed_porosity(v, mm_x, mm_y, depths, conn, lo, hi, pore_size=pore_size)
            moved = {k for k, x in pipeline.COUNTERS.items() if x != c0[k]}
            assert not any("geodesic" in k for k in moved)                            # off: nothing new runs
            if not pore_size:
                assert plain == V.porosity(v, conn, depths, mm_x, mm_y, lo, hi)       # ... and the report is what it was
            _devcache.clear()
            c0 = dict(pipeline.COUNTERS)
            got = volume_calculator.closed_porosity(v, mm_x, mm_y, depths, conn, lo, hi, pore_size=pore_size, pore_geodesic=True)
            moved = {k: x - c0[k] for k, x in pipeline.COUNTERS.items() if x != c0[k]}
            assert moved["components_label"] == 2 and moved["component_geodesic"] == 1 and "component_caliper" not in moved, moved
            assert [r["label"] for r in got["table"]] == [r["label"] for r in rows]
            for i, r in enumerate(got["table"]):
                assert (r["geodesic_length_mm"], r["tortuosity"]) == (rows[i]["length_mm"], rows[i]["tortuosity"])
                assert type(r["geodesic_length_mm"]) is float and type(r["tortuosity"]) is float
                assert list(r)[-2:] == ["geodesic_length_mm", "tortuosity"]
            assert got["longest_pore_path_mm"] == max((r["length_mm"] for r in rows), default=0.0) and list(got)[-1] == "longest_pore_path_mm"
            assert type(got["longest_pore_path_mm"]) is float
            stripped = {k: x for k, x in got.items() if k != "longest_pore_path_mm"}
            stripped["table"] = [{k: x for k, x in r.items() if k not in ("geodesic_length_mm", "tortuosity")} for r in got["table"]]
            assert stripped == plain and list(stripped) == list(plain)                # everything else is unchanged
    both = volume_calculator.closed_porosity(v, mm_x, mm_y, depths, conn, pore_size=True, pore_geodesic=True, pore_caliper=True)
    assert list(both)[-3:] == ["largest_pore_diameter_mm", "longest_pore_mm", "longest_pore_path_mm"]
    assert [r["geodesic_length_mm"] for r in both["table"]] == [r["length_mm"] for r in rows_all]
    _devcache.clear()
    _memo.clear()


def test_flags_off_is_the_code_as_it_was(dev):
    v = np.ascontiguousarray(FIXTURES["noise_tiles"])
    c0 = dict(pipeline.COUNTERS)
    rows_ = volume_calculator.component_properties(v, 1.0, 1.0, np.ones(v.shape[0]), shape=True, topology=True, surface=True)
    assert rows_ and all(not any("geodesic" in k or "tortuosity" in k for k in r) for r in rows_)
    report = volume_calculator.closed_porosity(np.ascontiguousarray(PORES["pore_box"]), 1.0, 1.0, np.ones(9), pore_size=True, pore_caliper=True)
    assert "longest_pore_path_mm" not in report and all(not any("geodesic" in k or "tortuosity" in k for k in r) for r in report["table"])
    assert not any("geodesic" in k for k, x in pipeline.COUNTERS.items() if x != c0[k])
    _devcache.clear()
    _memo.clear()
