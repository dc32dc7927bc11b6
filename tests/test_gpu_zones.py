"""GPU tier of the geodesic zones, the cut and the separation (csrc/geodesic.hip -> pipeline.geodesic_zones / split_zones /
separate_components -> volume_calculator.separate_grains and component_properties(separate_mm=...)).  Every expected value
comes from tests/zones_reference.py and is compared byte for byte: the tight graph is fixed, so the label sweeps have one
fixed point whatever the order of the tiles."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import fenced  # noqa: E402
import geodesic_reference as G  # noqa: E402
import thickness_reference as T  # noqa: E402
import zones_reference as Z  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, _lib, _memo, pipeline, volume_calculator  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = {name: G.fixtures()[name] for name in ("noise_tiles", "noise_words", "weave")}
FIXTURES["dumbbell"] = Z.dumbbell()
INF = np.float32(np.inf)
ZONE_COUNTERS = ("zone_calls", "zone_sweeps", "zone_cuts", "separate_components")


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


def markers_of(name):
    """The int32 marker map of a fixture: labels that are not consecutive, entries on unset voxels, negative entries."""
    v = FIXTURES[name]
    if name == "weave":                                                              # one marker at each end of the path
        m = Z.end_markers(v) * 4 - 1                                                 # labels 7 and 3 ...
        m[m < 0] = 0
        m[~v & (np.indices(v.shape).sum(axis=0) % 37 == 0)] = 5                      # ... and entries on unset voxels
        return m.astype(np.int32)
    return Z.scattered_markers(v)


def reference(name, conn, kind, form):
    """-> (zones, dist, cut volume) of the reference for the int32 map ("map") or the bool volume of its positive entries ("bits")."""
    def make():
        v = FIXTURES[name]
        m = markers_of(name)
        zone, dist, _ = Z.zones(v, m if form == "map" else m > 0, *G.weights(v.shape, kind), conn)
        return zone, dist, Z.cut(v, zone, conn)
    return memo((name, conn, kind, form), make)


def separated(v_key, v, kind, r, conn):
    return memo(("separate", v_key, kind, r, conn), lambda: Z.separate(v, kind, r, conn))


def delta(c0, key):
    return pipeline.COUNTERS[key] - c0[key]


def same_map(got, ref, dtype, what):
    assert isinstance(got, torch.Tensor) and got.dtype == dtype and tuple(got.shape) == ref.shape, what
    host = got.cpu().numpy()
    if host.tobytes() != ref.tobytes():
        bad = np.flatnonzero(host.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
        at = np.unravel_index(int(bad[0]), ref.shape)
        raise AssertionError("%s: %d voxels differ, the first at %s: %r here, %r in the reference" % (what, len(bad), at, host[at], ref[at]))


def same_volume(got, ref, what):
    assert isinstance(got, pipeline.BitVolume) and tuple(got.shape) == ref.shape and got.bits.dtype == torch.int64, what
    assert np.array_equal(got.bits.cpu().numpy(), C.pack(ref)), what                 # the tail bits are zero as well


# ------------------------------------------------------------------ zones and the cut
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_zones_and_cut(dev, name, conn, kind):
    """Every fixture x connectivity x spacing; the markers as an int32 map with scattered labels and as a BitVolume."""
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    m = markers_of(name)
    assert ((m > 0) & ~v).any() and ((m > 0) & v).sum() >= 2 and not np.array_equal(np.unique(m[m > 0]), np.arange(1, len(np.unique(m[m > 0])) + 1))
    before = vol.bits.clone()
    for form in ("map", "bits"):
        zref, dref, cref = reference(name, conn, kind, form)
        given = torch.from_numpy(m).to(dev) if form == "map" else resident(m > 0, dev)
        kept = given.clone() if form == "map" else given.bits.clone()
        c0 = dict(pipeline.COUNTERS)
        zone, dist = pipeline.geodesic_zones(vol, given, *args, conn)
        same_map(dist, dref, torch.float32, (name, conn, kind, form, "dist"))
        same_map(zone, zref, torch.int32, (name, conn, kind, form, "zones"))
        out = pipeline.split_zones(vol, zone, conn)
        same_volume(out, cref, (name, conn, kind, form, "cut"))
        assert delta(c0, "zone_calls") == 1 and delta(c0, "zone_cuts") == 1 and delta(c0, "separate_components") == 0
        assert delta(c0, "zone_sweeps") > 0 and delta(c0, "geodesic_sweeps") > 0 and delta(c0, "geodesic_calls") == 0
        assert torch.equal(given if form == "map" else given.bits, kept), "the markers were modified"
        print("%s/%d/%s/%s: %d distance sweeps, %d label sweeps, %d voxels cut" % (name, conn, kind, form, delta(c0, "geodesic_sweeps"),
                                                                                  delta(c0, "zone_sweeps"), int(v.sum() - cref.sum())))
    assert cref.sum() < v.sum()
    ref_dist = G.dijkstra(v, (m > 0) & v, *G.weights(v.shape, kind), conn) if name == "weave" else None
    if ref_dist is not None:                                                         # dist is geodesic_distance's, byte for byte
        same_map(pipeline.geodesic_distance(vol, resident(m > 0, dev), *args, conn), ref_dist, torch.float32, "geodesic_distance")
        assert ref_dist.tobytes() == dref.tobytes()
    assert torch.equal(vol.bits, before), "the volume was modified"


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_a_map_with_entries_on_unset_voxels_cuts_nothing_there(dev, conn):
    """split_zones takes any int32 map: an entry on an unset voxel is no neighbour, an entry <= 0 is no zone."""
    v = FIXTURES["noise_tiles"]
    rng = np.random.default_rng(7)
    zone = rng.integers(-2, 6, v.shape).astype(np.int32)
    got = pipeline.split_zones(resident(v, dev), torch.from_numpy(zone).to(dev), conn)
    same_volume(got, Z.cut(v, zone, conn), conn)


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_a_rod(dev, conn):
    """1 x 1 x 9, label 2 at the left end and 1 at the right: the middle voxel is a tie and reads 1; the cut clears exactly one
    voxel, on the side of zone 2."""
    v = np.ones((1, 1, 9), dtype=bool)
    m = np.zeros(v.shape, dtype=np.int32)
    m[0, 0, 0], m[0, 0, 8] = 2, 1
    vol = resident(v, dev)
    zone, dist = pipeline.geodesic_zones(vol, torch.from_numpy(m).to(dev), connectivity=conn)
    assert dist.cpu().numpy()[0, 0].tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    assert zone.cpu().numpy()[0, 0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]
    out = pipeline.unpack(pipeline.split_zones(vol, zone, conn)).cpu().numpy()
    assert out[0, 0].tolist() == [True, True, True, False, True, True, True, True, True]


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_the_batch_size_does_not_change_the_bytes(dev, conn, monkeypatch):
    name, kind = "weave", "sided"
    v = FIXTURES[name]
    vol = resident(v, dev)
    given = torch.from_numpy(markers_of(name)).to(dev)
    zref, dref, _ = reference(name, conn, kind, "map")
    sweeps = {}
    for batch in (1, 8):
        monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_BATCH", batch)
        c0 = dict(pipeline.COUNTERS)
        zone, dist = pipeline.geodesic_zones(vol, given, *call_spacing(kind, v.shape[0]), conn)
        same_map(zone, zref, torch.int32, (conn, batch, "zones"))
        same_map(dist, dref, torch.float32, (conn, batch, "dist"))
        sweeps[batch] = (delta(c0, "geodesic_sweeps"), delta(c0, "zone_sweeps"))
        assert all(s % batch == 0 for s in sweeps[batch])
    assert sweeps[1][1] >= 8                                                         # the path crosses tile faces again and again
    assert all(b >= 16 for b in sweeps[8]), sweeps                                   # more than one batch in each phase


def test_the_sweep_limit_guards_the_label_phase(dev, monkeypatch):
    v = FIXTURES["weave"]
    given = torch.from_numpy(markers_of("weave")).to(dev)
    distances = pipeline._GeodesicPlan.propagate

    def then_a_small_limit(self, dist):
        done = distances(self, dist)
        monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_LIMIT", 2)
        return done
    monkeypatch.setattr(pipeline, "GEODESIC_SWEEP_BATCH", 1)
    monkeypatch.setattr(pipeline._GeodesicPlan, "propagate", then_a_small_limit)
    with pytest.raises(_lib.TomoError, match="geodesic zones: no fixed point after 2 sweeps .GEODESIC_SWEEP_LIMIT"):
        pipeline.geodesic_zones(resident(v, dev), given, connectivity=6)


# ------------------------------------------------------------------ the degenerate volumes
def test_empty_full_one_voxel_and_no_marker(dev):
    batch = pipeline.GEODESIC_SWEEP_BATCH
    # empty volume, markers everywhere: nothing is a marker
    v = np.zeros((3, 9, 70), dtype=bool)
    c0 = dict(pipeline.COUNTERS)
    zone, dist = pipeline.geodesic_zones(resident(v, dev), torch.full(v.shape, 3, dtype=torch.int32, device=dev))
    assert not zone.any() and torch.isinf(dist).all() and delta(c0, "zone_sweeps") == 0 and delta(c0, "geodesic_sweeps") == 0
    same_volume(pipeline.split_zones(resident(v, dev), zone), v, "empty")
    zone, _ = pipeline.geodesic_zones(resident(v, dev), resident(np.ones_like(v), dev))
    assert not zone.any() and delta(c0, "zone_sweeps") == 0
    # no marker on a set voxel: an all-zero map, a BitVolume without bits, entries <= 0, entries on unset voxels only
    v = FIXTURES["noise_tiles"]
    vol = resident(v, dev)
    off = np.where(v, 0, 4).astype(np.int32)
    for given in (torch.zeros(v.shape, dtype=torch.int32, device=dev), resident(np.zeros_like(v), dev),
                  torch.full(v.shape, -1, dtype=torch.int32, device=dev), torch.from_numpy(off).to(dev), resident(~v, dev)):
        c0 = dict(pipeline.COUNTERS)
        zone, dist = pipeline.geodesic_zones(vol, given)
        assert zone.dtype == torch.int32 and not zone.any() and torch.isinf(dist).all()
        assert delta(c0, "zone_sweeps") == 0 and delta(c0, "geodesic_sweeps") == 0 and delta(c0, "zone_calls") == 1
        same_volume(pipeline.split_zones(vol, zone), v, "no marker")
    # markers on every set voxel: zones == markers under the bits, one batch per phase and no second one
    m = np.where(v, np.arange(v.size, dtype=np.int32).reshape(v.shape) * 3 + 2, 0).astype(np.int32)
    c0 = dict(pipeline.COUNTERS)
    zone, dist = pipeline.geodesic_zones(vol, torch.from_numpy(np.where(v, m, 9).astype(np.int32)).to(dev))
    same_map(zone, m, torch.int32, "covered")
    same_map(dist, np.where(v, np.float32(0), INF).astype(np.float32), torch.float32, "covered")
    assert delta(c0, "geodesic_sweeps") == batch and delta(c0, "zone_sweeps") == batch
    # one voxel
    one = np.ones((1, 1, 1), dtype=bool)
    zone, dist = pipeline.geodesic_zones(resident(one, dev), torch.full((1, 1, 1), 5, dtype=torch.int32, device=dev))
    assert zone.cpu().numpy().tolist() == [[[5]]] and dist.cpu().numpy().tolist() == [[[0.0]]]
    same_volume(pipeline.split_zones(resident(one, dev), zone), one, "one voxel")
    # full, two markers in opposite corners, across a word boundary
    full = np.ones((3, 9, 66), dtype=bool)
    m = np.zeros(full.shape, dtype=np.int32)
    m[0, 0, 0], m[2, 8, 65] = 9, 4
    for conn in C.CONNECTIVITIES:
        zref, dref, _ = Z.zones(full, m, *G.weights(full.shape, "unit"), conn)
        zone, dist = pipeline.geodesic_zones(resident(full, dev), torch.from_numpy(m).to(dev), connectivity=conn)
        same_map(zone, zref, torch.int32, ("full", conn))
        same_map(dist, dref, torch.float32, ("full", conn))
        same_volume(pipeline.split_zones(resident(full, dev), zone, conn), Z.cut(full, zref, conn), ("full", conn))


# ------------------------------------------------------------------ the separation
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("kind,r", Z.DUMBBELL_CASES + (Z.DUMBBELL_WHOLE,))
def test_separate_components_on_the_dumbbell(dev, kind, r, conn):
    v = FIXTURES["dumbbell"]
    vol = resident(v, dev)
    ref = separated("dumbbell", v, kind, r, conn)
    whole = (kind, r) == Z.DUMBBELL_WHOLE
    before = vol.bits.clone()
    c0 = dict(pipeline.COUNTERS)
    sep = pipeline.separate_components(vol, r, *call_spacing(kind, v.shape[0]), conn)
    assert isinstance(sep, pipeline.Separation) and type(sep.markers) is int and type(sep.cut_voxels) is int
    assert (sep.markers, sep.cut_voxels) == (ref["markers"], ref["cut_voxels"]) and sep.markers == (0 if whole else 2)
    same_volume(sep.volume, ref["volume"], (kind, r, conn))
    same_map(sep.zones, ref["zones"], torch.int32, (kind, r, conn))
    assert pipeline.ComponentRuns(vol, conn).sizes().shape[0] == 1
    assert pipeline.ComponentRuns(sep.volume, conn).sizes().shape[0] == C.label(ref["volume"], conn)[1] == (1 if whole else 2)
    assert isinstance(sep.sweeps, tuple) and sep.sweeps == (delta(c0, "geodesic_sweeps"), delta(c0, "zone_sweeps"))
    assert (sep.sweeps == (0, 0)) == whole
    assert delta(c0, "separate_components") == 1 and delta(c0, "zone_calls") == 1 and delta(c0, "zone_cuts") == 1
    assert delta(c0, "distance_offset") == 1 and delta(c0, "components_filter") == 0
    assert torch.equal(vol.bits, before)
    if not whole:
        dropped = pipeline.separate_components(vol, r, *call_spacing(kind, v.shape[0]), conn, min_marker_voxels=10 ** 6)
        assert dropped.markers == 0 and dropped.cut_voxels == 0 and torch.equal(dropped.volume.bits, vol.bits)
        kept = pipeline.separate_components(vol, r, *call_spacing(kind, v.shape[0]), conn, min_marker_voxels=2)
        assert kept.markers == 2 and torch.equal(kept.volume.bits, sep.volume.bits)


def test_separate_grains_and_component_properties(dev):
    v = np.ascontiguousarray(FIXTURES["dumbbell"])
    depths = np.ones(v.shape[0])
    ref = separated("dumbbell", v, "unit", 3.0, 6)
    _devcache.clear()
    got = volume_calculator.separate_grains(v, 1.0, 1.0, depths, 3.0)
    assert list(got) == ["volume", "components_before", "components_after", "markers", "cut_voxels", "cut_share"]
    assert got["volume"].dtype == np.bool_ and np.array_equal(got["volume"], ref["volume"])
    assert (got["components_before"], got["components_after"], got["markers"], got["cut_voxels"]) == (1, 2, 2, ref["cut_voxels"])
    assert got["cut_share"] == ref["cut_voxels"] / 1848
    empty = volume_calculator.separate_grains(np.zeros((3, 4, 5), dtype=bool), 1.0, 1.0, np.ones(3), 1.0)
    assert not empty["volume"].any() and (empty["components_before"], empty["components_after"], empty["cut_share"]) == (0, 0, 0.0)
    # component_properties(separate_mm=...): the rows of the separated grains, every flag included
    _devcache.clear()
    rows = volume_calculator.component_properties(v, 1.0, 1.0, depths, separate_mm=3.0, shape=True, caliper=True)
    _devcache.clear()
    want = volume_calculator.component_properties(np.ascontiguousarray(ref["volume"]), 1.0, 1.0, depths, shape=True, caliper=True)
    assert len(rows) == 2 and rows == want and [list(a) for a in rows] == [list(b) for b in want]
    assert sum(r["voxels"] for r in rows) == 1848 - ref["cut_voxels"]
    assert all(r["max_caliper_mm"] < 15.0 for r in rows)                             # a ball of radius 6, not the pair
    # off: the answer of the call without the argument, and nothing new runs
    _devcache.clear()
    plain = volume_calculator.component_properties(v, 1.0, 1.0, depths, shape=True, caliper=True)
    _devcache.clear()
    c0 = dict(pipeline.COUNTERS)
    off = volume_calculator.component_properties(v, 1.0, 1.0, depths, separate_mm=None, shape=True, caliper=True)
    assert off == plain and len(plain) == 1 and plain[0]["max_caliper_mm"] > 20.0
    assert all(delta(c0, k) == 0 for k in ZONE_COUNTERS + ("geodesic_sweeps", "distance_offset"))
    _devcache.clear()
    _memo.clear()


def test_pore_bodies_joined_by_a_throat(dev):
    """separate_components(cavity_volume(v)): a solid block that holds the dumbbell as a void has one pore and two pore bodies."""
    void = np.pad(FIXTURES["dumbbell"], 1)
    v = ~void
    assert v[0].all() and v[:, 0].all() and v[:, :, 0].all()
    pores = pipeline.cavity_volume(resident(v, dev))
    same_volume(pores, void, "the pore space")
    assert pipeline.ComponentRuns(pores, 6).sizes().shape[0] == 1
    ref = separated("void", void, "unit", 3.0, 6)
    sep = pipeline.separate_components(pores, 3.0)
    assert sep.markers == 2 == ref["markers"] and sep.cut_voxels == ref["cut_voxels"] > 0
    same_volume(sep.volume, ref["volume"], "pore bodies")
    assert pipeline.ComponentRuns(sep.volume, 6).sizes().shape[0] == 2


# ------------------------------------------------------------------ fences and the budget
@pytest.mark.parametrize("poison", ["ff", "rand"])
def test_in_fenced_poisoned_buffers(dev, poison):
    name, conn, kind = "noise_tiles", 26, "sided"
    v = FIXTURES[name]
    vol = resident(v, dev)
    args = call_spacing(kind, v.shape[0])
    for form in ("map", "bits"):
        zref, dref, cref = reference(name, conn, kind, form)
        m = markers_of(name)
        given = torch.from_numpy(m).to(dev) if form == "map" else resident(m > 0, dev)
        with fenced.fenced(poison, fenced.package_modules()) as fz:
            with fz.unchanged(vol.bits, given if form == "map" else given.bits):
                zone, dist = pipeline.geodesic_zones(vol, given, *args, conn)
                out = pipeline.split_zones(vol, zone, conn)
            assert fz.check() >= 5 and fz.ran("_geodesic_zones") == 2 and fz.ran("_split_zones") == 2
        same_map(zone, zref, torch.int32, (poison, form))
        same_map(dist, dref, torch.float32, (poison, form))
        same_volume(out, cref, (poison, form))
    d = FIXTURES["dumbbell"]
    ref = separated("dumbbell", d, "sided", 2.0, 26)
    with fenced.fenced(poison, fenced.package_modules()) as fz:
        sep = pipeline.separate_components(resident(d, dev), 2.0, *call_spacing("sided", d.shape[0]), 26)
        fz.check()
    same_volume(sep.volume, ref["volume"], poison)
    same_map(sep.zones, ref["zones"], torch.int32, poison)


def test_the_budget_raises_before_any_allocation(dev, monkeypatch):
    v = FIXTURES["noise_tiles"]
    vol = resident(v, dev)
    given = torch.from_numpy(markers_of("noise_tiles")).to(dev)
    monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", 12 * v.size - 1)
    c0 = dict(pipeline.COUNTERS)
    with fenced.fenced("ff", fenced.package_modules()) as fz:
        for call in (lambda: pipeline.geodesic_zones(vol, given), lambda: pipeline.geodesic_zones(vol, resident(v, dev)),
                     lambda: pipeline.separate_components(vol, 1.0)):
            with pytest.raises(_lib.TomoError, match="GEODESIC_VOLUME_BUDGET"):
                call()
        assert fz.total == 0
    assert pipeline.COUNTERS == c0
    monkeypatch.setattr(pipeline, "GEODESIC_VOLUME_BUDGET", 12 * v.size)
    zone, _ = pipeline.geodesic_zones(vol, given)
    same_map(zone, reference("noise_tiles", 26, "unit", "map")[0], torch.int32, "at the budget")
