"""CPU tier: tests/sweep_scale_reference.py against the per-feature references it stands in for at scale, on the small fixtures,
byte for byte -- so that the scale tier of the sweeps (tests/test_gpu_sweep_scale.py) leans on nothing nobody checked.  The
certificates accept the exact references and reject every single-voxel change; the level-set reconstruction equals the sweeps
and the plateau definition; a mosaic computed whole equals the assembly of its parts, and stops doing so for thinning at odd
offsets; the volumes are the pinned ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import geodesic_reference as G  # noqa: E402
import reconstruct_reference as R  # noqa: E402
import skeleton_reference as S  # noqa: E402
import sweep_scale_reference as X  # noqa: E402
import topology_reference as T  # noqa: E402
import zones_reference as Z  # noqa: E402

FIXTURES = {name: G.fixtures()[name] for name in ("noise_tiles", "noise_words")}
_cache = {}


def memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def exact(name, kind, conn):
    """-> (weights, seeds, Dijkstra's map, marker map, the reference's zones and their dist)."""
    def make():
        v = FIXTURES[name]
        w = G.weights(v.shape, kind)
        seeds = G.default_seeds(v)
        m = Z.scattered_markers(v)
        zone, dist, _ = Z.zones(v, m, *w, conn)
        return w, seeds, G.dijkstra(v, seeds, *w, conn), m, zone, dist
    return memo((name, kind, conn), make)


# ------------------------------------------------------------------ 1. the certificates
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_distance_certificate_accepts_dijkstra_and_rejects_one_ulp(name, conn, kind):
    v = FIXTURES[name]
    w, seeds, d, _, _, _ = exact(name, kind, conn)
    labels, _ = T.label(v, conn)
    assert X.distance_defects(v, seeds, d, *w, conn) is None and X.reach_defects(v, seeds, d, labels) is None
    assert X.distance_defects(v, G.seeds_mask(v.shape, seeds), d, *w, conn) is None              # the seeds as a bool volume
    rng = np.random.default_rng(3)
    finite = np.argwhere(v & np.isfinite(d))
    rejected = 0
    for at in finite[rng.choice(len(finite), 20, replace=False)]:
        for towards in (X.INF, -X.INF):
            bad = d.copy()
            bad[tuple(at)] = np.nextafter(d[tuple(at)], towards)
            said = X.distance_defects(v, seeds, bad, *w, conn)
            rejected += said is not None and "tile" in said
    assert rejected == 40                                                             # 20 of 20, up and down
    bad = d.copy()
    bad[tuple(np.argwhere(~v)[5])] = 1.0                                              # an unset voxel that is not +inf
    assert "unset" in X.distance_defects(v, seeds, bad, *w, conn)
    assert "float32" in X.distance_defects(v, seeds, d.astype(np.float64), *w, conn)


def test_the_distance_certificate_rejects_a_finite_value_in_an_unseeded_component():
    name, kind, conn = "noise_tiles", "sided", 6
    v = FIXTURES[name]
    w, seeds, d, _, _, _ = exact(name, kind, conn)
    labels, n = T.label(v, conn)
    dark = v & ~np.isfinite(d)
    assert dark.any() and n > 1
    sizes = np.bincount(labels[dark])
    whole = np.argmax(sizes)                                                          # the largest component no seed reaches
    bad = d.copy()
    bad[labels == whole] = 5.0                                                        # a plateau that would support itself ...
    assert "does not exceed" not in (X.distance_defects(v, seeds, bad, *w, conn) or "") and sizes[whole] >= 2
    assert X.distance_defects(v, seeds, bad, *w, conn) is not None                    # ... but is no sum over a neighbour
    assert "finite where no seed reaches" in X.reach_defects(v, seeds, bad, labels)
    one = d.copy()
    one[tuple(np.argwhere(labels == whole)[0])] = 5.0
    assert X.reach_defects(v, seeds, one, labels) is not None and X.distance_defects(v, seeds, one, *w, conn) is not None
    assert X.seeded_share(v, seeds, labels) == X.reached(v, seeds, labels).sum() / v.sum() < 1.0


def test_the_strictness_is_asserted():
    """A weight that vanishes against a large value makes a plateau that supports itself: the certificate says so."""
    v = np.ones((1, 1, 6), dtype=bool)
    wxy, wz = np.array([1.0, 1.0, 1.5], dtype=np.float32), np.ones((1, 4), dtype=np.float32)
    d = np.float32([0, 1, 2, 3, 4, 5]).reshape(v.shape)
    assert X.distance_defects(v, np.array([[0, 0, 0]]), d, wxy, wz, 6) is None
    big = (np.float32(2.0 ** 25) + d).astype(np.float32)                              # 2^25 + 1 == 2^25 in float32
    big[0, 0, 0] = 0.0
    assert "does not exceed" in X.distance_defects(v, np.array([[0, 0, 0]]), big, wxy, wz, 6)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_zone_certificate_accepts_the_reference_and_rejects_a_swapped_label(name, conn, kind):
    v = FIXTURES[name]
    w, _, _, m, zone, dist = exact(name, kind, conn)
    assert X.distance_defects(v, v & (m > 0), dist, *w, conn) is None
    assert X.zone_defects(v, m, dist, zone, *w, conn) is None
    assert np.array_equal(Z.cut(v, zone, conn), Z.cut(v, np.where(v, zone, 7), conn))               # the cut is pointwise over set voxels
    rng = np.random.default_rng(4)
    labels = np.unique(zone[zone > 0])
    zoned = np.argwhere(zone > 0)
    rejected = 0
    for at in zoned[rng.choice(len(zoned), 20, replace=False)]:
        at = tuple(at)
        for other in (zone[at] + 1, zone[at] - 1, int(rng.choice(labels[labels != zone[at]]))):
            bad = zone.copy()
            bad[at] = other
            rejected += X.zone_defects(v, m, dist, bad, *w, conn) is not None
    assert rejected == 60
    a, b = labels[0], labels[-1]
    swapped = np.where(zone == a, b, np.where(zone == b, a, zone)).astype(np.int32)   # two whole zones change places
    assert X.zone_defects(v, m, dist, swapped, *w, conn) is not None
    unzoned = zone.copy()
    unzoned[tuple(np.argwhere(v & (zone > 0) & ~(m > 0))[0])] = 0
    assert "none where it is finite" in X.zone_defects(v, m, dist, unzoned, *w, conn)


# ------------------------------------------------------------------ 2. the level sets
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_level_sets_equal_the_sweeps_and_the_plateau_definition(shape, conn):
    for density in (0.3, 0.7):
        seed = 100 * R.SHAPES.index(shape) + int(10 * density) + 1                    # the five-level cases of the GPU tier
        v = R.noise(shape, density, seed)
        for f, m in ((R.level_map(shape, 5, seed + 1), R.level_map(shape, 5, seed + 2)),
                     (X.level_map(shape, seed + 3), X.sparse_marker(shape, seed + 4, 0.01))):
            assert X.reconstruct(v, f, m, conn).tobytes() == R.reconstruct(v, f, m, conn).tobytes()
            assert X.reconstruct(v, f, m, conn).tobytes() == R.flood(v, f, m, conn).tobytes()
            domes = R.h_maxima(v, f, 1.0, conn)
            assert X.h_maxima(v, f, 1.0, conn).tobytes() == domes.tobytes()
            assert np.array_equal(X.regional_maxima(v, f, conn), R.plateau_maxima(v, f, conn))
            assert np.array_equal(X.extended_maxima(v, f, 1.0, conn), R.plateau_maxima(v, domes, conn))
    f = X.level_map(shape, 9)
    assert (np.signbit(f) & (f == 0)).any() and (~np.signbit(f) & (f == 0)).any() and len(np.unique(R.canon(f))) == 5
    g = X.reconstruct(v, f, f, conn)
    assert (g == 0).any() and not (np.signbit(g) & (g == 0)).any()                    # -0.0 comes back as +0.0
    with pytest.raises(AssertionError, match="at most"):
        X.reconstruct(v, R.float_map(shape, 1), R.float_map(shape, 2), conn)


# ------------------------------------------------------------------ 3. the mosaics
OFFSETS = [(2 * a, 2 * b, 2 * c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]     # jitter inside the 2 x 2 x 2 cells


def two_cubed(sizes):
    """Eight blocks in 2 x 2 x 2 cells, even offsets, boxes two clear voxels apart -> (shape, [(index, offset)])."""
    cell = tuple(max(s[a] for s in sizes) + 4 for a in range(3))
    cell = tuple(c + (c & 1) for c in cell)
    placed = [(i, tuple(cell[a] * ((i >> (2 - a)) & 1) + OFFSETS[(i * 3) % 8][a] for a in range(3))) for i in range(8)]
    shape = tuple(2 * c for c in cell)
    assert X.layout_defects(shape, sizes, placed, rules=("inside", "even", "apart")) is None     # eight blocks cannot cover the residues
    return shape, placed


@pytest.mark.parametrize("kind", ["unit", "sided"])
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_a_mosaic_of_distances_and_zones_is_the_assembly_of_its_parts(conn, kind):
    rng = np.random.default_rng(5)
    vols = [rng.random((5 + i % 3, 7, 20 + 3 * i)) < 0.6 for i in range(8)]
    marks = [Z.scattered_markers(v, 23) for v in vols]
    shape, placed = two_cubed([v.shape for v in vols])
    wxy, wz = G.weights(shape, kind)
    big = X.assemble(shape, vols, placed, False)
    assert big.sum() == sum(v.sum() for v in vols)
    bigm = X.assemble(shape, [X.shifted_labels(m, 1000 * i) for i, m in enumerate(marks)], placed, 0)
    zone, dist, _ = Z.zones(big, bigm, wxy, wz, conn)
    parts = [Z.zones(v, m, wxy, X.block_weights(wz, p[0], v.shape[0]), conn) for v, m, (_, p) in zip(vols, marks, placed)]
    assert dist.tobytes() == X.assemble(shape, [p[1] for p in parts], placed, X.INF).tobytes()
    want = X.assemble(shape, [np.where(p[0] > 0, p[0] + 1000 * i, 0).astype(np.int32) for i, p in enumerate(parts)], placed, 0)
    assert zone.tobytes() == want.tobytes()
    if kind == "sided":                                                               # the rows of the table matter: unit weights differ
        assert dist.tobytes() != X.assemble(shape, [Z.zones(v, m, *G.weights(v.shape, kind), conn)[1] for v, m in zip(vols, marks)],
                                            placed, X.INF).tobytes()
    top = X.shifted_labels(marks[0], 2 ** 31 - 1 - int(marks[0].max()))
    assert top.max() == 2 ** 31 - 1 and top.dtype == np.int32 and np.array_equal(top[marks[0] <= 0], marks[0][marks[0] <= 0])


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_a_mosaic_of_reconstructions_is_the_assembly_of_its_parts(conn):
    rng = np.random.default_rng(6)
    vols = [rng.random((5 + i % 3, 7, 20 + 3 * i)) < 0.7 for i in range(8)]
    masks = [R.float_map(v.shape, 20 + i, signed=True) for i, v in enumerate(vols)]
    marks = [R.float_map(v.shape, 30 + i, signed=True) for i, v in enumerate(vols)]
    shape, placed = two_cubed([v.shape for v in vols])
    big = X.assemble(shape, vols, placed, False)
    f, m = X.assemble(shape, masks, placed, np.float32(0)), X.assemble(shape, marks, placed, np.float32(0))
    want = X.assemble(shape, [R.reconstruct(v, a, b, conn) for v, a, b in zip(vols, masks, marks)], placed, np.float32(0))
    assert R.reconstruct(big, f, m, conn).tobytes() == want.tobytes()


@pytest.mark.parametrize("conn,curve", [(26, True), (26, False), (6, False)])
def test_a_mosaic_of_skeletons_is_the_assembly_of_its_parts(conn, curve):
    vols = [S.noise((7 + i % 2, 9, 20 + 2 * i), 0.4 + 0.05 * i, 40 + i) for i in range(8)]
    keeps = [S.noise(v.shape, 0.03, 50 + i) if i % 2 else None for i, v in enumerate(vols)]
    shape, placed = two_cubed([v.shape for v in vols])
    big = X.assemble(shape, vols, placed, False)
    anchors = X.assemble(shape, [np.zeros(v.shape, dtype=bool) if k is None else k for v, k in zip(vols, keeps)], placed, False)
    want = X.assemble(shape, [S.skeleton(v, curve, conn, k)[0] for v, k in zip(vols, keeps)], placed, False)
    got, iterations = S.skeleton(big, curve, conn, anchors)
    assert np.array_equal(got, want) and iterations == max(S.skeleton(v, curve, conn, k)[1] for v, k in zip(vols, keeps))


def test_thinning_at_odd_offsets_is_another_skeleton():
    """The parity rule of the mosaics, kept as a test: three blocks in (22, 28, 84) at even offsets give the translated small
    skeletons; moved by one voxel on every axis they do not -- the subfields are parities of the coordinates."""
    vols = [S.noise((8, 10, 30), 0.5, 60 + i) for i in range(3)]
    small = [S.skeleton(v, True, 26)[0] for v in vols]
    even = [(0, (2, 2, 2)), (1, (12, 4, 40)), (2, (2, 16, 50))]
    odd = [(k, tuple(a + 1 for a in p)) for k, p in even]
    shape = (22, 28, 84)
    sizes = [v.shape for v in vols]
    assert X.layout_defects(shape, sizes, even, rules=("inside", "even", "apart")) is None
    assert X.layout_defects(shape, sizes, odd, rules=("inside", "even", "apart")) == "an odd offset"
    assert np.array_equal(S.skeleton(X.assemble(shape, vols, even, False), True, 26)[0], X.assemble(shape, small, even, False))
    differ = S.skeleton(X.assemble(shape, vols, odd, False), True, 26)[0] != X.assemble(shape, small, odd, False)
    assert differ.sum() > 0


@pytest.mark.parametrize("family", list(X.PARTS))
def test_the_layout_of_the_tier_keeps_its_rules(family):
    names, placed = X.mosaic(family)
    parts = X.PARTS[family]()
    sizes = [parts[n][0].shape for n in names]
    assert X.layout_defects(X.SHAPE, sizes, placed) is None
    assert {k for k, _ in placed} == set(range(len(names))) and len(placed) >= 40     # every part takes part, many times
    lo = np.array([p for _, p in placed])
    assert {0, 2, 4, 6} == set((lo[:, 0] % 8).tolist()) == set((lo[:, 1] % 8).tolist()) and not (lo & 1).any()
    assert len(set((lo[:, 2] % 64).tolist())) >= 16
    hi = lo + np.array([sizes[k] for k, _ in placed])
    assert (lo[:, 2] // 64 != (hi[:, 2] - 1) // 64).any() and hi[:, 2].max() > 64 * 16   # across word boundaries, into the ragged word
    big = X.assemble(X.SHAPE, [parts[names[k]][0] for k, _ in placed], placed, False)
    assert X.digest(C.pack(big)) == X.SHA256[family] and int(big.sum()) == X.VOXELS[family] and len(placed) == X.BLOCKS[family]
    tiles = np.unique(np.argwhere(big) // np.array(X.TILE), axis=0)
    assert 3 * len(tiles) > X.tile_grid(X.SHAPE)[3]                                   # set voxels in a third of the tiles ...
    assert all(tiles[:, a].max() >= X.tile_grid(X.SHAPE)[a] - 2 for a in range(3))    # ... and up to the far faces
    close = [(0, (0, 0, 0)), (0, (0, 0, sizes[0][2] + sizes[0][2] % 2))]            # even, and less than two clear voxels on
    assert "apart" in X.layout_defects(X.SHAPE, sizes, close + placed[-1:])


# ------------------------------------------------------------------ 4. the pins
@pytest.mark.parametrize("name", list(X.MAKERS))
def test_the_pinned_volumes(name):
    v = X.volume(name)
    tz, ty, wx, tiles = X.tile_grid(v.shape)
    assert X.digest(C.pack(v)) == X.SHA256[name] and int(v.sum()) == X.VOXELS[name]
    assert tiles >= X.FLOOR > X.RESIDENT and wx >= 16
    assert v.shape[2] % 64 and v.shape[1] % 8 and v.shape[0] % 8                      # a ragged last word, ragged last tile rows
    for conn in C.CONNECTIVITIES:
        labels, n = T.label(v, conn)
        assert n == X.COUNTS[(name, conn)]
        if name == "noise":
            seeds = X.every_tile_seeds(v)
            assert len({X.tile_of(p) for p in seeds[v[tuple(seeds.T)]]}) == tiles     # a seed in every tile: the first sweep finds all dirty
            assert not v[tuple(seeds.T)].all()                                        # and some on unset voxels
            assert X.seeded_share(v, seeds, labels) >= X.SHARE
            one = X.corner_seed(v, labels)
            assert X.tile_of(one[0]) == (0, 0, 0) and X.seeded_share(v, one, labels) >= X.SHARE
    if name == "lattice":
        z, y, x = (s // 2 for s in v.shape)
        assert v[z - 12:z + 13, y - 12:y + 13, x - 12:x + 13].all()                   # the ball is solid
