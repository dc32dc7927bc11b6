"""GPU tier of the homotopic thinning (csrc/thin.hip -> pipeline.skeleton / skeleton_nodes / component_skeleton ->
volume_calculator.skeleton_report and component_properties(skeleton=True)).  Every expected volume comes from
tests/skeleton_reference.py, which tests every voxel in every sub-pass, and is compared byte for byte: a sub-pass reads the
volume as it stood when it began, so the bytes depend on no schedule and on no skipped tile.  The shapes are the smallest at
which the kernel can go wrong: (19, 21, 150) has tile and word tails on every axis and x crosses 63|64 and 127|128."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import fenced  # noqa: E402
import reconstruct_reference as R  # noqa: E402
import skeleton_reference as S  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _devcache, pipeline, volume_calculator  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (19, 21, 150)
MODES = ((26, True), (26, False), (6, False))
DENSITIES = (0.3, 0.5, 0.7)
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def resident(v, dev):
    return pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)


def memo(key, fn):
    """A reference computed once and shared, read-only."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def delta(c0, key):
    return pipeline.COUNTERS[key] - c0[key]


def same_volume(got, ref, what):
    assert isinstance(got, pipeline.BitVolume) and tuple(got.shape) == ref.shape and got.bits.dtype == torch.int64, what
    host = got.bits.cpu().numpy()
    if not np.array_equal(host, C.pack(ref)):                                         # the tail bits are zero as well
        bad = np.argwhere(C.unpack(host, ref.shape) != ref)
        raise AssertionError("%s: %d voxels differ, the first at %s" % (what, len(bad), bad[:1].tolist()))


# ------------------------------------------------------------------ the volumes
def corridor():
    """A one-voxel corridor through every tile of SHAPE: a line along x in every (z, y) tile column, joined into one serpentine."""
    v = np.zeros(SHAPE, dtype=bool)
    order = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2)]
    at = [(8 * bz + 2, 8 * by + 3) for bz, by in order]
    for k, (z, y) in enumerate(at):
        v[z, y, :] = True
        if k + 1 < len(at):
            z1, y1 = at[k + 1]
            x = SHAPE[2] - 1 if k % 2 == 0 else 0
            v[min(z, z1):max(z, z1) + 1, min(y, y1):max(y, y1) + 1, x] = True
    return v


def shapes_scene():
    """One scene: a bar along x through two word boundaries, a bar along z through three tiles, a torus and a hollow shell."""
    v = np.zeros((24, 40, 150), dtype=bool)
    v[2:7, 2:7, 30:141] = True
    v[1:23, 3:8, 4:9] = True
    v[10:19, 9:40, 20:51] |= S.torus((9, 31, 31), (4, 15, 15), 10, 3)
    v[9:24, 12:27, 70:85] |= S.shell((15, 15, 15), (7, 7, 7), 6, 3)
    return v


def full_block():
    return np.ones(SHAPE, dtype=bool)


VOLUMES = {"scene": shapes_scene, "grains": lambda: np.ascontiguousarray(R.scene()),
           "ball": lambda: S.ball((33, 33, 70), (16, 16, 35), 14), "corridor": corridor, "block": full_block,
           "empty": lambda: np.zeros(SHAPE, dtype=bool)}
for _d in DENSITIES:
    VOLUMES["noise%d" % int(10 * _d)] = (lambda d: lambda: S.noise(SHAPE, d, int(100 * d)))(_d)
# name -> the modes it is thinned under
CASES = [("noise%d" % int(10 * d), conn, curve, anchored) for d in DENSITIES for conn, curve in MODES for anchored in (False, True)]
CASES += [(name, conn, curve, False) for name in ("scene", "grains", "ball", "corridor", "block", "empty") for conn, curve in MODES]


def volume(name):
    return memo(("volume", name), VOLUMES[name])


def anchors_of(name):
    return memo(("anchors", name), lambda: S.noise(SHAPE, 0.02, 7 + len(name)))


def expected(name, conn, curve, anchored):
    """-> the reference's (skeleton, iterations)."""
    return memo(("skeleton", name, conn, curve, anchored),
                lambda: S.skeleton(volume(name), curve, conn, anchors_of(name) if anchored else None))


def check_case(dev, name, conn, curve, anchored):
    v = volume(name)
    ref, iterations = expected(name, conn, curve, anchored)
    vol = resident(v, dev)
    keep = resident(anchors_of(name), dev) if anchored else None
    before = vol.bits.clone()
    c0 = dict(pipeline.COUNTERS)
    got = pipeline.skeleton(vol, curve, conn, keep)
    same_volume(got, ref, (name, conn, curve, anchored))
    assert torch.equal(vol.bits, before) and got.bits.data_ptr() != vol.bits.data_ptr()          # the input is untouched
    assert delta(c0, "thin_calls") == 1
    if v.any():
        assert delta(c0, "thin_iterations") == iterations and delta(c0, "thin_passes") == 48 * iterations, (name, conn, curve)
    else:                                                                             # an empty volume launches no sub-pass
        assert delta(c0, "thin_iterations") == 0 and delta(c0, "thin_passes") == 0


@pytest.mark.parametrize("name,conn,curve,anchored", CASES)
def test_skeleton_matches_the_reference_byte_for_byte(dev, name, conn, curve, anchored):
    check_case(dev, name, conn, curve, anchored)


def test_the_scenes_that_try_the_skip_rule_are_what_they_claim():
    """The ball of R = 14 takes several iterations before its inner tiles lose a voxel -- a skip rule that is not conservative
    would leave them asleep -- and the corridor loses the corners of its serpentine and nothing else, so nearly every tile is
    idle after the first iteration.  Their bytes are compared above, in every mode."""
    ref, iterations = expected("ball", 26, False, False)
    assert iterations >= 4 and ref.sum() == 1
    v = volume("corridor")
    ref, iterations = expected("corridor", 26, True, False)
    assert iterations == 2 and v.sum() - ref.sum() == 2 * 8 and T.label(ref, 26)[1] == 1
    assert expected("corridor", 26, False, False)[1] > 48                             # a line shrinks for many iterations


def check_schedule(dev, monkeypatch):
    for name, conn, curve in (("noise5", 26, True), ("ball", 26, False), ("noise7", 6, False)):
        ref, iterations = expected(name, conn, curve, False)
        vol = resident(volume(name), dev)
        for batch in (1, 3):
            monkeypatch.setattr(pipeline, "THIN_ITERATION_BATCH", batch)
            c0 = dict(pipeline.COUNTERS)
            same_volume(pipeline.skeleton(vol, curve, conn), ref, (name, batch))
            assert delta(c0, "thin_iterations") == iterations
            assert delta(c0, "thin_passes") == 48 * batch * -(-iterations // batch)
    monkeypatch.setattr(pipeline, "THIN_ITERATION_BATCH", 1)


def test_the_batch_changes_neither_bytes_nor_iterations(dev, monkeypatch):
    check_schedule(dev, monkeypatch)


def check_topology(dev):
    for name, conn, curve in (("noise5", 26, True), ("noise5", 6, False), ("scene", 26, True), ("scene", 26, False)):
        vol = resident(volume(name), dev)
        a, b = pipeline.volume_topology(vol, conn), pipeline.volume_topology(pipeline.skeleton(vol, curve, conn), conn)
        assert a == b and a["components"] > 0, (name, conn, curve, a, b)


def test_topology_by_the_devices_own_tools(dev):
    check_topology(dev)
    a = pipeline.volume_topology(resident(volume("scene"), dev), 26)
    assert a["handles"] >= 1 and a["cavities"] == 1


def check_nodes(dev):
    for v in (expected("noise5", 26, True, False)[0], expected("scene", 26, True, False)[0], volume("noise3"), volume("block"),
              volume("empty")):
        ref = S.nodes(v)
        got = pipeline.skeleton_nodes(resident(v, dev))
        same_volume(got.ends, ref["ends"], "ends")
        same_volume(got.junctions, ref["junctions"], "junctions")
        assert (got.voxels, got.end_points, got.junction_voxels, got.isolated) == (
            ref["voxels"], ref["end_points"], ref["junction_voxels"], ref["isolated"])
        assert all(type(x) is int for x in (got.voxels, got.end_points, got.junction_voxels, got.isolated))


def test_skeleton_nodes(dev):
    check_nodes(dev)
    ref = S.nodes(expected("scene", 26, True, False)[0])
    assert ref["end_points"] >= 4                                                     # the two bars alone have four


def component_reference(v, s, conn, min_voxels=0, largest=False):
    """Per-label sums over scipy.ndimage.label of the ORIGINAL volume -> rows (label, voxels, skeleton, ends, junctions)."""
    labels, n = T.label(v, conn)
    nodes = S.nodes(s)
    rows = []
    for c in range(1, n + 1):
        m = labels == c
        rows.append((c, int(m.sum()), int((s & m).sum()), int((nodes["ends"] & m).sum()), int((nodes["junctions"] & m).sum())))
    rows = [r for r in rows if r[1] >= min_voxels]
    if largest and rows:
        rows = [max(rows, key=lambda r: (r[1], -r[0]))]
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def check_components(dev):
    for name, conn, curve, anchored in (("noise3", 26, True, False), ("noise5", 6, False, False), ("scene", 26, True, False),
                                        ("noise3", 26, True, True)):
        v = volume(name)
        s = expected(name, conn, curve, anchored)[0]
        vol = resident(v, dev)
        keep = resident(anchors_of(name), dev) if anchored else None
        for min_voxels, largest in ((0, False), (5, False), (3, True)):
            ref = component_reference(v, s, conn, min_voxels, largest)
            got = pipeline.component_skeleton(vol, conn, min_voxels, largest, curve, keep)
            rows = np.stack((got.labels, got.voxels, got.skeleton_voxels, got.end_points, got.junction_voxels), axis=1)
            assert np.array_equal(rows, ref), (name, conn, min_voxels, largest)
            p = pipeline.component_properties(vol, connectivity=conn, min_voxels=min_voxels, largest=largest)
            assert np.array_equal(p.labels, got.labels) and np.array_equal(p.voxels, got.voxels)
            assert (got.skeleton_voxels >= 1).all()                                   # every component owns a piece of the skeleton
    empty = pipeline.component_skeleton(resident(volume("empty"), dev))
    assert len(empty) == 0 and len(pipeline.component_skeleton(resident(volume("noise3"), dev), min_voxels=10 ** 6)) == 0


def test_component_skeleton(dev):
    check_components(dev)


def check_cavities(dev):
    v = np.zeros((16, 20, 100), dtype=bool)
    v[1:15, 1:19, 1:99] = True
    v[6:9, 8:11, 10:90] = False                                                       # a pore along x, through the word boundary
    v[3:6, 3:6, 3:6] = False
    v[4:12, 14, 40] = False                                                           # open at neither end: a third pore
    hollow = ~v
    ref = component_reference(hollow, S.skeleton(hollow, True, 26)[0], 26)
    ref = ref[1:]                                                                     # the first component is the outside
    got = pipeline.cavity_skeleton(resident(v, dev))
    rows = np.stack((got.labels, got.voxels, got.skeleton_voxels, got.end_points, got.junction_voxels), axis=1)
    assert np.array_equal(rows, ref) and len(ref) == 3


def test_cavity_skeleton(dev):
    check_cavities(dev)


def check_calculator(dev):
    v = np.ascontiguousarray(volume("scene"))
    depths = np.full(v.shape[0], 0.5)
    s, iterations = expected("scene", 26, True, False)
    _devcache.clear()
    rep = volume_calculator.skeleton_report(v)
    n = S.nodes(s)
    assert list(rep) == ["skeleton", "voxels", "end_points", "junction_voxels", "isolated", "iterations"]
    assert rep["skeleton"].dtype == np.bool_ and np.array_equal(rep["skeleton"], s)
    assert [rep[k] for k in list(rep)[1:]] == [n["voxels"], n["end_points"], n["junction_voxels"], n["isolated"], iterations]
    assert all(type(rep[k]) is int for k in list(rep)[1:])
    c0 = dict(pipeline.COUNTERS)
    plain = volume_calculator.component_properties(v, 0.9, 0.7, depths, connectivity=26, min_voxels=5, topology=True)
    assert delta(c0, "thin_calls") == 0 and delta(c0, "thin_nodes") == 0 and delta(c0, "component_skeleton") == 0      # off: nothing new
    full = volume_calculator.component_properties(v, 0.9, 0.7, depths, connectivity=26, min_voxels=5, topology=True, skeleton=True)
    assert delta(c0, "thin_calls") == 1 and delta(c0, "component_skeleton") == 1
    ref = component_reference(v, s, 26, 5)
    assert len(full) == len(plain) == len(ref) > 0
    for d, e, r in zip(full, plain, ref):
        assert list(d)[:len(e)] == list(e) and all(d[k] == e[k] for k in e)           # the other keys: unchanged, in their order
        assert list(d)[len(e):] == ["skeleton_voxels", "skeleton_ends", "skeleton_junctions"]
        assert (d["label"], d["voxels"], d["skeleton_voxels"], d["skeleton_ends"], d["skeleton_junctions"]) == tuple(r)
        assert all(type(d[k]) is int for k in ("skeleton_voxels", "skeleton_ends", "skeleton_junctions"))


def test_skeleton_report_and_component_properties(dev):
    check_calculator(dev)


# ------------------------------------------------------------------ fencing
def test_in_fenced_poisoned_buffers(dev, monkeypatch):
    """The whole set above once more, inside fenced buffers whose fresh payload is 0xFF: nothing is written outside a buffer and
    nothing is read before it was written.  The references are the shared ones."""
    with fenced.fenced("ff", fenced.package_modules()) as fz:
        for case in CASES:
            check_case(dev, *case)
        assert fz.check() >= len(CASES) and fz.ran("_skeleton") == 3 * len(CASES) - 6
        check_schedule(dev, monkeypatch)
        check_topology(dev)
        check_nodes(dev)
        assert fz.ran("_skeleton_nodes") >= 15
        check_components(dev)
        check_cavities(dev)
        check_calculator(dev)
        fz.check()
