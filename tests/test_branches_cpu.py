"""CPU tier of the branch table of a skeleton: the reference (tests/branches_reference.py, shifted comparisons) against an
independent WALK -- it starts at every node voxel, follows each path voxel by voxel and classifies every step --, the
identities every table obeys, hand-checked rows of simple shapes, what pruning keeps, and the plumbing (exports, argument
checks before any device use, signatures).  None of it needs a GPU."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branches_reference as B  # noqa: E402
import skeleton_reference as S  # noqa: E402
import surface_reference as SR  # noqa: E402
import test_abi  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

NEW_SYMBOLS = ("tomo_branch_attach", "tomo_branch_clear", "tomo_branch_hist", "tomo_branch_lookup", "tomo_branch_split")
SHAPE = (7, 9, 70)
UNEVEN = np.array([0.5, 1.0, 2.0, 0.25, 0.5, 1.0, 1.0, 0.5])                          # dyadic: sums of them are exact
_cache = {}


def memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def fixtures():
    """name -> bool volume; computed once."""
    def build():
        out = {"noise%02d" % int(100 * d): S.noise(SHAPE, d, 3 + int(100 * d)) for d in (0.02, 0.1, 0.3)}
        out["thinned"] = S.skeleton(S.noise((9, 11, 70), 0.5, 4), True, 26)[0]
        out["torus"] = S.skeleton(S.torus((9, 31, 31), (4, 15, 15), 10, 3), True, 26)[0]
        out["bar_x"] = B.bar((3, 3, 70), (1, 1, 1), (0, 0, 1), 67)
        out["bar_z"] = B.bar((8, 3, 3), (0, 1, 1), (1, 0, 0), 8)
        out["diagonal"] = B.bar((9, 9, 9), (0, 0, 0), (1, 1, 1), 9)
        out["ring"], out["lollipop"], out["plus"], out["ypsilon"] = B.ring(), B.lollipop(), B.plus(), B.ypsilon()
        out["spur"], out["end_beside_junction"] = B.one_step_spur(), B.end_beside_junction()
        out["two"] = B.bar((2, 2, 3), (0, 0, 0), (1, 1, 1), 2)
        out["one"] = B.bar((1, 1, 1), (0, 0, 0), (0, 0, 0), 1)
        out["block"] = np.ones((4, 4, 4), dtype=bool)
        out["empty"] = np.zeros((3, 4, 5), dtype=bool)
        return out
    return memo("fixtures", build)


def table(name, depths=None, mm_y=1.0, mm_x=1.0):
    return memo(("table", name, None if depths is None else tuple(depths), mm_y, mm_x),
                lambda: B.table(fixtures()[name], depths, mm_y, mm_x))


# ------------------------------------------------------------------ the independent walk
def walk(vol):
    """-> the branches in the raster order of their first voxel: dicts with voxels (a set), counts (nz, 11), attached (the flat
    indices of the attached node voxels, with multiplicity).  No label array, no shifted comparison: neighbour lists."""
    vol = np.asarray(vol, dtype=bool)
    nz, ny, nx = vol.shape
    cells = set(map(tuple, np.argwhere(vol).tolist()))
    around = {p: [q for q in ((p[0] + dz, p[1] + dy, p[2] + dx) for dz, dy, dx in SR.STEPS) if q in cells] for p in cells}
    regular = {p for p in cells if len(around[p]) == 2}
    done, out = set(), []

    def step(branch, a, b):
        """the edge {a, b}, a regular: filed at a when b is a node voxel, else at the raster-earlier of the two"""
        if b in regular and b < a:
            a, b = b, a
        branch["counts"][a[0], SR.column(b[0] - a[0], b[1] - a[1], b[2] - a[2])] += 1

    def follow(prev, cur):
        branch = {"voxels": set(), "counts": np.zeros((nz, 11), dtype=np.int64), "attached": []}
        first = cur
        if prev is not None:                                                          # the attaching step
            step(branch, cur, prev)
            branch["attached"].append((prev[0] * ny + prev[1]) * nx + prev[2])
        while True:
            branch["voxels"].add(cur)
            done.add(cur)
            a, b = around[cur]
            nxt = b if a == prev else a
            if prev is None:                                                          # a cycle starts towards either side
                nxt = a
            if nxt not in regular:
                step(branch, cur, nxt)
                branch["attached"].append((nxt[0] * ny + nxt[1]) * nx + nxt[2])
                return branch
            step(branch, cur, nxt)
            if nxt == first:                                                          # the cycle is closed
                return branch
            prev, cur = cur, nxt

    for q in sorted(cells - regular):
        for p in around[q]:
            if p in regular and p not in done:
                out.append(follow(q, p))
    for p in sorted(regular):                                                         # what no node reaches: the cycles
        if p not in done:
            out.append(follow(None, p))
    return sorted(out, key=lambda b: min(b["voxels"]))


def node_facts(vol):
    """Per node in scipy's order: (voxels, free end), and the label array -- from scipy where it imports."""
    regular, nodes, deg = B.split(vol)
    labels, n = T.label(nodes, 26)
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
    free = np.array([sizes[c] == 1 and deg[labels == c + 1][0] == 1 for c in range(n)], dtype=bool).reshape(-1)
    return labels, sizes, free


@pytest.mark.parametrize("name", sorted(fixtures()))
def test_the_reference_agrees_with_the_walk(name):
    vol = fixtures()[name]
    t = table(name)
    b = t["branches"]
    paths = walk(vol)
    labels, sizes, free = node_facts(vol)
    assert len(paths) == len(b["label"]) and b["label"].tolist() == list(range(1, len(paths) + 1))
    flat_nodes = labels.reshape(-1)
    for i, p in enumerate(paths):
        assert b["voxels"][i] == len(p["voxels"]), (name, i)
        assert all(t["branch_labels"][v] == i + 1 for v in p["voxels"])               # labels ascend with the first voxel
        assert np.array_equal(t["counts"][i], p["counts"]), (name, i)
        assert t["attach_count"][i] == len(p["attached"]) and len(p["attached"]) in (0, 2)
        if p["attached"]:
            lo, hi = min(p["attached"]), max(p["attached"])
            assert b["attach_index"][i].tolist() == [lo, hi]
            assert b["nodes"][i].tolist() == [int(flat_nodes[lo]), int(flat_nodes[hi])]
            assert b["kind"][i] == 3 - int(free[flat_nodes[lo] - 1]) - int(free[flat_nodes[hi] - 1])
        else:
            assert b["attach_index"][i].tolist() == [-1, -1] and b["nodes"][i].tolist() == [0, 0] and b["kind"][i] == 0
            assert math.isnan(b["chord_mm"][i]) and math.isnan(b["tortuosity"][i])
        assert np.array_equal(b["step_counts"][i], SR.fold(p["counts"].sum(axis=0)))
    assert np.array_equal(t["nodes"]["voxels"], sizes) and np.array_equal(t["nodes"]["free_end"], free)


@pytest.mark.parametrize("name", sorted(fixtures()))
def test_the_identities(name):
    vol = fixtures()[name]
    t = table(name)
    b, n = t["branches"], t["nodes"]
    ref = S.nodes(vol)
    assert b["voxels"].sum() + n["voxels"].sum() == vol.sum() == t["voxels"]
    assert t["regular_voxels"] == b["voxels"].sum() and t["node_voxel_count"] == n["voxels"].sum()
    assert n["end_voxels"].sum() == ref["end_points"] + ref["isolated"] and n["junction_voxels"].sum() == ref["junction_voxels"]
    assert (n["end_voxels"] + n["junction_voxels"] == n["voxels"]).all() and t["isolated"] == ref["isolated"]
    assert n["branches"].sum() == 2 * int((b["kind"] != 0).sum())
    assert np.array_equal(t["regular"] | t["node_voxels"], vol) and not (t["regular"] & t["node_voxels"]).any()
    assert (b["step_counts"].sum(axis=1) == b["voxels"] + (b["kind"] != 0)).all()     # a path of v voxels has v + 1 edges, a cycle v


def test_min_voxels_selects_rows_and_nothing_else():
    vol = fixtures()["noise10"]
    full, some = table("noise10"), B.table(vol, min_voxels=3)
    keep = full["branches"]["voxels"] >= 3
    assert 0 < keep.sum() < len(keep)
    for k in ("label", "voxels", "length_mm", "attach_index", "nodes", "kind", "step_counts"):
        assert np.array_equal(some["branches"][k], full["branches"][k][keep]), k
    assert np.array_equal(some["nodes"]["voxels"], full["nodes"]["voxels"])
    assert some["nodes"]["branches"].sum() == 2 * int((some["branches"]["kind"] != 0).sum())


# ------------------------------------------------------------------ hand-checked rows
@pytest.mark.parametrize("mm_x", (1.0, 0.25, 2.0))
def test_a_bar_along_x(mm_x):
    t = B.table(fixtures()["bar_x"], None, 0.5, mm_x)
    b, n = t["branches"], t["nodes"]
    assert b["kind"].tolist() == [1] and b["voxels"].tolist() == [65] and n["free_end"].tolist() == [True, True]
    assert b["length_mm"][0] == 66 * mm_x and b["chord_mm"][0] == 66 * mm_x and b["tortuosity"][0] == 1.0
    assert b["step_counts"].tolist() == [[66, 0, 0, 0, 0, 0, 0]] and b["nodes"].tolist() == [[1, 2]]
    assert b["attach_index"].tolist() == [[(1 * 3 + 1) * 70 + 1, (1 * 3 + 1) * 70 + 67]] and n["branches"].tolist() == [1, 1]


def test_a_bar_along_z_under_uneven_depths():
    t = B.table(fixtures()["bar_z"], UNEVEN, 0.7, 0.9)
    b = t["branches"]
    zc = np.cumsum(UNEVEN) - UNEVEN / 2
    assert b["kind"].tolist() == [1] and b["voxels"].tolist() == [6] and b["step_counts"].tolist() == [[0, 0, 0, 7, 0, 0, 0]]
    assert b["length_mm"][0] == zc[7] - zc[0] == b["chord_mm"][0]                      # dyadic depths: every sum is exact
    assert t["counts"][0][:, 3].tolist() == [0, 1, 1, 1, 1, 1, 1, 0] and t["counts"][0][:, 7].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


def test_a_space_diagonal_bar():
    b = table("diagonal")["branches"]
    assert b["kind"].tolist() == [1] and b["voxels"].tolist() == [7] and b["step_counts"].tolist() == [[0, 0, 0, 0, 0, 0, 8]]
    assert abs(b["length_mm"][0] - 8 * math.sqrt(3)) < 1e-12 and abs(b["tortuosity"][0] - 1) < 1e-12


def test_a_square_ring_is_one_cycle():
    t = table("ring")
    b = t["branches"]
    assert len(t["nodes"]["label"]) == 0 and b["kind"].tolist() == [0] and b["voxels"].tolist() == [16]
    assert b["step_counts"].tolist() == [[6, 6, 4, 0, 0, 0, 0]] and abs(b["length_mm"][0] - (12 + 4 * math.sqrt(2))) < 1e-12
    assert b["attach_index"].tolist() == [[-1, -1]] and b["nodes"].tolist() == [[0, 0]]


def test_a_lollipop():
    t = table("lollipop")
    b, n = t["branches"], t["nodes"]
    assert b["kind"].tolist() == [3, 2] and b["nodes"].tolist() == [[1, 1], [1, 2]]    # the loop returns to its node
    assert n["voxels"].tolist() == [4, 1] and n["free_end"].tolist() == [False, True] and n["branches"].tolist() == [3, 1]
    assert b["voxels"].tolist() == [13, 5] and b["length_mm"][1] == 6.0


def test_a_plus():
    t = table("plus")
    b, n = t["branches"], t["nodes"]
    assert b["kind"].tolist() == [2, 2, 2, 2] and b["voxels"].tolist() == [2] * 4 and b["length_mm"].tolist() == [3.0] * 4
    assert sorted(n["voxels"].tolist()) == [1, 1, 1, 1, 5] and n["free_end"].sum() == 4 and n["branches"].max() == 4


def test_a_y_and_its_spur():
    vol = fixtures()["ypsilon"]
    b = table("ypsilon")["branches"]
    assert b["kind"].tolist() == [2, 2, 2] and sorted(b["length_mm"].tolist()) == [2.0, 19.0, 19.0]
    for rounds in (1, None):
        out, nb, nv, done = B.prune(vol, 5.0, rounds=rounds)
        assert (nb, nv, done) == (1, 2, 1)
        stub = B.ypsilon(short=1)                                                     # the bar with the voxel inside its node
        assert np.array_equal(out, stub)
        assert sorted(B.table(out)["branches"]["length_mm"].tolist()) == [19.0, 19.0]
    assert B.prune(vol, 2.0)[1] == 0                                                  # the bound is strict
    everything = B.prune(vol, 100.0, rounds=None)
    left = B.table(everything[0])["branches"]                                         # the T of four voxels: its two side voxels are
    assert everything[1] == 3 and everything[0].sum() == 4 and left["kind"].tolist() == [3, 3]     # regular now, between junctions


def test_an_end_beside_a_junction_and_a_one_step_spur():
    n = table("end_beside_junction")["nodes"]
    b = table("end_beside_junction")["branches"]
    assert sorted(zip(n["voxels"].tolist(), n["end_voxels"].tolist(), n["junction_voxels"].tolist(), n["free_end"].tolist())) == [
        (1, 1, 0, True), (1, 1, 0, True), (2, 1, 1, False)]
    assert b["kind"].tolist() == [2, 2] and b["voxels"].tolist() == [2, 2]
    n = table("spur")["nodes"]
    assert sorted(n["voxels"].tolist()) == [1, 1, 4] and table("spur")["branches"]["kind"].tolist() == [2, 2]


def test_two_voxels_one_voxel_a_block_and_nothing():
    for name, voxels, ends, junctions, isolated in (("two", 2, 2, 0, 0), ("one", 1, 1, 0, 1), ("block", 64, 0, 64, 0)):
        t = table(name)
        n = t["nodes"]
        assert len(t["branches"]["label"]) == 0 and t["regular_voxels"] == 0 and t["isolated"] == isolated
        assert (n["voxels"].tolist(), n["end_voxels"].tolist(), n["junction_voxels"].tolist()) == ([voxels], [ends], [junctions])
        assert n["free_end"].tolist() == [False] and n["branches"].tolist() == [0]
    t = table("empty")
    assert len(t["branches"]["label"]) == 0 and len(t["nodes"]["label"]) == 0 and t["voxels"] == 0


# ------------------------------------------------------------------ pruning
@pytest.mark.parametrize("name", ("thinned", "torus", "noise10", "noise30", "plus", "lollipop"))
def test_pruning_keeps_the_topology(name):
    vol = fixtures()[name]
    before = T.volume(T.components(vol, 26)[2])
    for rounds in (1, None):
        out, nb, nv, done = B.prune(vol, 4.0, UNEVEN[:vol.shape[0]] if vol.shape[0] <= 8 else None, 0.7, 0.9, rounds)
        assert not (out & ~vol).any() and vol.sum() - out.sum() == nv and (nb > 0) == (done > 0)
        assert T.volume(T.components(out, 26)[2]) == before, (name, rounds)
        if rounds is None:
            b = B.table(out, UNEVEN[:vol.shape[0]] if vol.shape[0] <= 8 else None, 0.7, 0.9)["branches"]
            assert not ((b["kind"] == 2) & (b["length_mm"] < 4.0)).any()
    assert B.prune(vol, 4.0, rounds=0)[1:] == (0, 0, 0)


def test_the_fixtures_prune_something():
    assert B.prune(fixtures()["thinned"], 4.0)[1] > 0 and B.prune(fixtures()["torus"], 6.0)[1] > 0
    out, nb, _, done = B.prune(fixtures()["thinned"], 4.0, rounds=None)
    assert done >= 1 and nb >= B.prune(fixtures()["thinned"], 4.0)[1]


# ------------------------------------------------------------------ the step table
@pytest.mark.parametrize("depths,mm_y,mm_x", ((None, 1.0, 1.0), (UNEVEN, 0.5, 0.25), (np.array([0.3, 1.7, 0.9, 0.31, 2.2]), 0.7, 0.9)))
def test_branch_steps(depths, mm_y, mm_x):
    nz = 6 if depths is None else len(depths)
    F = pipeline.branch_steps(depths, nz, mm_y, mm_x)
    assert F.dtype == np.float64 and F.shape == (nz, 11) and np.array_equal(F, B.steps(depths, nz, mm_y, mm_x))      # bitwise
    wxy, wz = pipeline.geodesic_weights(depths, nz, mm_y, mm_x)
    assert np.array_equal(F[:, :3].astype(np.float32), np.broadcast_to(wxy, (nz, 3)))
    assert np.array_equal(F[:-1, 3:7].astype(np.float32), wz) and np.array_equal(F[1:, 7:11].astype(np.float32), wz)
    assert F[-1, 3] == 0.0 and F[0, 7] == 0.0 and np.array_equal(F[-1, 4:7], F[-1, :3]) and np.array_equal(F[0, 8:11], F[0, :3])
    zt, _, _ = pipeline.distance_positions(depths, nz, mm_y, mm_x)
    assert np.array_equal(F[:-1, 3], np.diff(zt[1:-1]))
    for bad in ((np.ones(nz - 1), 1.0, 1.0), (np.ones(nz), 0.0, 1.0), (np.ones(nz), 1.0, float("nan")), (-np.ones(nz), 1.0, 1.0)):
        with pytest.raises(ValueError):
            pipeline.branch_steps(bad[0], nz, bad[1], bad[2])


# ------------------------------------------------------------------ the library without a GPU
def test_new_symbols_are_declared_and_bound():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("tomo_branch_")) == sorted(NEW_SYMBOLS)
    assert sorted(s for s in syms if s.startswith("tomo_branch_")) == sorted(NEW_SYMBOLS)
    assert {"skeleton_branches", "branch_split", "skeleton_branches_hist", "branch_attach", "branch_lookup", "branch_clear",
            "prune_rounds"} <= set(pipeline.COUNTERS)
    spec = pipeline._BRANCHES
    assert (spec.name, spec.columns, spec.words, spec.hist, spec.counter, spec.finish, spec.tables) == (
        "skeleton_branches", 0, 11, "tomo_branch_hist", "skeleton_branches_hist", "tomo_cc_surface", 1)
    assert spec.results == ((torch.float64, ()), (torch.int64, (7,)))


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(12)]
    a, b, c, d, e, f, g, h, i, j, k, m = (ctypes.addressof(x) for x in bufs)          # distinct host buffers, never dereferenced
    big = (1 << 12, 1 << 13, 1 << 12)                                                 # 2^31 words
    shapes = ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4))
    calls = {
        "tomo_branch_split": ([a, 4, 4, 4, b, c, d], (0, 4, 5, 6), ()),
        "tomo_branch_hist": ([a, 4, 4, 4, b, 8, c, d, e, f, 8, g, h, i, 8, j], (0, 4, 6, 7, 8, 9, 11, 12, 13, 15), (5, 10, 14)),
        "tomo_branch_attach": ([a, 4, 4, 4, b, 8, c, d, e, f, g, h, i, j, 8, 8], (0, 4, 6, 7, 8, 9, 10, 11, 12, 13), (5, 14, 15)),
        "tomo_branch_lookup": ([a, 4, 4, 4, b, 8, c, d, e, 8, f, 8, g], (0, 4, 6, 7, 8, 10, 12), (5, 9, 11)),
        "tomo_branch_clear": ([a, 4, 4, 4, b, 8, c, d, e, f, 8, g, h], (0, 4, 6, 7, 8, 9, 11, 12), (5, 10)),
    }
    for name, (good, pointers, sizes) in calls.items():
        fn = getattr(L, name)
        for bad in shapes:
            assert fn(*good[:1], *bad, *good[4:], None) == -1, name
        assert fn(*good[:1], *big, *good[4:], None) == -3, name
        for at in pointers:
            args = list(good)
            args[at] = None
            assert fn(*args, None) == -1, (name, at)
        for at in sizes:
            for bad in (0, -1):
                args = list(good)
                args[at] = bad
                assert fn(*args, None) == -1, (name, at)
    for name, at in (("tomo_branch_hist", 5), ("tomo_branch_hist", 10), ("tomo_branch_attach", 5), ("tomo_branch_attach", 14),
                     ("tomo_branch_attach", 15), ("tomo_branch_lookup", 5), ("tomo_branch_lookup", 9), ("tomo_branch_lookup", 11),
                     ("tomo_branch_clear", 5)):
        args = list(calls[name][0])
        args[at] = 1 << 31
        if name == "tomo_branch_clear":
            args[10] = 8
        assert getattr(L, name)(*args, None) == -3, (name, at)
    assert L.tomo_branch_hist(a, 4, 4, 4, b, 8, c, d, e, f, 8, g, h, i, (1 << 60) // 11, j, None) == -3
    assert L.tomo_branch_split(a, 4, 4, 4, a, c, d, None) == -1                       # in place
    assert L.tomo_branch_split(a, 4, 4, 4, b, a, d, None) == -1
    assert L.tomo_branch_split(a, 4, 4, 4, b, b, d, None) == -1                       # one volume for both answers
    assert L.tomo_branch_hist(a, 4, 4, 4, b, 8, c, d, e, f, 8, g, h, a, 8, j, None) == -1          # the histogram over the bits
    assert L.tomo_branch_hist(a, 4, 4, 4, b, 8, c, d, e, f, 8, g, h, j, 8, j, None) == -1          # ... over the other volume
    assert L.tomo_branch_attach(a, 4, 4, 4, b, 8, c, d, e, f, g, h, i, i, 8, 8, None) == -1        # one array for both answers
    assert L.tomo_branch_attach(a, 4, 4, 4, b, 8, c, d, e, f, g, h, a, j, 8, 8, None) == -1
    assert L.tomo_branch_attach(a, 4, 4, 4, b, 8, c, d, e, f, g, h, i, f, 8, 8, None) == -1
    assert L.tomo_branch_lookup(a, 4, 4, 4, b, 8, c, d, e, 8, f, 8, f, None) == -1                 # the labels over the queries
    assert L.tomo_branch_clear(a, 4, 4, 4, b, 8, c, d, e, f, 8, g, g, None) == -1                  # out == in
    assert L.tomo_branch_clear(a, 4, 4, 4, b, 8, c, d, e, f, 8, g, a, None) == -1                  # out over the tables' volume
    assert L.tomo_branch_clear(a, 4, 4, 4, b, 8, c, d, e, f, 9, g, h, None) == -1                  # more flags than runs


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(pipeline._lib, "lib", boom)
    monkeypatch.setattr(volume_calculator, "to_device_volume", boom)


def host_volume(shape=(3, 4, 70)):
    return pipeline.BitVolume(torch.zeros((shape[0], shape[1], (shape[2] + 63) // 64), dtype=torch.int64), shape)


def test_argument_errors(no_device):
    vol = host_volume()
    for bad in (vol.bits, np.zeros(vol.shape, dtype=bool), None):
        with pytest.raises(TypeError, match="BitVolume"):
            pipeline.skeleton_branches(bad)
        with pytest.raises(TypeError, match="BitVolume"):
            pipeline.prune_skeleton(bad, 1.0)
    for call in (lambda **k: pipeline.skeleton_branches(vol, **k), lambda **k: pipeline.prune_skeleton(vol, 1.0, **k)):
        for bad in (dict(slice_depths=np.ones(4)), dict(slice_depths=[1.0, -1.0, 1.0]), dict(mm_per_pixel_y=0.0),
                    dict(mm_per_pixel_x=float("inf"))):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(AssertionError, match="device"):                           # good arguments reach the device
            call(slice_depths=[0.5, 1.0, 2.0], mm_per_pixel_y=0.7, mm_per_pixel_x=0.9)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="min_voxels"):
            pipeline.skeleton_branches(vol, min_voxels=bad)
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="rounds"):
            pipeline.prune_skeleton(vol, 1.0, rounds=bad)
    with pytest.raises(ValueError, match="min_length_mm"):
        pipeline.prune_skeleton(vol, float("nan"))
    with pytest.raises(AssertionError, match="device"):
        pipeline.prune_skeleton(vol, 1.0, rounds=None)
    v = np.ones((3, 4, 5), dtype=bool)
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool)):
        with pytest.raises(TypeError, match="bool"):
            volume_calculator.skeleton_branch_report(bad, 0.9, 0.7, np.ones(3))
    with pytest.raises(ValueError, match="connectivity"):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(3), connectivity=18)
    with pytest.raises(ValueError, match="curve"):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(3), connectivity=6)
    with pytest.raises(ValueError, match="prune_mm"):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(3), prune_mm=-1.0)
    with pytest.raises(ValueError, match="rounds"):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(3), prune_rounds=-1)
    with pytest.raises(ValueError):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(4))
    with pytest.raises(AssertionError, match="device"):
        volume_calculator.skeleton_branch_report(v, 0.9, 0.7, np.ones(3), prune_mm=2.0, prune_rounds=None)


def test_signatures_and_defaults():
    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}

    assert names(pipeline.branch_steps) == ["slice_depths", "nz", "mm_per_pixel_y", "mm_per_pixel_x"]
    assert names(pipeline.skeleton_branches) == ["skel", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "min_voxels"]
    assert defaults(pipeline.skeleton_branches) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "min_voxels": 0}
    assert names(pipeline.prune_skeleton) == ["skel", "min_length_mm", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "rounds"]
    assert defaults(pipeline.prune_skeleton) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "rounds": 1}
    assert names(pipeline.ComponentRuns.label_at) == ["self", "indices"]
    assert [f for f in pipeline.SkeletonBranches.__dataclass_fields__] == [
        "branches", "nodes", "regular", "node_voxels", "voxels", "regular_voxels", "node_voxel_count", "isolated"]
    assert [f for f in pipeline.SkeletonBranchRows.__dataclass_fields__] == [
        "label", "voxels", "length_mm", "step_counts", "attach_index", "nodes", "chord_mm", "tortuosity", "kind"]
    assert [f for f in pipeline.SkeletonNodeRows.__dataclass_fields__] == [
        "label", "voxels", "end_voxels", "junction_voxels", "branches", "index_box", "centroid_index", "centroid_mm", "free_end"]
    assert [f for f in pipeline.PrunedSkeleton.__dataclass_fields__] == ["volume", "removed_branches", "removed_voxels", "rounds"]
    assert names(volume_calculator.skeleton_branch_report) == [
        "voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "connectivity", "curve", "prune_mm", "prune_rounds"]
    assert defaults(volume_calculator.skeleton_branch_report) == {"connectivity": 26, "curve": True, "prune_mm": 0.0, "prune_rounds": 1}
    assert "skeleton_branches" not in names(volume_calculator.component_properties)   # no flag there: its order is pinned
    empty = pipeline._empty_branch_rows()
    assert len(empty) == 0 and empty.step_counts.shape == (0, 7) and empty.attach_index.shape == (0, 2) and empty.kind.dtype == np.int64
    assert len(pipeline._empty_node_rows()) == 0 and pipeline._empty_node_rows().index_box.shape == (0, 6)


def test_the_host_arithmetic_of_the_rows():
    """_branch_rows_from on the reference's own downloads gives the reference's chord, tortuosity and kind, bit for bit."""
    for name, depths, mm_y, mm_x in (("thinned", None, 1.0, 1.0), ("lollipop", UNEVEN[:3], 0.7, 0.9), ("ring", None, 0.5, 0.25),
                                     ("noise10", UNEVEN[:7], 0.7, 0.9)):
        t = table(name, depths, mm_y, mm_x)
        b = t["branches"]
        zt, _, _ = pipeline.distance_positions(depths, fixtures()[name].shape[0], mm_y, mm_x)
        rows = pipeline._branch_rows_from(fixtures()[name].shape, zt[1:-1], mm_y, mm_x, b["voxels"], b["label"], b["length_mm"],
                                          b["step_counts"], b["attach_index"].copy(), t["attach_count"], b["nodes"], t["nodes"]["free_end"])
        assert rows.chord_mm.tobytes() == b["chord_mm"].tobytes() and rows.tortuosity.tobytes() == b["tortuosity"].tobytes()
        assert np.array_equal(rows.kind, b["kind"]) and rows.kind.dtype == np.int64


def test_the_round_limit_guards_the_host_loop():
    src = inspect.getsource(pipeline.prune_skeleton)
    assert "PRUNE_ROUND_LIMIT" in src and "TomoError" in src and pipeline.PRUNE_ROUND_LIMIT >= 1 << 10
