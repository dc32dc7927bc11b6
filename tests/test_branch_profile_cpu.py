"""CPU tier of the value profile along skeleton branches: the reference (tests/branch_profile_reference.py, NumPy scatter
reductions over label arrays) against an independent WALK that visits every branch voxel by voxel with Python floats, the
two-scale scene on which no fixed pruning length is right, the rounding rule of the fixed-point sum, and the plumbing (exports,
argument checks without a device, signatures).  None of it needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branch_profile_reference as P  # noqa: E402
import branches_reference as B  # noqa: E402
import skeleton_reference as S  # noqa: E402
import surface_reference as SR  # noqa: E402
import test_abi  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

NEW_SYMBOLS = ("tomo_profile_rows", "tomo_profile_stats", "tomo_profile_where")
SHAPE = (19, 21, 150)
LARGEST = np.array([P.ADMITTED - 1], dtype=np.uint32).view(np.float32)[0]             # 2^20 - 2^-4
_cache = {}


def memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def scene():
    """-> (the object, its curve skeleton, the distance map of the object), computed once."""
    def build():
        v = P.two_scale_scene()
        return v, S.skeleton(v, True, 26)[0], P.edt(v)
    return memo("scene", build)


def seeded_map(shape, seed, levels=None):
    """A float32 map of admitted values: uniform in [0, 40), or `levels` values only (ties everywhere)."""
    rng = np.random.default_rng(seed)
    if levels is None:
        return (rng.random(shape) * 40).astype(np.float32)
    return rng.integers(0, levels, shape).astype(np.float32) * np.float32(0.75)


# ------------------------------------------------------------------ the independent walk
def walk(vol, values):
    """-> the branches in the raster order of their first voxel: dicts with voxels, min, min_index, max, max_index, sum_q.  No
    label array and no NumPy reduction: neighbour lists, a flood per branch, Python comparisons and Python's round (half to even)."""
    vol = np.asarray(vol, dtype=bool)
    nz, ny, nx = vol.shape
    cells = set(map(tuple, np.argwhere(vol).tolist()))
    around = {p: [q for q in ((p[0] + dz, p[1] + dy, p[2] + dx) for dz, dy, dx in SR.STEPS) if q in cells] for p in cells}
    regular = {p for p in cells if len(around[p]) == 2}
    done, out = set(), []
    for start in sorted(regular):
        if start in done:
            continue
        branch, stack = [], [start]
        done.add(start)
        while stack:
            p = stack.pop()
            branch.append(p)
            for q in around[p]:
                if q in regular and q not in done:
                    done.add(q)
                    stack.append(q)
        row = {"voxels": len(branch), "sum_q": 0}
        for p in sorted(branch):                                                      # ascending flat index: a tie keeps the first
            v, at = float(values[p]), (p[0] * ny + p[1]) * nx + p[2]
            if "min" not in row or v < row["min"]:
                row["min"], row["min_index"] = v, at
            if "max" not in row or v > row["max"]:
                row["max"], row["max_index"] = v, at
            row["sum_q"] += round(v * 65536.0)
        out.append(row)
    return out


WALKED = {"noise10": lambda: S.noise(SHAPE, 0.1, 10), "plus": B.plus, "ypsilon": B.ypsilon, "ring": B.ring, "lollipop": B.lollipop}


@pytest.mark.parametrize("name", sorted(WALKED))
@pytest.mark.parametrize("levels", (None, 5))
def test_the_reference_agrees_with_the_walk(name, levels):
    vol = memo(("volume", name), WALKED[name])
    values = seeded_map(vol.shape, 3, levels)
    got = P.profile(vol, values, table=memo(("table", name), lambda: B.table(vol)))
    b, rows = got["branches"], walk(vol, values)
    assert len(rows) == len(b["label"]) > 0 and b["label"].tolist() == list(range(1, len(rows) + 1))
    for key in ("voxels", "min_index", "max_index", "sum_q"):
        assert b[key].dtype == np.int64 and b[key].tolist() == [r[key] for r in rows], (name, key)
    for key in ("min", "max"):
        assert b[key].dtype == np.float32 and b[key].tolist() == [r[key] for r in rows], (name, key)
    assert b["mean"].tolist() == [r["sum_q"] / 65536.0 / r["voxels"] for r in rows]
    flat = values.reshape(-1)
    assert np.array_equal(flat[b["min_index"]], b["min"]) and np.array_equal(flat[b["max_index"]], b["max"])
    assert (got["table"]["branch_labels"].reshape(-1)[b["min_index"]] == b["label"]).all()
    cycle = got["table"]["branches"]["kind"] == 0
    assert np.isnan(b["attach_value"][cycle]).all() and b["attach_value"].dtype == np.float32
    assert np.array_equal(b["attach_value"][~cycle], flat[got["table"]["branches"]["attach_index"][~cycle]])
    n = got["nodes"]
    labels = got["table"]["node_labels"]
    for i, c in enumerate(n["label"]):                                                # the nodes: a plain maximum per label
        inside = np.flatnonzero(labels.reshape(-1) == c)
        assert n["max"][i] == flat[inside].max() and n["max_index"][i] == inside[np.argmax(flat[inside])], (name, c)
    if levels and name == "noise10":                                                  # ties: the first index decides
        assert (b["min"] == b["max"])[b["voxels"] > 1].any()


def test_a_constant_map_reads_the_lowest_voxel_of_every_branch():
    vol = memo(("volume", "noise10"), WALKED["noise10"])
    t = memo(("table", "noise10"), lambda: B.table(vol))
    b = P.profile(vol, np.full(vol.shape, 2.5, dtype=np.float32), table=t)["branches"]
    first = np.array([np.flatnonzero(t["branch_labels"].reshape(-1) == c)[0] for c in b["label"]])
    assert np.array_equal(b["min_index"], first) and np.array_equal(b["max_index"], first)
    assert (b["min"] == 2.5).all() and (b["mean"] == 2.5).all() and np.array_equal(b["sum_q"], b["voxels"] * 163840)


def test_values_off_the_skeleton_are_never_read_and_bad_ones_on_it_are_refused():
    vol = B.ypsilon()
    good = seeded_map(vol.shape, 4)
    want = P.profile(vol, good)["branches"]
    for poison in (np.nan, -1.0, np.inf, -0.0):
        values = np.where(vol, good, np.float32(poison)).astype(np.float32)
        got = P.profile(vol, values)["branches"]
        assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in want), poison
        for at in (np.argwhere(B.split(vol)[0])[0], np.argwhere(B.split(vol)[1])[0]):  # on a regular voxel, on a node voxel
            values = good.copy()
            values[tuple(at)] = poison
            with pytest.raises(ValueError):
                P.profile(vol, values)


# ------------------------------------------------------------------ the rounding rule
def test_the_rounding_rule_of_the_fixed_point_sum():
    half = 2.0 ** -17
    assert P.quantum(np.float32(0.0)) == 0 and P.quantum(np.float32(2.0 ** -16)) == 1
    for k in (0, 1, 2, 3, 6, 7, 1000, 1001, 65534, 65535):                            # a tie goes to the even neighbour
        v = np.float32(k * 2.0 ** -16 + half)
        assert float(v) == k * 2.0 ** -16 + half                                      # the float32 holds the tie exactly
        assert P.quantum(v) == (k if k % 2 == 0 else k + 1), k
    assert float(LARGEST) == 2.0 ** 20 - 2.0 ** -4 and P.quantum(LARGEST) == 2 ** 36 - 2 ** 12
    assert P.quantum(LARGEST) * 2 ** 27 < 2 ** 63                                     # a branch of 2^27 voxels cannot overflow
    assert P.admitted(np.array([0.0, 2.0 ** -149, 1.0, LARGEST], dtype=np.float32)).all()
    assert not P.admitted(np.array([-0.0, -1.0, 2.0 ** 20, np.inf, -np.inf, np.nan], dtype=np.float32)).any()
    assert pipeline.PROFILE_ADMITTED == P.ADMITTED == 0x49800000
    vol = B.bar((1, 1, 12), (0, 0, 0), (0, 0, 1), 12)                                  # ten regular voxels between two ends
    values = np.zeros(vol.shape, dtype=np.float32)
    values[0, 0, 1:11] = [k * 2.0 ** -16 + half for k in (0, 1, 2, 3, 4, 5)] + [0.0, LARGEST, 1.0, 2.0 ** -16]
    b = P.profile(vol, values)["branches"]
    assert b["sum_q"].tolist() == [(0 + 2 + 2 + 4 + 4 + 6) + 0 + (2 ** 36 - 2 ** 12) + 65536 + 1] and b["voxels"].tolist() == [10]
    assert b["min"].tolist() == [0.0] and b["min_index"].tolist() == [7] and b["max"].tolist() == [float(LARGEST)]
    assert b["max_index"].tolist() == [8] and b["mean"][0] == (b["sum_q"][0] / 65536.0) / 10
    rows = pipeline._profile_rows_from(np.array([[1, 10, 0, P.ADMITTED - 1, b["sum_q"][0], 7, 8]], dtype=np.int64))
    assert rows.mean.tobytes() == b["mean"].tobytes() and rows.max.tobytes() == b["max"].tobytes() and rows.min.tolist() == [0.0]


def test_the_host_arithmetic_of_the_rows():
    """_profile_rows_from / _node_value_rows_from on the reference's own integers give the reference's floats, bit for bit."""
    _, skel, dist = scene()
    ref = P.profile(skel, dist)
    b, n = ref["branches"], ref["nodes"]
    raw = np.stack([b["label"], b["voxels"], b["min"].view(np.uint32).astype(np.int64), b["max"].view(np.uint32).astype(np.int64),
                    b["sum_q"], b["min_index"], b["max_index"]], axis=1)
    rows = pipeline._profile_rows_from(raw, b["attach_value"])
    for key in ("label", "voxels", "min_index", "max_index", "sum_q"):
        assert getattr(rows, key).dtype == np.int64 and np.array_equal(getattr(rows, key), b[key]), key
    for key, dtype in (("min", np.float32), ("max", np.float32), ("mean", np.float64), ("attach_value", np.float32)):
        assert getattr(rows, key).dtype == dtype and getattr(rows, key).tobytes() == b[key].tobytes(), key
    raw = np.stack([n["label"], n["label"], n["max"].view(np.uint32).astype(np.int64), n["max_index"]], axis=1)
    rows = pipeline._node_value_rows_from(raw)
    assert rows.max.tobytes() == n["max"].tobytes() and np.array_equal(rows.max_index, n["max_index"]) and len(rows) == len(n["label"])
    empty = pipeline._profile_rows_from(np.zeros((0, 7)))
    assert len(empty) == 0 and empty.attach_value.shape == (0, 2) and empty.min.dtype == np.float32 and empty.mean.dtype == np.float64
    assert len(pipeline._node_value_rows_from(np.zeros((0, 4)))) == 0


# ------------------------------------------------------------------ the two-scale scene
def spurs(skel):
    b = B.table(skel)["branches"]
    return sorted(b["length_mm"][b["kind"] == 2].tolist()), len(b["label"])


def test_no_fixed_length_prunes_the_two_scale_scene():
    v, skel, _ = scene()
    assert skel.sum() == 79 and spurs(skel) == ([2.0, 2.0] + [7.0] * 6 + [16.0], 9) and all(skel[p] for p in P.SCENE_TIPS)
    for least in (2.0, 2.5, 5.0, 7.0):                                                # the five spurs of the big ball stay
        out = B.prune(skel, least, rounds=None)[0]
        assert spurs(out)[0] == ([2.0, 2.0] if least <= 2.0 else []) + [7.0] * 6 + [16.0], least
        assert all(out[p] for p in P.SCENE_TIPS)
    for least in (7.5, 8.0, 12.0):                                                    # ... and go only together with the small ball's arm
        out = B.prune(skel, least, rounds=None)[0]
        assert not out[:, :, 66].any() and out[P.SCENE_TIPS[0]], least


@pytest.mark.parametrize("factor", (1.0, 1.25))
def test_relative_pruning_leaves_the_two_arms(factor):
    v, skel, dist = scene()
    before = T.volume(T.components(skel, 26)[2])
    for rounds in (1, 2, None):
        out, nb, nv, done = P.prune_relative(skel, dist, factor, rounds=rounds)
        assert (nb, nv, done) == (7, 39, 1) and out.sum() == 40 and not (out & ~skel).any()
        assert spurs(out) == ([7.0, 16.0], 2) and all(out[p] for p in P.SCENE_TIPS)
        assert T.volume(T.components(out, 26)[2]) == before
    assert P.prune_relative(skel, dist, factor, rounds=0)[1:] == (0, 0, 0)


def test_relative_pruning_below_the_radius_and_without_a_factor():
    v, skel, dist = scene()
    out, nb, nv, done = P.prune_relative(skel, dist, 0.75)
    assert (nb, nv, done) == (0, 0, 0) and np.array_equal(out, skel)
    for least in (2.5, 8.0):                                                          # factor 0: the absolute rule
        assert all(np.array_equal(a, b) for a, b in zip(P.prune_relative(skel, dist, 0.0, least), B.prune(skel, least, rounds=None)))
    got = P.prune_relative(skel, dist, 0.75, 2.5)                                     # the larger of the two thresholds
    assert got[1:] == (2, 4, 1) and spurs(got[0])[0] == [7.0] * 6 + [16.0]
    noise = S.noise(SHAPE, 0.1, 10)
    values = seeded_map(SHAPE, 8)
    before = T.volume(T.components(noise, 26)[2])
    out, nb, nv, done = P.prune_relative(noise, values, 0.2)
    assert nb > 0 and done >= 1 and noise.sum() - out.sum() == nv and T.volume(T.components(out, 26)[2]) == before


# ------------------------------------------------------------------ the library without a GPU
def test_new_symbols_are_declared_and_bound():
    L = _lib.lib()
    assert L.tomo_abi_version() == 9
    syms = test_abi.header_symbols()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("tomo_profile_")) == sorted(NEW_SYMBOLS)
    assert sorted(s for s in syms if s.startswith("tomo_profile_")) == sorted(NEW_SYMBOLS)
    assert {"components_profile", "branch_profile", "prune_relative"} <= set(pipeline.COUNTERS)
    assert (pipeline.PROFILE_COLUMNS, pipeline.PROFILE_F_VALUE) == (7, 8)


def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(12)]
    a, b, c, d, e, f, g, h, i, j, k, m = (ctypes.addressof(x) for x in bufs)          # distinct host buffers, never dereferenced
    big = (1 << 12, 1 << 13, 1 << 12)                                                 # 2^31 words
    shapes = ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4))
    calls = {                                                                         # name: (good arguments, pointers, sizes)
        "tomo_profile_stats": ([a, 4, 4, 4, b, 8, c, d, e, f, g, h, i, 8], (0, 4, 6, 7, 8, 9, 10, 11, 12), (5, 13)),
        "tomo_profile_where": ([a, 4, 4, 4, b, 8, c, d, e, f, g, h, i, j, 8], (0, 4, 6, 7, 8, 9, 10, 11, 12, 13), (5, 14)),
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
            args = list(good)
            args[at] = 1 << 31
            assert fn(*args, None) == -3, (name, at)
    outputs = {"tomo_profile_stats": (10, 11, 12), "tomo_profile_where": (10, 11, 12, 13)}
    for name, outs in outputs.items():                                                # any two of the arrays, or one over the bits / the map
        good = calls[name][0]
        for x in outs:
            for y in (0, 9) + tuple(o for o in outs if o < x):
                args = list(good)
                args[x] = good[y]
                assert getattr(L, name)(*args, None) == -1, (name, x, y)
    rows = [a, b, c, d, e, f, 8, g, h, i, j, 8]                                       # table, lo, hi, sum, lo_first, hi_first, cap, tot, sel, slot, out, cap_sel
    for at in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10):
        args = list(rows)
        args[at] = None
        assert L.tomo_profile_rows(*args, None) == -1, at
    for at in (6, 11):
        for bad in (0, -1):
            args = list(rows)
            args[at] = bad
            assert L.tomo_profile_rows(*args, None) == -1, at
        args = list(rows)
        args[at] = 1 << 31
        assert L.tomo_profile_rows(*args, None) == -3, at
    for x in (1, 2, 3, 4, 5, 10):                                                     # the five arrays and the rows: no two are one
        for y in (0,) + tuple(o for o in (1, 2, 3, 4, 5) if o < x):
            args = list(rows)
            args[x] = rows[y]
            assert L.tomo_profile_rows(*args, None) == -1, (x, y)


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
    values = torch.zeros(vol.shape, dtype=torch.float32)
    calls = (lambda s=vol, v=values, **k: pipeline.skeleton_branch_profile(s, v, **k),
             lambda s=vol, v=values, **k: pipeline.prune_skeleton_relative(s, v, **k))
    for call in calls:
        for bad in (vol.bits, np.zeros(vol.shape, dtype=bool), None):
            with pytest.raises(TypeError, match="BitVolume"):
                call(s=bad)
        for bad in (None, np.zeros(vol.shape, dtype=np.float32), values.double(), values.to(torch.int32)):
            with pytest.raises(TypeError, match="float32"):
                call(v=bad)
        for bad in (values[:2], values.reshape(4, 3, 70), values[0]):
            with pytest.raises(ValueError, match="shape"):
                call(v=bad)
        with pytest.raises(ValueError, match="device"):
            call(v=torch.zeros(vol.shape, dtype=torch.float32, device="meta"))
        for bad in (dict(slice_depths=np.ones(4)), dict(slice_depths=[1.0, -1.0, 1.0]), dict(mm_per_pixel_y=0.0),
                    dict(mm_per_pixel_x=float("inf"))):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(AssertionError, match="device"):                           # good arguments reach the device
            call(slice_depths=[0.5, 1.0, 2.0], mm_per_pixel_y=0.7, mm_per_pixel_x=0.9)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="min_voxels"):
            pipeline.skeleton_branch_profile(vol, values, min_voxels=bad)
    for bad in (-1.0, float("nan"), -1e-300, "1", None, True):
        with pytest.raises(ValueError, match="factor"):
            pipeline.prune_skeleton_relative(vol, values, bad)
    with pytest.raises(ValueError, match="min_length_mm"):
        pipeline.prune_skeleton_relative(vol, values, 1.0, float("nan"))
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="rounds"):
            pipeline.prune_skeleton_relative(vol, values, rounds=bad)
    for good in (dict(factor=0), dict(factor=0.0, min_length_mm=3.0), dict(factor=float("inf")), dict(rounds=3)):
        with pytest.raises(AssertionError, match="device"):
            pipeline.prune_skeleton_relative(vol, values, **good)
    v = np.ones((3, 4, 5), dtype=bool)
    report = volume_calculator.skeleton_thickness_report
    for bad in (np.ones((3, 4, 5), dtype=np.uint8), np.ones((4, 5), dtype=bool)):
        with pytest.raises(TypeError, match="bool"):
            report(bad, 0.9, 0.7, np.ones(3))
    with pytest.raises(ValueError, match="connectivity"):
        report(v, 0.9, 0.7, np.ones(3), connectivity=18)
    with pytest.raises(ValueError, match="curve"):
        report(v, 0.9, 0.7, np.ones(3), connectivity=6)
    with pytest.raises(ValueError, match="prune_mm"):
        report(v, 0.9, 0.7, np.ones(3), prune_mm=-1.0)
    with pytest.raises(ValueError, match="rounds"):
        report(v, 0.9, 0.7, np.ones(3), prune_rounds=-1)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="factor"):
            report(v, 0.9, 0.7, np.ones(3), prune_factor=bad)
    with pytest.raises(ValueError):
        report(v, 0.9, 0.7, np.ones(4))
    with pytest.raises(AssertionError, match="device"):
        report(v, 0.9, 0.7, np.ones(3), prune_factor=1.25, prune_mm=2.0, prune_rounds=2)


def test_signatures_and_defaults():
    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}

    assert names(pipeline.ComponentRuns.value_profile) == ["self", "values", "min_voxels"]
    assert defaults(pipeline.ComponentRuns.value_profile) == {"min_voxels": 0}
    assert names(pipeline.skeleton_branch_profile) == ["skel", "values", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "min_voxels"]
    assert defaults(pipeline.skeleton_branch_profile) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "min_voxels": 0}
    assert names(pipeline.prune_skeleton_relative) == ["skel", "values", "factor", "min_length_mm", "slice_depths", "mm_per_pixel_y",
                                                       "mm_per_pixel_x", "rounds"]
    assert defaults(pipeline.prune_skeleton_relative) == {"factor": 1.0, "min_length_mm": 0.0, "slice_depths": None, "mm_per_pixel_y": 1.0,
                                                          "mm_per_pixel_x": 1.0, "rounds": None}
    assert [f for f in pipeline.SkeletonProfile.__dataclass_fields__] == ["table", "branches", "nodes"]
    assert [f for f in pipeline.BranchValueRows.__dataclass_fields__] == [
        "label", "voxels", "min", "min_index", "max", "max_index", "sum_q", "mean", "attach_value"]
    assert [f for f in pipeline.NodeValueRows.__dataclass_fields__] == ["label", "max", "max_index"]
    assert names(volume_calculator.skeleton_thickness_report) == [
        "voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "connectivity", "curve", "prune_factor", "prune_mm", "prune_rounds"]
    assert defaults(volume_calculator.skeleton_thickness_report) == {"connectivity": 26, "curve": True, "prune_factor": 1.0, "prune_mm": 0.0,
                                                                     "prune_rounds": None}
    # what was there before keeps its shape
    assert names(pipeline.prune_skeleton) == ["skel", "min_length_mm", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "rounds"]
    assert [f for f in pipeline.PrunedSkeleton.__dataclass_fields__] == ["volume", "removed_branches", "removed_voxels", "rounds"]
    assert "rule" in names(pipeline._prune) and "_prune(" in inspect.getsource(pipeline.prune_skeleton)
    assert "_prune(" in inspect.getsource(pipeline.prune_skeleton_relative)           # one loop behind both rules
