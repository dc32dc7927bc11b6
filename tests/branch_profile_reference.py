"""Host reference for a value along the branches of a skeleton (include/tomo_hip.h, "A value along the components of a labelled
volume"): the definition restated in NumPy on the label arrays of branches_reference.table, for small dense arrays.

stats():           per label the smallest and the largest float32 bit pattern (np.minimum.at / np.maximum.at on the uint32 views),
                   the lowest flat index that attains each (a masked arg-min over flat indices) and sum_q, the int64 sum of
                   np.rint(float64(v) * 65536) (np.add.at).
profile():         stats over the branch labels and the node labels, in the rows of the table.
prune_relative():  pruning with the threshold max(min_length_mm, factor * values[the attached voxel of the node that stays]).
two_scale_scene(): the acceptance scene: two balls of two sizes, each with a real arm."""
import numpy as np

import branches_reference as B
import edt_reference as E
import skeleton_reference as S

ADMITTED = 0x49800000                # float32 bit patterns below it: 0.0 <= v < 2^20, finite, not -0.0
FAR = np.iinfo(np.int64).max


def admitted(values):
    return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32) < ADMITTED


def quantum(values):
    """q(v) = rint(float64(v) * 2^16) as int64: the product is exact, the rounding is half to even."""
    return np.rint(np.asarray(values, dtype=np.float32).astype(np.float64) * 65536.0).astype(np.int64)


def stats(labels, n, values):
    """-> dict of arrays over the labels 1 .. n: voxels, min, max (float32), min_index, max_index, sum_q, mean."""
    labels = np.asarray(labels)
    values = np.ascontiguousarray(values, dtype=np.float32)
    flat = np.flatnonzero(labels.reshape(-1) > 0).astype(np.int64)
    c = labels.reshape(-1)[flat].astype(np.int64) - 1
    bits = values.reshape(-1).view(np.uint32)[flat]
    if (bits >= ADMITTED).any():
        raise ValueError("a labelled voxel holds a value that is not admitted")
    lo, hi = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    np.minimum.at(lo, c, bits)
    np.maximum.at(hi, c, bits)
    lo_at, hi_at = np.full(n, FAR, dtype=np.int64), np.full(n, FAR, dtype=np.int64)
    np.minimum.at(lo_at, c, np.where(bits == lo[c], flat, FAR))
    np.minimum.at(hi_at, c, np.where(bits == hi[c], flat, FAR))
    total = np.zeros(n, dtype=np.int64)
    np.add.at(total, c, quantum(values.reshape(-1)[flat]))
    voxels = np.bincount(c, minlength=n).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (total.astype(np.float64) / 65536.0) / voxels.astype(np.float64)
    return {"voxels": voxels, "min": lo.view(np.float32), "max": hi.view(np.float32), "min_index": lo_at, "max_index": hi_at,
            "sum_q": total, "mean": mean}


def values_at(values, index):
    """The entries at flat indices, NaN where the index is negative -> float32 of the shape of index."""
    index = np.asarray(index, dtype=np.int64)
    flat = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    return np.where(index < 0, np.float32(np.nan), flat[np.where(index < 0, 0, index)]).astype(np.float32)


def profile(vol, values, slice_depths=None, mm_y=1.0, mm_x=1.0, min_voxels=0, table=None):
    """-> dict: table (branches_reference.table's), branches and nodes (dicts of arrays that line up with the table's rows)."""
    t = B.table(vol, slice_depths, mm_y, mm_x, min_voxels) if table is None else table
    vol = np.asarray(vol, dtype=bool)
    if not admitted(values)[vol].all():
        raise ValueError("a set voxel holds a value that is not admitted")
    nb, nn = int(t["branch_labels"].max()) if t["regular_voxels"] else 0, len(t["nodes"]["label"])
    s = stats(t["branch_labels"], nb, values)
    pick = t["branches"]["label"] - 1
    branches = {k: v[pick] for k, v in s.items()}
    branches["label"] = t["branches"]["label"].copy()
    branches["attach_value"] = values_at(values, t["branches"]["attach_index"])
    assert np.array_equal(branches["voxels"], t["branches"]["voxels"])
    s = stats(t["node_labels"], nn, values)
    nodes = {"label": t["nodes"]["label"].copy(), "max": s["max"], "max_index": s["max_index"]}
    return {"table": t, "branches": branches, "nodes": nodes}


def prune_relative_round(vol, values, factor=1.0, min_length_mm=0.0, slice_depths=None, mm_y=1.0, mm_x=1.0):
    """One round -> (the pruned volume, removed branches, removed voxels): every branch of kind 2 with length_mm <
    max(min_length_mm, factor * r) goes, with the free-end voxel it hangs from; r = the float64 of the value at the attached
    voxel of the node that is not the free end."""
    vol = np.asarray(vol, dtype=bool)
    t = B.table(vol, slice_depths, mm_y, mm_x)
    b = t["branches"]
    free = np.concatenate([[False], t["nodes"]["free_end"]])
    gone = np.zeros(len(b["label"]), dtype=bool)
    for i in np.flatnonzero(b["kind"] == 2):
        a0, a1 = b["attach_index"][i]
        held = a1 if free[b["nodes"][i][0]] else a0
        r = float(np.asarray(values, dtype=np.float32).reshape(-1)[held])
        gone[i] = b["length_mm"][i] < np.maximum(float(min_length_mm), float(factor) * r)
    out = vol.copy()
    if gone.any():
        out &= ~np.isin(t["branch_labels"], b["label"][gone])
        ends = b["nodes"][gone]
        ends = ends[free[ends]]
        out &= ~np.isin(t["node_labels"], ends)
    return out, int(gone.sum()), int(vol.sum() - out.sum())


def prune_relative(vol, values, factor=1.0, min_length_mm=0.0, slice_depths=None, mm_y=1.0, mm_x=1.0, rounds=None):
    """-> (volume, removed branches, removed voxels, the rounds that removed something); rounds=None: to the fixed point."""
    vol = np.asarray(vol, dtype=bool)
    branches = voxels = done = 0
    while rounds is None or done < rounds:
        vol, nb, nv = prune_relative_round(vol, values, factor, min_length_mm, slice_depths, mm_y, mm_x)
        if nb == 0:
            break
        branches, voxels, done = branches + nb, voxels + nv, done + 1
    return vol, branches, voxels, done


# ------------------------------------------------------------------------------------------------ the two-scale scene
SCENE_SHAPE = (24, 26, 80)
SCENE_TIPS = ((12, 12, 31), (12, 12, 66))            # the far ends of the two real arms


def two_scale_scene():
    """A ball of radius 9.3 with a 3 x 3 arm and a ball of radius 3.3 with a one-voxel arm: the spurs of the big ball are as long
    as the small ball's real arm, so no fixed length prunes it right."""
    v = S.ball(SCENE_SHAPE, (12, 12, 14), 9.3) | S.ball(SCENE_SHAPE, (12, 12, 58), 3.3)
    v[11:14, 11:14, 14:32] = True
    v[12, 12, 58:67] = True
    return v


def edt(vol, slice_depths=None, mm_y=1.0, mm_x=1.0):
    """The inside distance of a volume in mm, everything outside the stack background -> float32: distance_transform's
    definition, by edt_reference's exhaustive passes."""
    vol = np.asarray(vol, dtype=bool)
    return E.edt(vol, *E.positions(vol.shape, slice_depths, mm_y, mm_x))
