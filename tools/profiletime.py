#!/usr/bin/env python3
"""The value profile along skeleton branches at n^3 (default 512), resident, on the two volumes of tools/branchtime.py: the
curve skeleton (pipeline.skeleton) of the benchmark's ellipsoid with a few hundred spherical pores, profiled with the distance
map of that OBJECT, and seeded noise at 50 %, used raw with its own distance map.  For each volume, in ONE run
  * the kernels on the run tables of the regular voxels, labelled once: tomo_profile_stats and tomo_profile_where, and next to
    them the yardstick, tomo_cc_value_max and tomo_cc_value_first on the same tables and the same map.  The four are timed in
    --rounds alternating rounds, so a drift of the machine lands on both sides; `ratio` = (stats + where) / (max + first) of
    the medians over all rounds.  The pair reads the same words and values and sends one atomic per run where the new passes
    send up to three and two;
  * the whole calls, host reads included: pipeline.skeleton_branch_profile next to pipeline.skeleton_branches, and
    pipeline.prune_skeleton_relative (--factor, to the fixed point) next to pipeline.prune_skeleton (--prune-mm, to the fixed
    point), both under unit spacing.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/profiletime.py [--n 512] [--warmup 1] [--reps 3] [--rounds 3] [--volumes skeleton noise] [--out t.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cavitytime import porous_ellipsoid, timed  # noqa: E402
from zonetime import counted  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

KEYS = ("prune_rounds", "branch_clear", "components_label", "components_profile", "components_value")
KERNELS = ("tomo_profile_stats", "tomo_profile_where", "tomo_cc_value_max", "tomo_cc_value_first")


def kernels(skel, values, warmup, reps, rounds):
    """Event times of the two new passes and of the value-kernel pair on the tables of the regular voxels of one split."""
    L, dev, st = _lib.lib(), skel.device, _stream()
    t = pipeline.skeleton_branches(skel)
    out = {"regular_voxels": t.regular_voxels, "branches": len(t.branches), "nodes": len(t.nodes)}
    if t.regular_voxels == 0:
        return out
    runs = pipeline.ComponentRuns(t.regular, 26)
    n = runs._checked()
    out["runs"] = runs.runs
    lo, hi, best = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    total, lo_first, hi_first, first = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
    head = (_p(runs.bits), *skel.shape, *runs._tables(), _p(runs.tot))
    calls = {
        "tomo_profile_stats": lambda: _lib.check(L.tomo_profile_stats(*head, _p(values), _p(lo), _p(hi), _p(total), n, st), "tomo_profile_stats"),
        "tomo_profile_where": lambda: _lib.check(L.tomo_profile_where(*head, _p(values), _p(lo), _p(hi), _p(lo_first), _p(hi_first), n, st),
                                                 "tomo_profile_where"),
        "tomo_cc_value_max": lambda: _lib.check(L.tomo_cc_value_max(*head, _p(values), None, _p(best), n, st), "tomo_cc_value_max"),
        "tomo_cc_value_first": lambda: _lib.check(L.tomo_cc_value_first(*head, _p(values), None, _p(best), _p(first), n, st),
                                                  "tomo_cc_value_first"),
    }
    medians = {k: [] for k in KERNELS}
    for _ in range(rounds):                                                           # stats before where, max before first: each
        for k in KERNELS:                                                             # second pass reads what the first one left
            medians[k].append(timed(calls[k], warmup, reps))
    for k in KERNELS:
        out[k] = {"median_ms": round(float(np.median([m["median_ms"] for m in medians[k]])), 3),
                  "min_ms": min(m["min_ms"] for m in medians[k]), "max_ms": max(m["max_ms"] for m in medians[k])}
    new = out["tomo_profile_stats"]["median_ms"] + out["tomo_profile_where"]["median_ms"]
    pair = out["tomo_cc_value_max"]["median_ms"] + out["tomo_cc_value_first"]["median_ms"]
    out["ratio"] = round(new / pair, 3)
    runs._checked()
    assert torch.equal(hi, best) and torch.equal(hi_first, first)                     # both sides found the same maxima
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--prune-mm", type=float, default=4.0)
    ap.add_argument("--factor", type=float, default=1.0)
    ap.add_argument("--volumes", nargs="+", default=["skeleton", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("profiletime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)

    def skeleton():
        solid = pipeline.pack(porous_ellipsoid(n, a.pores, dev))
        return pipeline.skeleton(solid), pipeline.distance_transform(solid)

    def noise():
        vol = pipeline.pack((torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))
        return vol, pipeline.distance_transform(vol)

    rows = []
    for name in a.volumes:
        vol, values = {"skeleton": skeleton, "noise": noise}[name]()
        torch.cuda.empty_cache()
        row = {"n": n, "volume": name, "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(kernels(vol, values, a.warmup, a.reps, a.rounds))
        row["skeleton_branches"] = counted(lambda: pipeline.skeleton_branches(vol), a.warmup, a.reps, KEYS)
        row["skeleton_branch_profile"] = counted(lambda: pipeline.skeleton_branch_profile(vol, values), a.warmup, a.reps, KEYS)
        row["prune_skeleton"] = counted(lambda: pipeline.prune_skeleton(vol, a.prune_mm, rounds=None), a.warmup, a.reps, KEYS)
        p = pipeline.prune_skeleton(vol, a.prune_mm, rounds=None)
        row["prune_skeleton"].update(removed_branches=p.removed_branches, removed_voxels=p.removed_voxels, rounds=p.rounds)
        row["prune_skeleton_relative"] = counted(lambda: pipeline.prune_skeleton_relative(vol, values, a.factor), a.warmup, a.reps, KEYS)
        p = pipeline.prune_skeleton_relative(vol, values, a.factor)
        row["prune_skeleton_relative"].update(removed_branches=p.removed_branches, removed_voxels=p.removed_voxels, rounds=p.rounds)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del vol, values
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
