#!/usr/bin/env python3
"""The branch table of a skeleton at n^3 (default 512), resident as BitVolumes, on two volumes: the curve skeleton
(pipeline.skeleton) of the benchmark's ellipsoid with a few hundred spherical pores (tools/cavitytime.py), and seeded noise at
50 %, used raw -- nearly all of it node voxels.  For each volume, in ONE run
  * the entry points on their own, on the state pipeline.skeleton_branches builds: tomo_branch_split, tomo_branch_hist and
    tomo_branch_attach over the tables of the regular voxels, tomo_branch_lookup for the attached voxels, tomo_branch_clear with
    the flags of one pruning round -- and, on the same volume and the same tables, the passes they are shaped after:
    tomo_thin_nodes (for the split) and tomo_cc_surface_hist (for the histogram);
  * the whole calls, host reads included: pipeline.skeleton_branches, pipeline.prune_skeleton with rounds=1 and rounds=None
    (--prune-mm, unit spacing), and pipeline.skeleton_nodes as the scale.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/branchtime.py [--n 512] [--warmup 1] [--reps 3] [--volumes skeleton noise] [--out t.json]
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

KEYS = ("prune_rounds", "branch_clear", "components_label")


def entry_points(vol, prune_mm, warmup, reps):
    """Event times of the entry points on the state of one skeleton_branches call."""
    L, dev, st = _lib.lib(), vol.device, _stream()
    shape = vol.shape
    bits = vol.bits.contiguous()
    out = {}
    regular, nodes = torch.empty_like(bits), torch.empty_like(bits)
    ends, junctions = torch.empty_like(bits), torch.empty_like(bits)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    out["tomo_branch_split"] = timed(lambda: _lib.check(L.tomo_branch_split(_p(bits), *shape, _p(regular), _p(nodes), _p(counters), st),
                                                        "tomo_branch_split"), warmup, reps)
    out["tomo_thin_nodes"] = timed(lambda: _lib.check(L.tomo_thin_nodes(_p(bits), *shape, _p(ends), _p(junctions), _p(counters), st),
                                                      "tomo_thin_nodes"), warmup, reps)
    t = pipeline.skeleton_branches(vol)
    out["table"] = {"voxels": t.voxels, "regular_voxels": t.regular_voxels, "node_voxels": t.node_voxel_count, "isolated": t.isolated,
                    "branches": len(t.branches), "nodes": len(t.nodes), "kinds": np.bincount(t.branches.kind, minlength=4).tolist(),
                    "free_ends": int(t.nodes.free_end.sum()), "total_length_mm": float(t.branches.length_mm.sum())}
    if t.regular_voxels == 0:
        return out
    runs = pipeline.ComponentRuns(t.regular, 26)
    picked = runs.select()
    out["tables"] = {"runs": runs.runs, "branches": picked.m, "slice_entries": picked.total}
    hist = torch.empty(pipeline.SURFACE_COUNTERS * picked.total, dtype=torch.int64, device=dev)
    head = runs.hist_head(picked)
    out["tomo_branch_hist"] = timed(lambda: _lib.check(L.tomo_branch_hist(*head, _p(hist), picked.total, _p(bits), st),
                                                       "tomo_branch_hist"), warmup, reps)
    out["tomo_cc_surface_hist"] = timed(lambda: _lib.check(L.tomo_cc_surface_hist(*head, _p(hist), picked.total, st),
                                                           "tomo_cc_surface_hist"), warmup, reps)
    attach = torch.empty((picked.m, 2), dtype=torch.int64, device=dev)
    count = torch.empty(picked.m, dtype=torch.int64, device=dev)
    out["tomo_branch_attach"] = timed(lambda: _lib.check(L.tomo_branch_attach(_p(runs.bits), *shape, *runs._tables(), _p(runs.tot), _p(bits),
                                                                              _p(picked.sel), _p(picked.slot), _p(attach), _p(count),
                                                                              picked.table.shape[0], picked.m, st), "tomo_branch_attach"),
                                      warmup, reps)
    if t.node_voxel_count:
        nruns = pipeline.ComponentRuns(t.node_voxels, 26)
        q = torch.from_numpy(t.branches.attach_index).to(dev)
        out["tomo_branch_lookup"] = dict(timed(lambda: nruns.label_at(q), warmup, reps), queries=int(q.numel()))
    gone = (t.branches.kind == 2) & (t.branches.length_mm < prune_mm)
    flags = np.zeros(runs.n, dtype=np.uint8)
    flags[t.branches.label[gone] - 1] = 1
    flagged, cleared = torch.from_numpy(flags).to(dev), torch.empty_like(bits)
    out["tomo_branch_clear"] = dict(timed(lambda: _lib.check(L.tomo_branch_clear(_p(runs.bits), *shape, *runs._tables(), _p(runs.tot),
                                                                                 _p(flagged), runs.n, _p(bits), _p(cleared), st),
                                                             "tomo_branch_clear"), warmup, reps), flagged=int(gone.sum()))
    runs._checked()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--prune-mm", type=float, default=4.0)
    ap.add_argument("--volumes", nargs="+", default=["skeleton", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("branchtime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"skeleton": lambda: pipeline.skeleton(pipeline.pack(porous_ellipsoid(n, a.pores, dev))),
               "noise": lambda: pipeline.pack((torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name in a.volumes:
        vol = volumes[name]()
        torch.cuda.empty_cache()
        row = {"n": n, "volume": name, "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(entry_points(vol, a.prune_mm, a.warmup, a.reps))
        row["skeleton_nodes"] = timed(lambda: pipeline.skeleton_nodes(vol), a.warmup, a.reps)
        row["skeleton_branches"] = counted(lambda: pipeline.skeleton_branches(vol), a.warmup, a.reps, KEYS)
        for rounds in (1, None):
            key = "prune_skeleton_rounds_%s" % rounds
            row[key] = counted(lambda: pipeline.prune_skeleton(vol, a.prune_mm, rounds=rounds), a.warmup, a.reps, KEYS)
            p = pipeline.prune_skeleton(vol, a.prune_mm, rounds=rounds)
            row[key].update(removed_branches=p.removed_branches, removed_voxels=p.removed_voxels, rounds=p.rounds)
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
        del vol
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
