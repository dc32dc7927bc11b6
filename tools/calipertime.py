#!/usr/bin/env python3
"""Caliper (Feret) diameters per component at n^3 (default 512), unit spacing, on the two volumes of tools/cavitytime.py,
resident as BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores -- one solid body -- and seeded noise at
50 % -- millions of components, of which those of at least --noise-min-voxels voxels are selected (the extremes of ALL of them
along 64 directions are over COMPONENT_HIST_BUDGET).  HIP events around warmed-up repeats, median / min / max, of
  * the passes on their own, on run tables labelled and selected once: tomo_cc_caliper with the 64 default directions under
    both extents (8 batches of 8 directions in one launch) and with 8 directions (one batch), tomo_cc_caliper_axes along the
    components' own principal axes, and tomo_cc_caliper_rows;
  * tomo_cc_measure on the same tables in the same run, as context: the row pass every per-component number starts from;
  * the whole of pipeline.component_caliper without and with oriented (labelling, selection, moments, host reads and the
    download included, as a caller pays them), next to pipeline.component_properties and component_moments.
There is no time bar: the parent commit has no such path.

    python tools/calipertime.py [--n 512] [--warmup 1] [--reps 5] [--noise-min-voxels 8] [--out t.json]
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
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402


def passes(vol, conn, min_voxels, warmup, reps):
    """Event times of the caliper passes and of tomo_cc_measure on tables labelled and selected once."""
    L, dev, st = _lib.lib(), vol.device, _stream()
    nz, ny, nx = vol.shape
    runs = pipeline.ComponentRuns(vol, conn)
    picked = runs.select(min_voxels)
    out = {"runs": runs.runs, "components": runs.n, "selected": 0 if picked is None else picked.m}
    if picked is None:
        return out
    n, m = picked.table.shape[0], picked.m
    head = (_p(runs.bits), *vol.shape, *runs._tables(), _p(runs.tot))
    table = torch.empty_like(picked.table)
    out["measure"] = timed(lambda: _lib.check(L.tomo_cc_measure(*head, _p(table), n, st), "tomo_cc_measure"), warmup, reps)
    head = (*head, _p(picked.sel), _p(picked.slot), n)
    for count in (pipeline.CALIPER_DIRECTIONS, 8):
        dirs, tabs = pipeline._caliper_args(vol.shape, None, 1.0, 1.0, pipeline.caliper_directions(count), "voxels")
        shared = torch.from_numpy(np.concatenate([t.reshape(-1) for t in (tabs.pz, tabs.py, tabs.px, tabs.h)])).to(dev)
        ptr = [shared.data_ptr() + 8 * count * o for o in (0, nz, nz + ny, nz + ny + nx)]
        hi = torch.empty((m, count), dtype=torch.float64, device=dev)
        lo = torch.empty((m, count), dtype=torch.float64, device=dev)
        out["extremes_mib_%d" % count] = round(2 * hi.numel() * 8 / 2 ** 20, 1)
        for extent, h in (("voxels", ptr[3]), ("centres", None)):
            out["caliper_%d_%s" % (count, extent)] = timed(
                lambda: _lib.check(L.tomo_cc_caliper(*head, ptr[0], ptr[1], ptr[2], h, count, _p(hi), _p(lo), m, st), "tomo_cc_caliper"),
                warmup, reps)
        if count == pipeline.CALIPER_DIRECTIONS:
            width = torch.empty((m, count), dtype=torch.float64, device=dev)
            rows = torch.empty((m, 4), dtype=torch.int64, device=dev)
            ext = torch.empty((m, 2), dtype=torch.float64, device=dev)

            def finish():                                       # the keys are decoded in place: fill them again every time
                _lib.check(L.tomo_cc_caliper(*head, ptr[0], ptr[1], ptr[2], None, count, _p(hi), _p(lo), m, st), "tomo_cc_caliper")
                _lib.check(L.tomo_cc_caliper_rows(_p(picked.table), n, _p(runs.tot), _p(picked.sel), _p(picked.slot), _p(hi), _p(lo), count,
                                                  _p(width), _p(rows), _p(ext), m, st), "tomo_cc_caliper_rows")
            out["caliper_64_centres_and_rows"] = timed(finish, warmup, reps)
            out["largest_max_mm"] = round(float(ext[:, 0].max().item()), 3)
    axes = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(m, 1).contiguous()
    if m <= 4096:                                               # the real axes where the moments are cheap to get
        q = runs.moments(pipeline._slice_weights(None, nz, 1.0, 1.0), 1.0, 1.0, min_voxels)
        axes = torch.from_numpy(np.ascontiguousarray(q.principal_axes).reshape(m, 9)).to(dev)
    pos = torch.from_numpy(np.concatenate([tabs.zc, tabs.yt, tabs.xt, tabs.depth])).to(dev)
    at = [pos.data_ptr() + 8 * o for o in (0, nz, nz + ny, nz + ny + nx)]
    hi3 = torch.empty((m, 3), dtype=torch.float64, device=dev)
    lo3 = torch.empty((m, 3), dtype=torch.float64, device=dev)
    out["caliper_axes"] = timed(lambda: _lib.check(L.tomo_cc_caliper_axes(*head, _p(axes), *at, 1.0, 1.0, _p(hi3), _p(lo3), m, st),
                                                   "tomo_cc_caliper_axes"), warmup, reps)
    if pipeline._download(runs.tot)[2]:
        sys.exit("a guard of the kernels fired")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--noise-min-voxels", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calipertime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n, conn = a.n, a.connectivity
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (0, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_min_voxels, lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name, (min_voxels, make) in volumes.items():
        vol = pipeline.pack(make())
        row = {"n": n, "volume": name, "connectivity": conn, "min_voxels": min_voxels,
               "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(passes(vol, conn, min_voxels, a.warmup, a.reps))
        torch.cuda.empty_cache()
        calls = {"component_caliper": lambda: pipeline.component_caliper(vol, connectivity=conn, min_voxels=min_voxels),
                 "component_caliper_oriented": lambda: pipeline.component_caliper(vol, connectivity=conn, min_voxels=min_voxels, oriented=True),
                 "component_properties": lambda: pipeline.component_properties(vol, connectivity=conn, min_voxels=min_voxels),
                 "component_moments": lambda: pipeline.component_moments(vol, connectivity=conn, min_voxels=min_voxels)}
        if name == "porous_ellipsoid":
            calls["cavity_caliper"] = lambda: pipeline.cavity_caliper(vol, connectivity=conn)
        for key, fn in calls.items():
            try:
                row[key] = timed(fn, a.warmup, a.reps)
            except _lib.TomoError as e:
                row[key] = {"error": str(e)[:200]}
            torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
