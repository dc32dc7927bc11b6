#!/usr/bin/env python3
"""Geodesic distance and geodesic length at n^3 (default 512), unit spacing, on the two volumes of tools/cavitytime.py, resident
as BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores -- one solid body -- and seeded noise at 50 % --
millions of components, of which those of at least --noise-min-voxels voxels are selected.  For each volume
  * pipeline.distance_transform (tomo_edt_distance) in the same run, as the yardstick;
  * pipeline.geodesic_distance from ONE seed (the first set voxel of the middle slice): one traced propagation -- per sweep the
    dirty tiles it started with and its HIP event time -- and the whole call, host reads included, as a caller pays them;
  * the two value passes of a farthest-point search (tomo_cc_value_max + tomo_cc_value_first over the run tables) on their own, on
    the all-zero map (the search's a0) and on the traced distance map;
  * pipeline.component_geodesic under the selection and, on the ellipsoid, pipeline.cavity_geodesic: the whole call, with the
    sweeps it took (pipeline.COUNTERS).
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/geodesictime.py [--n 512] [--warmup 1] [--reps 3] [--noise-min-voxels 8] [--out t.json]
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


def counted(fn, warmup, reps):
    """timed(), with the sweeps one call took."""
    c0 = pipeline.COUNTERS["geodesic_sweeps"]
    fn()
    sweeps = pipeline.COUNTERS["geodesic_sweeps"] - c0
    return dict(timed(fn, warmup, reps), sweeps=sweeps)


def traced(vol, seed, conn, limit):
    """One propagation from `seed`, sweep by sweep: the dirty tiles a sweep starts with and its event time; the flags are read
    between the sweeps here, which the product never does."""
    L, st = _lib.lib(), _stream()
    nz, ny, nx = vol.shape
    plan = pipeline._GeodesicPlan(vol, pipeline._geodesic_tables(vol.shape, None, 1.0, 1.0), conn)
    dist = torch.full(vol.shape, float("inf"), dtype=torch.float32, device=vol.device)
    index = torch.tensor([seed], dtype=torch.int64, device=vol.device)
    _lib.check(L.tomo_geo_seed_index(_p(plan.bits), nz, ny, nx, _p(index), None, 1, _p(dist), *plan.seed_tail(), st), "tomo_geo_seed_index")
    tiles, ms = [], []
    cur = 0
    while len(tiles) < limit:
        dirty = int(plan.dirty[cur].sum().item())
        if dirty == 0:
            break
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.tomo_geo_sweep(_p(plan.bits), nz, ny, nx, conn, _p(plan.wxy), _p(plan.wz), _p(dist), _p(plan.dirty[cur]),
                                    _p(plan.dirty[1 - cur]), _p(plan.counters), st), "tomo_geo_sweep")
        b.record()
        b.synchronize()
        tiles.append(dirty)
        ms.append(a.elapsed_time(b))
        cur = 1 - cur
    finite = torch.isfinite(dist)
    return dist, {"tiles": plan.tiles, "sweeps": len(tiles), "converged": len(tiles) < limit, "dirty_tiles_per_sweep_mean": round(float(np.mean(tiles)), 1),
            "dirty_tiles_per_sweep_max": int(max(tiles)), "dirty_tiles_total": int(sum(tiles)), "ms_per_sweep_median": round(float(np.median(ms)), 4),
            "ms_per_sweep_max": round(float(max(ms)), 4), "ms_all_sweeps": round(float(sum(ms)), 3),
            "workgroups_that_changed": int(plan.counters[0].item()), "reached_voxels": int(finite.sum().item()),
            "farthest_mm": round(float(dist[finite].max().item()), 3)}


def value_passes(runs, dist, warmup, reps):
    """tomo_cc_value_max + tomo_cc_value_first over the tables of `runs` on the float32 map `dist`."""
    L, st = _lib.lib(), _stream()
    n = runs.table().shape[0]
    if n == 0:
        return None
    best = torch.empty(n, dtype=torch.int32, device=dist.device)
    first = torch.empty(n, dtype=torch.int64, device=dist.device)
    head = (_p(runs.bits), *runs.vol.shape, *runs._tables(), _p(runs.tot), _p(dist), None)

    def both():
        _lib.check(L.tomo_cc_value_max(*head, _p(best), n, st), "tomo_cc_value_max")
        _lib.check(L.tomo_cc_value_first(*head, _p(best), _p(first), n, st), "tomo_cc_value_first")
    return dict(timed(both, warmup, reps), components=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--noise-min-voxels", type=int, default=8)
    ap.add_argument("--trace-limit", type=int, default=1 << 14)
    ap.add_argument("--volumes", nargs="+", default=["porous_ellipsoid", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("geodesictime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n, conn = a.n, a.connectivity
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (0, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_min_voxels, lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name in a.volumes:
        min_voxels, make = volumes[name]
        mask = make()
        vol = pipeline.pack(mask)
        mid = torch.nonzero(mask[n // 2].reshape(-1))[0].item()
        seed = (n // 2) * n * n + int(mid)
        del mask
        row = {"n": n, "volume": name, "connectivity": conn, "min_voxels": min_voxels, "batch": pipeline.GEODESIC_SWEEP_BATCH,
               "set_voxels": int(pipeline.popcount_async(vol).item())}
        row["distance_transform"] = timed(lambda: pipeline.distance_transform(vol), a.warmup, a.reps)
        dist, row["trace"] = traced(vol, seed, conn, a.trace_limit)
        runs = pipeline.ComponentRuns(vol, conn)
        row["value_passes_distance_map"] = value_passes(runs, dist, a.warmup, a.reps)
        dist.zero_()
        row["value_passes_zero_map"] = value_passes(runs, dist, a.warmup, a.reps)
        if name == "porous_ellipsoid":
            dist.fill_(float("inf"))
            row["value_passes_complement_inf_map"] = value_passes(pipeline._complement_runs(vol, conn), dist, a.warmup, a.reps)
        del dist, runs
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        zyx = np.array([np.unravel_index(seed, vol.shape)], dtype=np.int64)
        calls = {"geodesic_distance": lambda: pipeline.geodesic_distance(vol, zyx, connectivity=conn),
                 "component_geodesic": lambda: pipeline.component_geodesic(vol, connectivity=conn, min_voxels=min_voxels)}
        if name == "porous_ellipsoid":
            calls["cavity_geodesic"] = lambda: pipeline.cavity_geodesic(vol, connectivity=conn)
        for key, fn in calls.items():
            try:
                row[key] = counted(fn, a.warmup, a.reps)
                if key != "geodesic_distance":
                    got = fn()
                    row[key].update(rows=len(got), longest_mm=round(float(got.length_mm.max()), 3) if len(got) else 0.0,
                                    largest_tortuosity=round(float(got.tortuosity.max()), 3) if len(got) else 0.0)
            except _lib.TomoError as e:
                row[key] = {"error": str(e)[:200]}
            print(json.dumps({key: row[key]}), flush=True)
            torch.cuda.empty_cache()
        rows.append(row)
        del vol
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
