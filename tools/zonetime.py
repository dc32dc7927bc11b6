#!/usr/bin/env python3
"""Geodesic zones, the cut and the separation at n^3 (default 512), unit spacing, on the two volumes of tools/geodesictime.py,
resident as BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores, and seeded noise at 50 %.  The markers are
separate_components' own: the ball erosion of the volume by --radius (--noise-radius on the noise).  For each volume and each
connectivity, in ONE run
  * one traced pipeline.geodesic_zones, sweep by sweep: per phase (distance sweeps, then label sweeps) the sweeps, the dirty
    tiles a sweep starts with and its HIP event time -- the flags are read between the sweeps here, which the product never
    does.  The label phase starts with every flag set, so its first sweep is reported apart.  label_over_distance is the ratio
    of the two phases' summed sweep times: the yardstick of the label phase is the distance phase of the same call;
  * tomo_zone_cut alone;
  * the whole of pipeline.separate_components (erosion, labelling of the markers, both phases, the cut, host reads included);
  * pipeline.geodesic_distance from the same markers and pipeline.component_properties on the same volume, as the units to
    read the others against.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/zonetime.py [--n 512] [--warmup 1] [--reps 3] [--radius 8] [--noise-radius 1] [--noise-min-voxels 8] [--out t.json]
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


def phase_row(tiles, ms):
    if not tiles:
        return {"sweeps": 0}
    row = {"sweeps": len(tiles), "dirty_tiles_per_sweep_mean": round(float(np.mean(tiles)), 1), "dirty_tiles_total": int(sum(tiles)),
           "ms_per_sweep_mean": round(float(np.mean(ms)), 4), "ms_per_sweep_median": round(float(np.median(ms)), 4),
           "ms_per_sweep_max": round(float(max(ms)), 4), "ms_all_sweeps": round(float(sum(ms)), 3),
           "us_per_dirty_tile": round(1e3 * float(sum(ms)) / max(1, sum(tiles)), 4)}
    if len(tiles) > 1:
        row["first_sweep"] = {"dirty_tiles": tiles[0], "ms": round(ms[0], 4)}
        row["later_sweeps"] = {"dirty_tiles_per_sweep_mean": round(float(np.mean(tiles[1:])), 1), "ms_per_sweep_mean": round(float(np.mean(ms[1:])), 4)}
    return row


def traced(vol, markers, conn, limit):
    """One geodesic_zones call taken apart -> (zones, the row)."""
    L, st = _lib.lib(), _stream()
    nz, ny, nx = vol.shape
    plan = pipeline._GeodesicPlan(vol, pipeline._geodesic_tables(vol.shape, None, 1.0, 1.0), conn)
    labels, n = pipeline.ComponentRuns(markers, conn).labels()
    dist = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    zone = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
    _lib.check(L.tomo_zone_seed_labels(_p(plan.bits), _p(labels), nz, ny, nx, _p(dist), _p(zone), plan.seed_tail()[0], st), "tomo_zone_seed_labels")
    del labels
    launches = {"distance": lambda cur, nxt: L.tomo_geo_sweep(_p(plan.bits), nz, ny, nx, conn, _p(plan.wxy), _p(plan.wz), _p(dist), cur, nxt,
                                                              _p(plan.counters), st),
                "label": lambda cur, nxt: L.tomo_zone_sweep(_p(plan.bits), nz, ny, nx, conn, _p(plan.wxy), _p(plan.wz), _p(dist), _p(zone), cur, nxt,
                                                            _p(plan.counters), st)}
    row = {"tiles": plan.tiles, "marker_components": int(n)}
    cur = 0
    for phase, launch in launches.items():
        if phase == "label":
            plan.dirty[cur].fill_(1)
        tiles, ms = [], []
        while len(tiles) < limit:
            dirty = int(plan.dirty[cur].sum().item())
            if dirty == 0:
                break
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(launch(_p(plan.dirty[cur]), _p(plan.dirty[1 - cur])), phase)
            b.record()
            b.synchronize()
            tiles.append(dirty)
            ms.append(a.elapsed_time(b))
            cur = 1 - cur
        row[phase] = dict(phase_row(tiles, ms), converged=len(tiles) < limit)
    if row["distance"]["sweeps"] and row["label"]["sweeps"]:
        row["label_over_distance"] = round(row["label"]["ms_all_sweeps"] / row["distance"]["ms_all_sweeps"], 3)
        row["label_over_distance_per_dirty_tile"] = round(row["label"]["us_per_dirty_tile"] / row["distance"]["us_per_dirty_tile"], 3)
    row["reached_voxels"] = int((zone > 0).sum().item())
    row["zones"] = int(torch.unique(zone).numel()) - 1
    return zone, row


def counted(fn, warmup, reps, keys=("geodesic_sweeps", "zone_sweeps")):
    """timed(), with the sweeps one call took."""
    c0 = dict(pipeline.COUNTERS)
    fn()
    took = {k: pipeline.COUNTERS[k] - c0[k] for k in keys}
    return dict(timed(fn, warmup, reps), **took)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--noise-radius", type=float, default=1.0)
    ap.add_argument("--connectivities", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--noise-min-voxels", type=int, default=8)
    ap.add_argument("--trace-limit", type=int, default=1 << 12)
    ap.add_argument("--volumes", nargs="+", default=["porous_ellipsoid", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zonetime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (0, a.radius, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_min_voxels, a.noise_radius,
                         lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name in a.volumes:
        min_voxels, radius, make = volumes[name]
        vol = pipeline.pack(make())
        markers = pipeline.offset_volume(vol, -radius)
        base = {"n": n, "volume": name, "radius_mm": radius, "batch": pipeline.GEODESIC_SWEEP_BATCH,
                "set_voxels": int(pipeline.popcount_async(vol).item()), "marker_voxels": int(pipeline.popcount_async(markers).item())}
        for conn in a.connectivities:
            row = dict(base, connectivity=conn)
            zone, row["trace"] = traced(vol, markers, conn, a.trace_limit)
            cleared = torch.zeros(1, dtype=torch.int64, device=dev)
            out = torch.empty_like(vol.bits)

            def cut():
                cleared.zero_()
                _lib.check(_lib.lib().tomo_zone_cut(_p(vol.bits), _p(zone), *vol.shape, conn, _p(out), _p(cleared), _stream()), "tomo_zone_cut")
            row["cut"] = dict(timed(cut, a.warmup, a.reps), cut_voxels=int(cleared.item()))
            del zone, out
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            calls = {"separate_components": lambda: pipeline.separate_components(vol, radius, connectivity=conn),
                     "geodesic_zones": lambda: pipeline.geodesic_zones(vol, markers, connectivity=conn),
                     "geodesic_distance": lambda: pipeline.geodesic_distance(vol, markers, connectivity=conn),
                     "component_properties": lambda: pipeline.component_properties(vol, connectivity=conn, min_voxels=min_voxels)}
            for key, fn in calls.items():
                try:
                    row[key] = counted(fn, a.warmup, a.reps)
                    if key == "separate_components":
                        got = fn()
                        row[key].update(markers=got.markers, cut_voxels=got.cut_voxels,
                                        components_after=int(pipeline.ComponentRuns(got.volume, conn).sizes().shape[0]))
                        del got
                except _lib.TomoError as e:
                    row[key] = {"error": str(e)[:200]}
                print(json.dumps({key: row[key]}), flush=True)
                torch.cuda.empty_cache()
            rows.append(row)
        del vol, markers
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
