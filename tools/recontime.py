#!/usr/bin/env python3
"""Grey reconstruction, the extended maxima and the separation by height at n^3 (default 512), unit spacing, on the two volumes
of tools/zonetime.py, resident as BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores, and seeded noise at
50 %.  The map is the volume's own inside distance (pipeline.distance_transform), the markers are separate_by_height's:
extended_maxima(vol, distance, --h) (--noise-h on the noise).  For each volume and each connectivity, in ONE run
  * the two reconstructions of one pipeline.extended_maxima traced sweep by sweep (tomo_recon_seed in mode 1, then in mode 2
    over the h-maxima): the sweeps, the dirty tiles a sweep starts with and its HIP event time -- the flags are read between
    the sweeps here, which the product never does.  Every phase starts with every flag set, so its first sweep is reported
    apart;
  * tools/zonetime.py's trace of pipeline.geodesic_zones from the same markers: the distance sweeps and the label sweeps of the
    separation that follows.  recon_over_zones is the summed sweep time of tomo_recon_sweep over that of tomo_geo_sweep and
    tomo_zone_sweep together;
  * the whole of pipeline.h_maxima, regional_maxima, extended_maxima, separate_by_height and, next to it,
    pipeline.distance_transform and pipeline.separate_components (--radius, --noise-radius), host reads included.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/recontime.py [--n 512] [--warmup 1] [--reps 3] [--h 1] [--noise-h 0.5] [--radius 8] [--noise-radius 1] [--out t.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cavitytime import porous_ellipsoid  # noqa: E402
from zonetime import counted, phase_row, traced as traced_zones  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

KEYS = ("recon_calls", "recon_sweeps", "geodesic_sweeps", "zone_sweeps")


def traced_phase(vol, mask, mode, h, conn, limit):
    """One reconstruction taken apart -> (g, the row)."""
    L, st = _lib.lib(), _stream()
    nz, ny, nx = vol.shape
    plan = pipeline._GeodesicPlan(vol, None, conn)
    g = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    _lib.check(L.tomo_recon_seed(_p(plan.bits), _p(mask), None, mode, h, nz, ny, nx, _p(g), _p(plan.counters), st), "tomo_recon_seed")
    below = int(pipeline.popcount_async(pipeline.BitVolume(below_bits(vol, mask, g), vol.shape)).item())
    tiles, ms = [], []
    cur = 0
    plan.dirty[cur].fill_(1)
    while len(tiles) < limit:
        dirty = int(plan.dirty[cur].sum().item())
        if dirty == 0:
            break
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.tomo_recon_sweep(_p(plan.bits), nz, ny, nx, conn, _p(mask), _p(g), _p(plan.dirty[cur]), _p(plan.dirty[1 - cur]),
                                      _p(plan.counters), st), "tomo_recon_sweep")
        b.record()
        b.synchronize()
        tiles.append(dirty)
        ms.append(a.elapsed_time(b))
        cur = 1 - cur
    return g, dict(phase_row(tiles, ms), converged=len(tiles) < limit, voxels_below_the_ceiling_at_the_start=below,
                   tile_launches_that_changed_something=int(plan.counters[0].item()))


def below_bits(vol, mask, g):
    out = torch.empty_like(vol.bits)
    _lib.check(_lib.lib().tomo_recon_below(_p(vol.bits), _p(mask), _p(g), *vol.shape, _p(out), _stream()), "tomo_recon_below")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--h", type=float, default=1.0)
    ap.add_argument("--noise-h", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--noise-radius", type=float, default=1.0)
    ap.add_argument("--connectivities", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--trace-limit", type=int, default=1 << 12)
    ap.add_argument("--volumes", nargs="+", default=["porous_ellipsoid", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("recontime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (a.h, a.radius, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_h, a.noise_radius, lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name in a.volumes:
        h, radius, make = volumes[name]
        vol = pipeline.pack(make())
        inside = pipeline.distance_transform(vol)
        base = {"n": n, "volume": name, "h_mm": h, "radius_mm": radius, "batch": pipeline.GEODESIC_SWEEP_BATCH,
                "set_voxels": int(pipeline.popcount_async(vol).item()), "max_distance_mm": float(inside.max().item())}
        for conn in a.connectivities:
            row = dict(base, connectivity=conn)
            domes, row["h_maxima_trace"] = traced_phase(vol, inside, 1, h, conn, a.trace_limit)
            g, row["regional_trace"] = traced_phase(vol, domes, 2, 0.0, conn, a.trace_limit)
            markers = pipeline.BitVolume(below_bits(vol, domes, g), vol.shape)
            del domes, g
            row["marker_voxels"] = int(pipeline.popcount_async(markers).item())
            row["marker_components"] = int(pipeline.ComponentRuns(markers, conn).sizes().shape[0])
            zone, row["zones_trace"] = traced_zones(vol, markers, conn, a.trace_limit)
            del zone, markers
            recon = row["h_maxima_trace"].get("ms_all_sweeps", 0.0) + row["regional_trace"].get("ms_all_sweeps", 0.0)
            zones = row["zones_trace"]["distance"].get("ms_all_sweeps", 0.0) + row["zones_trace"]["label"].get("ms_all_sweeps", 0.0)
            row["recon_sweeps_ms"], row["zone_sweeps_ms"] = round(recon, 3), round(zones, 3)
            row["recon_over_zones"] = round(recon / zones, 3) if zones else None
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            calls = {"distance_transform": lambda: pipeline.distance_transform(vol),
                     "h_maxima": lambda: pipeline.h_maxima(vol, inside, h, conn),
                     "regional_maxima": lambda: pipeline.regional_maxima(vol, inside, conn),
                     "extended_maxima": lambda: pipeline.extended_maxima(vol, inside, h, conn),
                     "separate_by_height": lambda: pipeline.separate_by_height(vol, h, connectivity=conn),
                     "separate_components": lambda: pipeline.separate_components(vol, radius, connectivity=conn)}
            for key, fn in calls.items():
                try:
                    row[key] = counted(fn, a.warmup, a.reps, KEYS)
                    if key.startswith("separate"):
                        got = fn()
                        row[key].update(markers=got.markers, cut_voxels=got.cut_voxels,
                                        components_after=int(pipeline.ComponentRuns(got.volume, conn).sizes().shape[0]))
                        del got
                except _lib.TomoError as e:
                    row[key] = {"error": str(e)[:200]}
                print(json.dumps({key: row[key]}), flush=True)
                torch.cuda.empty_cache()
            rows.append(row)
        del vol, inside
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
