#!/usr/bin/env python3
"""Homotopic thinning at n^3 (default 512) on the two volumes of tools/recontime.py, resident as BitVolumes: the benchmark's
ellipsoid with a few hundred spherical pores, and seeded noise at 50 %.  For each volume and each mode (connectivity 26 with
and without the end rule, 6 without), in ONE run
  * one pipeline.skeleton traced iteration by iteration: the voxels an iteration cleared and its HIP event time -- the counter
    is read per iteration, as the product does with THIN_ITERATION_BATCH = 1 -- and, from a second, untimed replay that reads
    the tile stamps in front of every sub-pass, the tiles its 48 sub-passes visit (stamp + 48 >= tick; a stamp raised during
    the launch that reads it is not counted);
  * the whole of pipeline.skeleton with THIN_ITERATION_BATCH 1 and 4, host loop and host reads included, with its iterations,
    and sub-passes launched, pipeline.skeleton_nodes on the result, and, as the scale,
    pipeline.distance_transform and pipeline.geodesic_distance (one seed in the middle slice) on the same volume.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/thintime.py [--n 512] [--warmup 1] [--reps 3] [--volumes porous_ellipsoid noise] [--out t.json]
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

KEYS = ("thin_iterations", "thin_passes")
MODES = ((26, True), (26, False), (6, False))


def traced(vol, conn, curve, limit):
    """One thinning taken apart -> (the skeleton, the rows of its iterations)."""
    L, st = _lib.lib(), _stream()
    nz, ny, nx = vol.shape
    tiles = int(L.tomo_geo_tiles(nz, ny, nx))

    def replay(count_tiles):
        bits = vol.bits.clone()
        stamp = torch.zeros(tiles, dtype=torch.int32, device=vol.device)
        out = []
        while len(out) < limit:
            counters = torch.zeros(pipeline.THIN_COUNTER_WORDS, dtype=torch.int64, device=vol.device)
            visited = torch.zeros(1, dtype=torch.int64, device=vol.device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(pipeline.THIN_SUBPASSES):
                tick = pipeline.THIN_SUBPASSES * len(out) + k + 1
                if count_tiles:
                    visited += (stamp.to(torch.int64) + pipeline.THIN_SUBPASSES >= tick).sum()
                _lib.check(L.tomo_thin_pass(_p(bits), None, nz, ny, nx, conn, int(curve), k // 8, k % 8, _p(stamp), tick, _p(counters), st),
                           "tomo_thin_pass")
            b.record()
            b.synchronize()
            out.append((int(counters.sum().item()), int(visited.item()), a.elapsed_time(b)))
            if out[-1][0] == 0:
                break
        return bits, out

    bits, timed_rows = replay(False)
    _, counted_rows = replay(True)
    rows = [{"cleared": c, "tiles_visited": v, "share": round(v / (tiles * pipeline.THIN_SUBPASSES), 4), "ms": round(ms, 3)}
            for (c, _, ms), (_, v, _) in zip(timed_rows, counted_rows)]
    return pipeline.BitVolume(bits, vol.shape), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--trace-limit", type=int, default=1 << 12)
    ap.add_argument("--volumes", nargs="+", default=["porous_ellipsoid", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("thintime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": lambda: porous_ellipsoid(n, a.pores, dev),
               "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
    rows = []
    for name in a.volumes:
        mask = volumes[name]()
        vol = pipeline.pack(mask)
        mid = torch.nonzero(mask[n // 2].reshape(-1))[0].item()
        zyx = np.array([np.unravel_index((n // 2) * n * n + int(mid), vol.shape)], dtype=np.int64)
        del mask
        tiles = int(_lib.lib().tomo_geo_tiles(*vol.shape))
        base = {"n": n, "volume": name, "tiles": tiles, "set_voxels": int(pipeline.popcount_async(vol).item())}
        base["distance_transform"] = timed(lambda: pipeline.distance_transform(vol), a.warmup, a.reps)
        print(json.dumps(base), flush=True)
        for conn, curve in MODES:
            row = dict(base, connectivity=conn, curve=curve)
            skel, trace = traced(vol, conn, curve, a.trace_limit)
            row["trace"] = trace
            row["trace_ms"] = round(sum(r["ms"] for r in trace), 3)
            row["share_of_tiles_per_sub_pass"] = round(sum(r["tiles_visited"] for r in trace) / (tiles * pipeline.THIN_SUBPASSES * len(trace)), 4)
            nodes = pipeline.skeleton_nodes(skel)
            row["skeleton"] = {"voxels": nodes.voxels, "end_points": nodes.end_points, "junction_voxels": nodes.junction_voxels,
                               "isolated": nodes.isolated}
            row["skeleton_nodes"] = timed(lambda: pipeline.skeleton_nodes(skel), a.warmup, a.reps)
            del skel, nodes
            for batch in a.batches:
                pipeline.THIN_ITERATION_BATCH = batch
                row["skeleton_batch_%d" % batch] = counted(lambda: pipeline.skeleton(vol, curve, conn), a.warmup, a.reps, KEYS)
            pipeline.THIN_ITERATION_BATCH = 1
            row["geodesic_distance"] = counted(lambda: pipeline.geodesic_distance(vol, zyx, connectivity=conn), a.warmup, a.reps,
                                               ("geodesic_sweeps",))
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
