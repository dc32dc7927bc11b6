#!/usr/bin/env python3
"""Connected components at n^3 (default 512 and 1024): the ellipsoid of the benchmark with a seeded speckle, resident as a
BitVolume.  HIP events around pipeline.keep_components, pipeline.label_components and -- the yardstick, same volume, same run --
pipeline.smooth; peak device memory of each; scipy.ndimage.label on the host where SciPy imports.  The event times of the two
component calls include their two small host reads (the run count sizes the tables), as a caller pays them.

    python tools/componentstime.py [--n 512 1024] [--warmup 2] [--reps 7] [--speckle 0.001] [--scipy] [--out components.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomography_3d_reconstructor_amd import pipeline  # noqa: E402


def timed(fn, warmup, reps):
    """-> (median ms, min ms, max ms by HIP events, peak bytes above what was allocated before the call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "peak_mib": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--speckle", type=float, default=0.001)
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.label on the host (tens of seconds at 1024^3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("componentstime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.n:
        mask = pipeline.ellipsoid_mask(n, n, n, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        mask = (mask.view(torch.bool) ^ (torch.rand((n, n, n), device=dev, generator=gen) < a.speckle)).view(torch.uint8)
        vol = pipeline.close_ends(pipeline.pack(mask), inplace=True)
        runs = pipeline.ComponentRuns(vol)
        row = {"n": n, "set_voxels": int(pipeline.popcount_async(vol).item()), "runs": runs.runs, "components": int(runs.sizes().shape[0]),
               "bitvolume_mib": round(vol.bits.numel() * 8 / 2 ** 20, 1)}
        del runs
        row["keep_components(min_voxels=64)"] = timed(lambda: pipeline.keep_components(vol, 64), a.warmup, a.reps)
        row["keep_components(largest)"] = timed(lambda: pipeline.keep_components(vol, 0, True), a.warmup, a.reps)
        row["label_components"] = timed(lambda: pipeline.label_components(vol), a.warmup, a.reps)
        row["label_components_26"] = timed(lambda: pipeline.label_components(vol, 26), a.warmup, a.reps)
        row["smooth(3, True)"] = timed(lambda: pipeline.smooth(vol, 3, True), a.warmup, a.reps)
        if a.scipy:
            try:
                from scipy import ndimage
                host = pipeline.unpack(vol).cpu().numpy()
                t0 = time.perf_counter()
                _, count = ndimage.label(host)
                row["scipy.ndimage.label_host_s"] = round(time.perf_counter() - t0, 2)
                assert count == row["components"], (count, row["components"])
                del host
            except ImportError:
                row["scipy.ndimage.label_host_s"] = "SciPy is not installed here"
        del mask, vol
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
