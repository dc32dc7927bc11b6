#!/usr/bin/env python3
"""The distance transform at n^3 (default 512 and 1024): the ellipsoid of the benchmark, resident as a BitVolume, with slice
depths in three sides.  HIP events around warmed-up repeats of pipeline.distance_transform, pipeline.offset_volume (r = -1 mm
and + 1 mm) and pipeline.inscribed_sphere; peak device memory of each; the bytes each call must move at the least (the bits in,
4 B per voxel or the bits out) and the share of the 8 TB/s peak that implies.  inscribed_sphere's time includes its one host
read, as a caller pays it.  Context only: scipy.ndimage.distance_transform_edt (uniform sampling -- it has no other) on the
host for the largest n it finishes in under a minute, where SciPy imports.

    python tools/edttime.py [--n 512 1024] [--warmup 2] [--reps 5] [--scipy] [--out edt.json]
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

PEAK_BYTES_PER_S = 8e12
MM_Y, MM_X = 0.7, 0.9


def timed(fn, warmup, reps, min_bytes):
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
    med = float(np.median(ms))
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "peak_mib": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), "min_bytes": int(min_bytes),
            "share_of_peak": round(min_bytes / (med * 1e-3) / PEAK_BYTES_PER_S, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.distance_transform_edt on the host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edttime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    scipy_budget_left = True
    for n in a.n:
        vol = pipeline.pack(pipeline.ellipsoid_mask(n, n, n, dev))
        s = n // 3
        depths = np.array([0.8] * s + [0.25] * s + [1.3] * (n - 2 * s))
        args = (depths, MM_Y, MM_X)
        bits_bytes, voxels = vol.bits.numel() * 8, n ** 3
        L = pipeline._lib.lib()
        ws = int(L.tomo_edt_workspace_bytes(n, n, n, pipeline.EDT_WORKSPACE_BUDGET))
        row = {"n": n, "set_voxels": int(pipeline.popcount_async(vol).item()), "bitvolume_mib": round(bits_bytes / 2 ** 20, 1),
               "workspace_mib": round(ws / 2 ** 20, 1), "chunk_columns": int(L.tomo_edt_chunk_columns(n, n, n, ws)),
               "sphere": pipeline.inscribed_sphere(vol, *args)}
        row["distance_transform"] = timed(lambda: pipeline.distance_transform(vol, *args), a.warmup, a.reps, bits_bytes + 4 * voxels)
        row["offset_volume(-1mm)"] = timed(lambda: pipeline.offset_volume(vol, -1.0, *args), a.warmup, a.reps, 2 * bits_bytes)
        row["offset_volume(+1mm)"] = timed(lambda: pipeline.offset_volume(vol, 1.0, *args), a.warmup, a.reps, 2 * bits_bytes)
        row["inscribed_sphere"] = timed(lambda: pipeline.inscribed_sphere(vol, *args), a.warmup, a.reps, bits_bytes)
        if a.scipy and scipy_budget_left:
            try:
                from scipy import ndimage
                host = np.pad(pipeline.unpack(vol).cpu().numpy(), 1)
                t0 = time.perf_counter()
                ndimage.distance_transform_edt(host, sampling=(0.5, MM_Y, MM_X))
                took = time.perf_counter() - t0
                row["scipy.distance_transform_edt_host_s"] = round(took, 2)
                scipy_budget_left = took * 8 < 60                # the next size is 8 times the voxels
                del host
            except ImportError:
                row["scipy.distance_transform_edt_host_s"] = "SciPy is not installed here"
        del vol
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
