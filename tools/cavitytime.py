#!/usr/bin/env python3
"""Cavities at n^3 (default 512) on two volumes, resident as BitVolumes: the benchmark's ellipsoid with a few hundred spherical
pores carved out of it -- few, compact cavities in one solid body -- and seeded noise at 50 % -- millions of background
components, most of them cavities.  HIP events around warmed-up repeats of
  * the whole of pipeline.fill_cavities and pipeline.cavity_table (labellings, host reads and the download included),
  * the whole of pipeline.component_topology on the same volume -- its complement-and-label work is the same, the unit the two
    are to be read against,
  * tomo_cc_select (enclosed) and tomo_cc_fill_map alone, on the tables of the complement labelled once,
and, as context only and once, scipy.ndimage.binary_fill_holes on the downloaded array on the host (--host).
2 warm-up calls and 5 timed ones by default; median / min / max.

    python tools/cavitytime.py [--n 512] [--warmup 2] [--reps 5] [--density 0.5] [--pores 300] [--connectivity 6] [--host] [--out cavities.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def porous_ellipsoid(n, pores, dev):
    """The benchmark's ellipsoid minus `pores` balls of radius 2 .. n / 64 voxels at seeded places in its inner half."""
    mask = pipeline.ellipsoid_mask(n, n, n, dev).view(torch.bool).clone()
    rng = np.random.default_rng(n)
    rmax = max(3, n // 64)
    for _ in range(pores):
        r = int(rng.integers(2, rmax + 1))
        c = [int(x) for x in rng.integers(n // 2 - n // 5, n // 2 + n // 5, 3)]
        lo, hi = [x - r for x in c], [x + r + 1 for x in c]
        z, y, x = torch.meshgrid(*[torch.arange(a, b, device=dev) - m for a, b, m in zip(lo, hi, c)], indexing="ij")
        mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] &= (z * z + y * y + x * x) > r * r
    return mask.view(torch.uint8)


def device_steps(vol, conn, warmup, reps):
    """Event times of the selection and of the fill pass on the tables of the complement, labelled once."""
    L, dev, st = _lib.lib(), vol.device, _stream()
    bg = pipeline._complement_runs(vol, conn)
    out = {"background_runs": bg.runs}
    if bg.runs == 0:
        return out
    table = bg.table()
    n = table.shape[0]
    sel = torch.empty(n, dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    slot = torch.empty(n, dtype=torch.int32, device=dev)
    blk = torch.empty(2 * L.tomo_cc_scan_blocks(n), dtype=torch.int64, device=dev)
    filled = torch.empty_like(vol.bits)
    steps = {
        "select_enclosed": lambda: _lib.check(L.tomo_cc_select(_p(table), n, _p(bg.tot), 0, pipeline.NO_MAX_VOXELS, 0, 1, *vol.shape, _p(sel),
                                                               _p(off), _p(slot), _p(blk), st), "tomo_cc_select"),
        "fill_map": lambda: _lib.check(L.tomo_cc_fill_map(_p(bg.bits), *vol.shape, *bg._tables(), _p(bg.tot), _p(sel), n, _p(vol.bits),
                                                          _p(filled), st), "tomo_cc_fill_map"),
    }
    out["background_components"] = n
    for name, fn in steps.items():
        out[name] = timed(fn, warmup, reps)
    tot = pipeline._download(bg.tot)
    if tot[2]:
        sys.exit("a guard of the kernels fired")
    out["cavities"] = tot[5]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6])
    ap.add_argument("--host", action="store_true", help="time scipy.ndimage.binary_fill_holes on the host as well (context only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cavitytime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.n:
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        volumes = {"porous_ellipsoid": lambda: porous_ellipsoid(n, a.pores, dev),
                   "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
        for name, make in volumes.items():
            vol = pipeline.pack(make())
            for conn in a.connectivity:
                row = {"n": n, "volume": name, "connectivity": conn, "set_voxels": int(pipeline.popcount_async(vol).item())}
                row.update(device_steps(vol, conn, a.warmup, a.reps))
                torch.cuda.empty_cache()
                filled = pipeline.fill_cavities(vol, conn)
                row["filled_voxels"] = int(pipeline.popcount_async(filled).item()) - row["set_voxels"]
                row["fill_cavities"] = timed(lambda: pipeline.fill_cavities(vol, conn), a.warmup, a.reps)
                row["cavity_table"] = timed(lambda: pipeline.cavity_table(vol, connectivity=conn), a.warmup, a.reps)
                row["component_topology"] = timed(lambda: pipeline.component_topology(vol, conn), a.warmup, a.reps)
                torch.cuda.empty_cache()
                if a.host:
                    from scipy import ndimage
                    host = pipeline.unpack(vol).cpu().numpy()
                    t0 = time.perf_counter()
                    ref = ndimage.binary_fill_holes(host, structure=ndimage.generate_binary_structure(3, 1 if conn == 26 else 3))
                    row["host_binary_fill_holes_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                    row["host_agrees"] = bool(np.array_equal(ref, pipeline.unpack(filled).cpu().numpy()))
                    del host, ref
                del filled
                rows.append(row)
                print(json.dumps(row), flush=True)
            del vol
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
