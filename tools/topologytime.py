#!/usr/bin/env python3
"""Euler number, cavities and handles at n^3 (default 512) on two volumes, resident as BitVolumes: the benchmark's ellipsoid --
one component, the wave-combined path of the kernels -- and seeded noise at 25 % -- millions of components, the divergent path
(the volumes of tools/componentpropstime.py).  HIP events around warmed-up repeats of
  * tomo_cc_euler without tables (pipeline.euler_number's launch: the whole-volume Euler number),
  * tomo_cc_euler on run tables labelled once (one counter per component),
  * tomo_cc_measure on the same tables -- the comparable one-pass-over-the-runs kernel, as context -- and the ratio of the medians,
  * the whole of pipeline.component_topology (both labellings, the complement, the attribution, the host reads and the download),
  * the whole of pipeline.euler_number (one launch, one host read).
2 warm-up calls and 5 timed ones by default; median / min / max.

    python tools/topologytime.py [--n 512] [--warmup 2] [--reps 5] [--density 0.25] [--connectivity 6 26] [--out topology.json]
"""
import argparse
import json
import os
import sys

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


def device_steps(vol, conn, warmup, reps):
    """Event times of the Euler pass (with and without tables) and of tomo_cc_measure on run tables labelled once."""
    nz, ny, nx = vol.shape
    L, dev, st = _lib.lib(), vol.device, _stream()
    cr = pipeline.ComponentRuns(vol, conn)
    n = cr._checked()
    geo = (_p(cr.bits), nz, ny, nx)
    euler = torch.empty(n, dtype=torch.int64, device=dev)
    chi = torch.empty(1, dtype=torch.int64, device=dev)
    table = torch.empty((n, pipeline.TABLE_COLUMNS), dtype=torch.int64, device=dev)
    steps = {
        "euler_whole_volume": lambda: _lib.check(L.tomo_cc_euler(*geo, conn, None, 0, None, None, None, _p(chi), 1, st), "tomo_cc_euler"),
        "euler_per_component": lambda: _lib.check(L.tomo_cc_euler(*geo, conn, *cr._tables(), _p(cr.tot), _p(euler), n, st), "tomo_cc_euler"),
        "measure": lambda: _lib.check(L.tomo_cc_measure(*geo, *cr._tables(), _p(cr.tot), _p(table), n, st), "tomo_cc_measure"),
    }
    out = {"runs": cr.runs, "components": n}
    for name, fn in steps.items():
        out[name] = timed(fn, warmup, reps)
    out["euler_per_component_over_measure"] = round(out["euler_per_component"]["median_ms"] / max(out["measure"]["median_ms"], 1e-3), 2)
    if pipeline._download(cr.tot)[2]:
        sys.exit("a guard of the kernels fired")
    if int(chi.item()) != int(euler.sum().item()):
        sys.exit("the components' Euler numbers do not add up to the volume's")
    out["euler_number"] = int(chi.item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topologytime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.n:
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        volumes = {"ellipsoid": lambda: pipeline.ellipsoid_mask(n, n, n, dev),
                   "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
        for name, make in volumes.items():
            vol = pipeline.pack(make())
            for conn in a.connectivity:
                row = {"n": n, "volume": name, "connectivity": conn, "set_voxels": int(pipeline.popcount_async(vol).item())}
                row.update(device_steps(vol, conn, a.warmup, a.reps))
                torch.cuda.empty_cache()
                row["volume_topology"] = pipeline.volume_topology(vol, conn)
                row["component_topology"] = timed(lambda: pipeline.component_topology(vol, conn), a.warmup, a.reps)
                row["component_topology_largest"] = timed(lambda: pipeline.component_topology(vol, conn, largest=True), a.warmup, a.reps)
                row["euler_number_call"] = timed(lambda: pipeline.euler_number(vol, conn), a.warmup, a.reps)
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
