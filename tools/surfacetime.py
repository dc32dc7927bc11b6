#!/usr/bin/env python3
"""Crofton surface area at n^3 (default 512) on two volumes, resident as BitVolumes: the benchmark's ellipsoid -- one component,
the wave-combined path of the kernels -- and seeded noise at 25 % -- millions of components, the divergent path (the volumes of
tools/componentpropstime.py).  HIP events around warmed-up repeats of
  * tomo_cc_surface_hist without tables (pipeline.surface_area's first launch: eleven counters per slice of the volume),
  * tomo_cc_surface_hist on run tables labelled and selected once (eleven counters per slice of every component's box),
  * tomo_cc_moment_hist on the same tables and the same selection -- the comparable pass with six sums per entry, the yardstick --
    and the ratio of the medians,
  * tomo_cc_surface, the finishing kernel, on those counters,
  * the whole of pipeline.component_surface (labelling, selection, both kernels, the host reads and the download),
  * the whole of pipeline.surface_area (two launches, one host read).
The per-component counts are checked to add up to the unlabelled ones.  2 warm-up calls and 5 timed ones by default; median /
min / max.

    python tools/surfacetime.py [--n 512] [--warmup 2] [--reps 5] [--density 0.25] [--connectivity 6] [--out surface.json]
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
    """Event times of the surface pass (with and without tables), of the moment pass on the same tables and of the finishing
    kernel, on run tables labelled once with every component selected."""
    nz, ny, nx = vol.shape
    L, dev, st = _lib.lib(), vol.device, _stream()
    cr = pipeline.ComponentRuns(vol, conn)
    picked = cr.select(0, False)
    n, total, m = picked.table.shape[0], picked.total, picked.m
    geo = (_p(cr.bits), nz, ny, nx)
    hist_head, finish_head = cr.hist_head(picked), cr.finish_head(picked)
    whole = torch.empty(pipeline.SURFACE_COUNTERS * nz, dtype=torch.int64, device=dev)
    surf = torch.empty(pipeline.SURFACE_COUNTERS * total, dtype=torch.int64, device=dev)
    mom = torch.empty(pipeline.MOMENT_SUMS * total, dtype=torch.int64, device=dev)
    tab = torch.from_numpy(pipeline.surface_factors(None, nz)).to(dev)
    area = torch.empty(m, dtype=torch.float64, device=dev)
    counts = torch.empty((m, pipeline.SURFACE_CLASSES), dtype=torch.int64, device=dev)
    labels = torch.empty(m, dtype=torch.int64, device=dev)
    steps = {
        "surface_hist_whole_volume": lambda: _lib.check(L.tomo_cc_surface_hist(*geo, None, 0, None, None, None, None, 0, None, None,
                                                                               _p(whole), nz, st), "tomo_cc_surface_hist"),
        "surface_hist_per_component": lambda: _lib.check(L.tomo_cc_surface_hist(*hist_head, _p(surf), total, st), "tomo_cc_surface_hist"),
        "moment_hist": lambda: _lib.check(L.tomo_cc_moment_hist(*hist_head, _p(mom), total, st), "tomo_cc_moment_hist"),
        "surface_finish": lambda: _lib.check(L.tomo_cc_surface(*finish_head, _p(surf), total, _p(tab), nz, 13, _p(area), _p(counts),
                                                               _p(labels), m, st), "tomo_cc_surface"),
    }
    out = {"runs": cr.runs, "components": n, "slice_entries": total, "surface_hist_bytes": 8 * pipeline.SURFACE_COUNTERS * total}
    for name, fn in steps.items():
        out[name] = timed(fn, warmup, reps)
    out["surface_hist_over_moment_hist"] = round(out["surface_hist_per_component"]["median_ms"] / max(out["moment_hist"]["median_ms"], 1e-3), 2)
    if pipeline._download(cr.tot)[2]:
        sys.exit("a guard of the kernels fired")
    per_slice = surf.view(total, pipeline.SURFACE_COUNTERS).sum(dim=0)
    if not torch.equal(per_slice, whole.view(nz, pipeline.SURFACE_COUNTERS).sum(dim=0)):
        sys.exit("the components' counts do not add up to the volume's")
    out["pair_counts"] = [int(x) for x in counts.sum(dim=0).cpu()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surfacetime needs a GPU: there is nothing to fall back to")
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
                whole = pipeline.surface_area(vol)
                row["surface_area_unit_spacing"] = whole.surface_area_mm2
                if whole.pair_counts.tolist() != row["pair_counts"]:
                    sys.exit("pipeline.surface_area disagrees with the per-component counts")
                # every noise speck is selected here: grant the counters of all of them (the default budget is 1 GiB)
                pipeline.COMPONENT_HIST_BUDGET = max(pipeline.COMPONENT_HIST_BUDGET, row["surface_hist_bytes"])
                row["component_surface"] = timed(lambda: pipeline.component_surface(vol, connectivity=conn), a.warmup, a.reps)
                row["component_surface_largest"] = timed(lambda: pipeline.component_surface(vol, connectivity=conn, largest=True),
                                                         a.warmup, a.reps)
                row["surface_area_call"] = timed(lambda: pipeline.surface_area(vol), a.warmup, a.reps)
                torch.cuda.empty_cache()
                rows.append(row)
                print(json.dumps(row), flush=True)
            del vol
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
