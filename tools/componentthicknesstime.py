#!/usr/bin/env python3
"""Inscribed sphere and local thickness per component at n^3 (default 512), unit spacing, on the two volumes of
tools/cavitytime.py, resident as BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores -- one solid body,
and its pores as the cavities of the complement -- and seeded noise at 50 % -- millions of components.  HIP events around
warmed-up repeats, median / min / max, of
  * the passes on their own, on run tables labelled and selected once: tomo_cc_value_max and tomo_cc_value_first reading the
    float32 distance map and reading the float64 squared distances, tomo_cc_level_hist and tomo_cc_level_sums;
  * the whole of pipeline.component_thickness without and with --radii (labelling, selection, transform, host reads and the
    download included, as a caller pays them), and pipeline.cavity_sizes on the porous ellipsoid;
  * in the same run the whole-volume calls the new passes ride on: pipeline.inscribed_sphere, pipeline.distance_transform and
    pipeline.local_thickness with the same radii.  What component_thickness costs above them is the price of "per component";
and, as context only and once, scipy.ndimage.distance_transform_edt + label + maximum / maximum_position on the host (--host).
There is no time bar: the parent commit has no such path.

    python tools/componentthicknesstime.py [--n 512] [--warmup 1] [--reps 3] [--radii 1 1.5 2 3] [--host] [--out t.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cavitytime import porous_ellipsoid, timed  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402


def passes(vol, conn, radii, warmup, reps):
    """Event times of the value passes, the level histogram and its sums on tables labelled and selected once."""
    L, dev, st = _lib.lib(), vol.device, _stream()
    runs = pipeline.ComponentRuns(vol, conn)
    picked = runs.select()
    out = {"runs": runs.runs, "components": 0 if picked is None else picked.m}
    if picked is None:
        return out
    n, K = picked.table.shape[0], len(radii)
    out["hist_entries"] = picked.total
    plan = pipeline._DistancePlan(vol, None, 1.0, 1.0)
    dist = torch.empty(vol.shape, dtype=torch.float32, device=dev)
    _lib.check(L.tomo_edt_distance(*plan.head(), 1, _p(dist), *plan.tail()), "tomo_edt_distance")
    d2 = torch.empty(vol.shape, dtype=torch.float64, device=dev)
    _lib.check(L.tomo_edt_squared(*plan.head(), 1, _p(d2), *plan.tail()), "tomo_edt_squared")
    best = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int64, device=dev)
    head = (_p(runs.bits), *vol.shape, *runs._tables(), _p(runs.tot))
    for name, src in (("float32", (_p(dist), None)), ("float64", (None, _p(d2)))):
        out["value_max_" + name] = timed(lambda: _lib.check(L.tomo_cc_value_max(*head, *src, _p(best), n, st), "tomo_cc_value_max"),
                                         warmup, reps)
        out["value_first_" + name] = timed(lambda: _lib.check(L.tomo_cc_value_first(*head, *src, _p(best), _p(first), n, st),
                                                              "tomo_cc_value_first"), warmup, reps)
    del dist
    r2 = np.asarray(radii, dtype=np.float64) ** 2
    live = int(np.searchsorted(r2, float(d2.max().item()), side="right"))
    level_map = torch.zeros(vol.shape, dtype=torch.int32, device=dev)
    eroded = torch.empty_like(plan.bits)
    pipeline._thickness_levels(plan, d2, r2, live, level_map, eroded)
    del d2, eroded
    hist = torch.empty((K + 1) * picked.total, dtype=torch.int64, device=dev)
    out["hist_mib"] = round(hist.numel() * 8 / 2 ** 20, 1)
    out["level_hist"] = timed(lambda: _lib.check(L.tomo_cc_level_hist(*runs.hist_head(picked), _p(hist), picked.total, _p(level_map), K,
                                                                      st), "tomo_cc_level_hist"), warmup, reps)
    w = torch.ones(vol.shape[0], dtype=torch.float64, device=dev)
    voxels = torch.empty((picked.m, K + 1), dtype=torch.int64, device=dev)
    volume = torch.empty((picked.m, K), dtype=torch.float64, device=dev)
    labels = torch.empty(picked.m, dtype=torch.int64, device=dev)
    out["level_sums"] = timed(lambda: _lib.check(L.tomo_cc_level_sums(*runs.finish_head(picked), _p(hist), picked.total, _p(w),
                                                                      vol.shape[0], K, _p(voxels), _p(volume), _p(labels), picked.m,
                                                                      st), "tomo_cc_level_sums"), warmup, reps)
    if pipeline._download(runs.tot)[2]:
        sys.exit("a guard of the kernels fired")
    out["voxels_counted"] = int(voxels.sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--radii", type=float, nargs="+", default=[1.0, 1.5, 2.0, 3.0])
    ap.add_argument("--host", action="store_true", help="time SciPy's transform and per-label maxima on the host as well (context only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("componentthicknesstime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n, conn, radii = a.n, a.connectivity, list(a.radii)
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": lambda: porous_ellipsoid(n, a.pores, dev),
               "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
    rows = []
    for name, make in volumes.items():
        vol = pipeline.pack(make())
        row = {"n": n, "volume": name, "connectivity": conn, "radii_mm": radii, "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(passes(vol, conn, radii, a.warmup, a.reps))
        torch.cuda.empty_cache()
        t = pipeline.component_thickness(vol, connectivity=conn, radii_mm=radii)
        row["largest_radius_mm"] = round(float(t.radius_mm.max()), 4) if len(t) else 0.0
        row["uncovered_voxels"] = int(t.uncovered_voxels.sum())
        del t
        calls = {"component_thickness": lambda: pipeline.component_thickness(vol, connectivity=conn),
                 "component_thickness_radii": lambda: pipeline.component_thickness(vol, connectivity=conn, radii_mm=radii),
                 "component_properties": lambda: pipeline.component_properties(vol, connectivity=conn),
                 "inscribed_sphere": lambda: pipeline.inscribed_sphere(vol),
                 "distance_transform": lambda: pipeline.distance_transform(vol),
                 "local_thickness_radii": lambda: pipeline.local_thickness(vol, radii_mm=radii)}
        if name == "porous_ellipsoid":
            calls["cavity_sizes"] = lambda: pipeline.cavity_sizes(vol, connectivity=conn)
            calls["cavity_table"] = lambda: pipeline.cavity_table(vol, connectivity=conn)
        for key, fn in calls.items():
            row[key] = timed(fn, a.warmup, a.reps)
            torch.cuda.empty_cache()
        if a.host:
            from scipy import ndimage
            host = pipeline.unpack(vol).cpu().numpy().astype(bool)
            t0 = time.perf_counter()
            d = ndimage.distance_transform_edt(np.pad(host, 1))[1:-1, 1:-1, 1:-1]
            t1 = time.perf_counter()
            lab, k = ndimage.label(host, ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
            t2 = time.perf_counter()
            idx = np.arange(1, k + 1)
            ndimage.maximum(d, lab, idx)
            ndimage.maximum_position(d, lab, idx)
            t3 = time.perf_counter()
            row["host_ms"] = {"distance_transform_edt": round(1e3 * (t1 - t0), 1), "label": round(1e3 * (t2 - t1), 1),
                              "maximum_and_position": round(1e3 * (t3 - t2), 1)}
            del host, d, lab
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
