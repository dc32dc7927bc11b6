#!/usr/bin/env python3
"""Local thickness at n^3 (default 512), unit spacing (1 mm voxels), resident as a BitVolume.  HIP events around warmed-up
repeats, median of --reps after --warmup calls, of

  solid   the ellipsoid of the benchmark, pipeline.local_thickness with 16 evenly spaced radii up to the inscribed radius: the
          whole call (its host reads included, as a caller pays them) and ONE level on its own (tomo_edt_at_least +
          tomo_edt_cover at the 8th radius, no host read);
  shell   the same ellipsoid minus its 4 mm erosion, a thin wall, in exact mode (every distinct squared distance a level): the
          whole call and one level;
  pipeline.distance_transform on the same volumes: the unit a level is to be read against (a level is one outside transform of
  a bit volume plus a ballot pass).

Peak device memory of each call above what was allocated before it.  There is no time bar: the parent commit has no such path.

    python tools/thicknesstime.py [--n 512] [--warmup 2] [--reps 5] [--out thickness.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402

LEVELS = 16
WALL_MM = 4.0


def timed(fn, warmup, reps):
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
            "peak_mib": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)}


def one_level(vol, r2, warmup, reps):
    """The two launches of a level on their own: the eroded set as bits, then its outside transform with the cover tail."""
    L = _lib.lib()
    plan = pipeline._DistancePlan(vol, None, 1.0, 1.0)
    d2 = torch.empty(vol.shape, dtype=torch.float64, device=vol.device)
    _lib.check(L.tomo_edt_squared(*plan.head(), 1, d2.data_ptr(), *plan.tail()), "tomo_edt_squared")
    eroded = torch.empty_like(plan.bits)
    level_map = torch.zeros(vol.shape, dtype=torch.int32, device=vol.device)
    head = plan.head()

    def level():
        _lib.check(L.tomo_edt_at_least(d2.data_ptr(), head[0], *head[1:4], r2, eroded.data_ptr(), plan.tail()[2]), "tomo_edt_at_least")
        _lib.check(L.tomo_edt_cover(eroded.data_ptr(), head[0], *head[1:4], *head[4:], r2, 1, level_map.data_ptr(), *plan.tail()),
                   "tomo_edt_cover")
    return timed(level, warmup, reps)


def summary(t):
    return {"levels": len(t.radii_mm), "levels_hit": int((t.level_voxels > 0).sum()), "uncovered_voxels": t.uncovered_voxels,
            "mean_mm": round(t.mean_mm, 4), "std_mm": round(t.std_mm, 4), "max_mm": round(t.max_mm, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("thicknesstime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    solid = pipeline.pack(pipeline.ellipsoid_mask(n, n, n, dev))
    core = pipeline.offset_volume(solid, -WALL_MM)
    shell = pipeline.BitVolume(solid.bits & ~core.bits, solid.shape)             # solid's tail bits are zero: so are these
    del core
    radius = pipeline.inscribed_sphere(solid)[0]
    radii = [radius * (k + 1) / LEVELS for k in range(LEVELS)]
    ws = int(_lib.lib().tomo_edt_workspace_bytes(n, n, n, pipeline.EDT_WORKSPACE_BUDGET))
    out = {"n": n, "spacing_mm": 1.0, "workspace_mib": round(ws / 2 ** 20, 1),
           "d2_mib": round(8 * n ** 3 / 2 ** 20, 1), "result_mib": round(4 * n ** 3 / 2 ** 20, 1)}
    for name, vol, kw, r2 in (("solid", solid, {"radii_mm": radii}, radii[LEVELS // 2 - 1] ** 2), ("shell", shell, {}, 2.0)):
        row = {"set_voxels": int(pipeline.popcount_async(vol).item())}
        if name == "solid":
            row["inscribed_radius_mm"] = round(radius, 4)
        row.update(summary(pipeline.local_thickness(vol, **kw)))
        row["local_thickness"] = timed(lambda: pipeline.local_thickness(vol, **kw), a.warmup, a.reps)
        row["one_level"] = dict(one_level(vol, float(r2), a.warmup, a.reps), r2=round(float(r2), 4))
        row["distance_transform"] = timed(lambda: pipeline.distance_transform(vol), a.warmup, a.reps)
        row["opening_volume"] = dict(timed(lambda: pipeline.opening_volume(vol, float(np.sqrt(r2))), a.warmup, a.reps),
                                     radius_mm=round(float(np.sqrt(r2)), 4))
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
