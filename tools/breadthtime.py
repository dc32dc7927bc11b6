#!/usr/bin/env python3
"""Crofton mean breadth at n^3 (default 512), unit spacing, on the two volumes of tools/cavitytime.py, resident as BitVolumes:
the benchmark's ellipsoid with a few hundred spherical pores -- one solid body, the wave-combined path of the kernels -- and
seeded noise at 50 % -- millions of components, the divergent path, of which those of at least --noise-min-voxels voxels are
selected.  HIP events around warmed-up repeats, median / min / max, of
  * tomo_cc_breadth_hist without tables (pipeline.mean_breadth's first launch: 18 words per slice of the volume),
  * tomo_cc_breadth_hist on run tables labelled and selected once (18 words per slice of every selected component's box),
  * tomo_cc_surface_hist on the same tables and the same selection in the same run -- nine row windows into eleven counters
    against five windows into 18: the yardstick -- and the ratio of the medians,
  * tomo_cc_breadth, the finishing kernel, on those entries,
  * the whole of pipeline.component_breadth (labelling, selection, both kernels, the host reads and the download), of
    pipeline.mean_breadth (two launches, one host read) and, on the ellipsoid, of pipeline.cavity_breadth.
The section Euler numbers of the selected components are checked against the unlabelled ones where every component is selected.
There is no time bar: the parent commit has no such path.

    python tools/breadthtime.py [--n 512] [--warmup 2] [--reps 5] [--density 0.5] [--pores 300] [--noise-min-voxels 8] [--out t.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cavitytime import porous_ellipsoid, timed  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402


def device_steps(vol, conn, min_voxels, warmup, reps):
    """Event times of the breadth pass (with and without tables), of the surface pass on the same tables and of the finishing
    kernel, on run tables labelled and selected once."""
    nz, ny, nx = vol.shape
    L, dev, st = _lib.lib(), vol.device, _stream()
    cr = pipeline.ComponentRuns(vol, conn)
    picked = cr.select(min_voxels, False)
    out = {"runs": cr.runs, "components": cr.n, "selected": 0 if picked is None else picked.m}
    if picked is None:
        return out
    total, m = picked.total, picked.m
    W = pipeline.BREADTH_WORDS
    geo = (_p(cr.bits), nz, ny, nx)
    hist_head, finish_head = cr.hist_head(picked), cr.finish_head(picked)
    whole = torch.empty(W * nz, dtype=torch.int64, device=dev)
    hist = torch.empty(W * total, dtype=torch.int64, device=dev)
    surf = torch.empty(pipeline.SURFACE_COUNTERS * total, dtype=torch.int64, device=dev)
    tab = torch.from_numpy(pipeline.breadth_factors(None, nz)).to(dev)
    breadth = torch.empty(m, dtype=torch.float64, device=dev)
    euler = torch.empty((m, pipeline.BREADTH_FAMILIES), dtype=torch.int64, device=dev)
    labels = torch.empty(m, dtype=torch.int64, device=dev)
    steps = {
        "breadth_hist_whole_volume": lambda: _lib.check(L.tomo_cc_breadth_hist(*geo, None, 0, None, None, None, None, 0, None, None,
                                                                               _p(whole), nz, st), "tomo_cc_breadth_hist"),
        "breadth_hist_per_component": lambda: _lib.check(L.tomo_cc_breadth_hist(*hist_head, _p(hist), total, st), "tomo_cc_breadth_hist"),
        "surface_hist_per_component": lambda: _lib.check(L.tomo_cc_surface_hist(*hist_head, _p(surf), total, st), "tomo_cc_surface_hist"),
        "breadth_finish": lambda: _lib.check(L.tomo_cc_breadth(*finish_head, _p(hist), total, _p(tab), nz, 13, _p(breadth), _p(euler),
                                                               _p(labels), m, st), "tomo_cc_breadth"),
    }
    out.update({"slice_entries": total, "breadth_hist_bytes": 8 * W * total})
    for name, fn in steps.items():
        out[name] = timed(fn, warmup, reps)
    out["breadth_hist_over_surface_hist"] = round(out["breadth_hist_per_component"]["median_ms"]
                                                  / max(out["surface_hist_per_component"]["median_ms"], 1e-3), 2)
    if pipeline._download(cr.tot)[2]:
        sys.exit("a guard of the kernels fired")
    out["section_euler"] = [int(x) for x in euler.sum(dim=0).cpu()]
    if m == cr.n and not torch.equal(hist.view(total, W).sum(dim=0), whole.view(nz, W).sum(dim=0)):
        sys.exit("the components' entries do not add up to the volume's")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--noise-min-voxels", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("breadthtime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n, conn = a.n, a.connectivity
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (0, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_min_voxels, lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name, (min_voxels, make) in volumes.items():
        vol = pipeline.pack(make())
        row = {"n": n, "volume": name, "connectivity": conn, "min_voxels": min_voxels,
               "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(device_steps(vol, conn, min_voxels, a.warmup, a.reps))
        torch.cuda.empty_cache()
        whole = pipeline.mean_breadth(vol)
        row["mean_breadth_unit_spacing"] = whole.mean_breadth_mm
        if min_voxels == 0 and whole.section_euler.tolist() != row.get("section_euler"):
            sys.exit("pipeline.mean_breadth disagrees with the per-component numbers")
        calls = {"component_breadth": lambda: pipeline.component_breadth(vol, connectivity=conn, min_voxels=min_voxels),
                 "component_breadth_largest": lambda: pipeline.component_breadth(vol, connectivity=conn, largest=True),
                 "component_surface": lambda: pipeline.component_surface(vol, connectivity=conn, min_voxels=min_voxels),
                 "mean_breadth_call": lambda: pipeline.mean_breadth(vol)}
        if name == "porous_ellipsoid":
            calls["cavity_breadth"] = lambda: pipeline.cavity_breadth(vol, connectivity=conn)
        for key, fn in calls.items():
            try:
                row[key] = timed(fn, a.warmup, a.reps)
            except _lib.TomoError as e:
                row[key] = {"error": str(e)[:200]}
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
