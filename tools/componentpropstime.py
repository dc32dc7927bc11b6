#!/usr/bin/env python3
"""Per-component measurements at n^3 (default 512) on two volumes, resident as BitVolumes: the benchmark's ellipsoid -- one
component, the wave-combined path of the kernels -- and seeded noise at 25 % -- millions of components, the divergent path.
HIP events around each of the four device steps (tomo_cc_measure, tomo_cc_zhist_offsets, tomo_cc_zhist, tomo_cc_zsums) on
tables labelled once, a host clock around pipeline.component_properties (labelling, four host reads and the downloads
included: it ends with the results on the host), and the CPU route on the same volume where SciPy imports: the label array
downloaded (its transfer timed apart), scipy.ndimage.label + find_objects + center_of_mass on it.  The CPU route stops short
of the volume in mm^3, which would take one pass over the whole array per component.

--moments times the second-moment chain on the same volumes and the same labelled tables, in the same run: HIP events around
tomo_cc_moment_hist (memset + the pass over the runs, six atomics where tomo_cc_zhist issues one) and tomo_cc_moments (one
thread per component: two walks over its slices and the 3 x 3 Jacobi iteration), a host clock around
pipeline.component_moments, and moment_hist / zhist as a ratio of the medians.

    python tools/componentpropstime.py [--n 512] [--warmup 2] [--reps 7] [--density 0.25] [--no-scipy] [--moments] [--out props.json]
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


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def device_steps(vol, depths, warmup, reps, moments=False):
    """Event times of the four steps for min_voxels = 0 (every component selected) on run tables labelled once; moments: of
    the two steps of the second-moment chain as well, on the same tables."""
    nz, ny, nx = vol.shape
    L, dev, st = _lib.lib(), vol.device, _stream()
    cr = pipeline.ComponentRuns(vol)
    n = cr._checked()
    geo = (_p(cr.bits), nz, ny, nx)
    table = torch.empty((n, pipeline.TABLE_COLUMNS), dtype=torch.int64, device=dev)
    sel = torch.empty(n, dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    slot = torch.empty(n, dtype=torch.int32, device=dev)
    blk = torch.empty(2 * L.tomo_cc_scan_blocks(n), dtype=torch.int64, device=dev)
    zt, _, _ = pipeline.distance_positions(depths, nz)
    tab = torch.from_numpy(np.concatenate([np.asarray(depths, dtype=np.float64), zt[1:-1]])).to(dev)
    steps = {
        "measure": lambda: L.tomo_cc_measure(*geo, *cr._tables(), _p(cr.tot), _p(table), n, st),
        "zhist_offsets": lambda: L.tomo_cc_zhist_offsets(_p(table), n, _p(cr.tot), 0, 0, _p(sel), _p(off), _p(slot), _p(blk), st),
    }
    for fn in steps.values():
        _lib.check(fn(), "step")
    host = pipeline._download(cr.tot)
    total, m = host[4], host[5]
    hist = torch.empty(total, dtype=torch.int64, device=dev)
    sums = torch.empty((m, 2), dtype=torch.float64, device=dev)
    labels = torch.empty(m, dtype=torch.int64, device=dev)
    picked = pipeline.ComponentSelection(table, sel, off, slot, total, m)
    hist_head, finish_head = cr.hist_head(picked), cr.finish_head(picked)
    steps["zhist"] = lambda: L.tomo_cc_zhist(*hist_head, _p(hist), total, st)
    steps["zsums"] = lambda: L.tomo_cc_zsums(*finish_head, _p(hist), total, _p(tab[:nz]), _p(tab[nz:]), nz, _p(sums), _p(labels), m, st)
    if moments:
        mom = torch.empty(pipeline.MOMENT_SUMS * total, dtype=torch.int64, device=dev)
        rows = torch.empty((m, pipeline.MOMENT_COLUMNS), dtype=torch.float64, device=dev)
        steps["moment_hist"] = lambda: L.tomo_cc_moment_hist(*hist_head, _p(mom), total, st)
        steps["moments"] = lambda: L.tomo_cc_moments(*finish_head, _p(mom), total, _p(tab[:nz]), _p(tab[nz:]), nz, 0.45, 0.7, _p(rows),
                                                     _p(labels), m, st)
    out = {"runs": cr.runs, "components": n, "selected": m, "hist_entries": total}
    for name, fn in steps.items():
        for _ in range(warmup):
            _lib.check(fn(), name)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(fn(), name)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name] = spread(ms)
    if moments:
        out["moment_hist_over_zhist"] = round(out["moment_hist"]["median_ms"] / max(out["zhist"]["median_ms"], 1e-3), 2)
    flags = pipeline._download(cr.tot)[2]
    if flags:
        sys.exit("a guard of the kernels fired (flags %d)" % flags)
    return out


def host_to_host(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return spread(ms)


def cpu_route(vol, components):
    try:
        from scipy import ndimage
    except ImportError:
        return "SciPy is not installed here"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev_labels, _ = pipeline.label_components(vol)
    host_labels = dev_labels.cpu().numpy()
    t1 = time.perf_counter()
    del dev_labels
    mask = host_labels != 0
    t2 = time.perf_counter()
    lab, count = ndimage.label(mask)
    t3 = time.perf_counter()
    assert count == components, (count, components)
    boxes = ndimage.find_objects(lab)
    t4 = time.perf_counter()
    com = ndimage.center_of_mass(mask, lab, np.arange(1, count + 1))
    t5 = time.perf_counter()
    assert len(boxes) == count and len(com) == count
    return {"label_components_and_download_s": round(t1 - t0, 3), "scipy_label_s": round(t3 - t2, 3),
            "scipy_find_objects_s": round(t4 - t3, 3), "scipy_center_of_mass_s": round(t5 - t4, 3),
            "scipy_total_s": round(t5 - t2, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU route (tens of seconds per volume at 512^3)")
    ap.add_argument("--moments", action="store_true", help="time the second-moment chain (tomo_cc_moment_hist, tomo_cc_moments) too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("componentpropstime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.n:
        depths = np.linspace(0.3, 1.7, n)
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        volumes = {"ellipsoid": lambda: pipeline.ellipsoid_mask(n, n, n, dev),
                   "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
        for name, make in volumes.items():
            vol = pipeline.pack(make())
            row = {"n": n, "volume": name, "set_voxels": int(pipeline.popcount_async(vol).item())}
            row.update(device_steps(vol, depths, a.warmup, a.reps, a.moments))
            torch.cuda.empty_cache()
            row["component_properties_host_to_host"] = host_to_host(
                lambda: pipeline.component_properties(vol, depths, 0.45, 0.7), a.warmup, a.reps)
            row["component_properties_largest_host_to_host"] = host_to_host(
                lambda: pipeline.component_properties(vol, depths, 0.45, 0.7, largest=True), a.warmup, a.reps)
            if a.moments:
                row["component_moments_host_to_host"] = host_to_host(
                    lambda: pipeline.component_moments(vol, depths, 0.45, 0.7), a.warmup, a.reps)
                row["component_moments_largest_host_to_host"] = host_to_host(
                    lambda: pipeline.component_moments(vol, depths, 0.45, 0.7, largest=True), a.warmup, a.reps)
            if not a.no_scipy:
                row["cpu_route"] = cpu_route(vol, row["components"])
            del vol
            torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
