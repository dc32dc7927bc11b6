#!/usr/bin/env python3
"""Chord lengths at n^3 (default 512), unit spacing, on the two volumes of tools/cavitytime.py, resident as BitVolumes: the
benchmark's ellipsoid with a few hundred spherical pores -- few, long chords: every line holds a handful -- and seeded noise at
50 % -- about n^3 / 4 chords per direction, three in four of one or two voxels -- and on an empty volume of the same size, where
the walk runs and no chord is filed.  HIP events around warmed-up repeats, median / min / max, of
  * tomo_chord_hist (all 13 directions, the tables zeroed by the call),
  * tomo_cc_surface_hist and tomo_cc_breadth_hist without tables -- the existing whole-volume passes that also look along all 13
    directions, one step ahead -- in the same run, and the ratios of the medians,
  * the whole of pipeline.chord_lengths for both phases (the steps, the launches, one host read, the host arithmetic).
From the tables: chords per direction, the share of chords of CHORD_LDS_BINS voxels or more -- they share the direct-mapped
slots of a workgroup, and the ones that find their slot taken are all that goes straight to the tables: an upper bound of the
global path -- and the share that was counted in registers (interior chords of one or two voxels).  The invariant is checked on
every volume.
There is no time bar: the parent commit has no such path.

    python tools/chordtime.py [--n 512] [--warmup 3] [--reps 9] [--density 0.5] [--pores 300] [--out t.json]
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
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402


def device_steps(vol, warmup, reps):
    """Event times of the chord pass and of the two one-step passes over the same bits."""
    nz, ny, nx = vol.shape
    L, dev, st = _lib.lib(), vol.device, _stream()
    lmax = max(vol.shape)
    cells = pipeline.CHORD_DIRECTIONS * (lmax + 1)
    tables = torch.zeros(3 * cells, dtype=torch.int64, device=dev)
    tab = torch.from_numpy(pipeline.chord_steps_q(pipeline.chord_steps(None, nz))).to(dev)
    surf = torch.empty(pipeline.SURFACE_COUNTERS * nz, dtype=torch.int64, device=dev)
    hist = torch.empty(pipeline.BREADTH_WORDS * nz, dtype=torch.int64, device=dev)
    geo = (_p(vol.bits), nz, ny, nx)
    steps = {
        "chord_hist": lambda: _lib.check(L.tomo_chord_hist(*geo, _p(tab), lmax, _p(tables), _p(tables[cells:]), _p(tables[2 * cells:]), st),
                                         "tomo_chord_hist"),
        "surface_hist_whole_volume": lambda: _lib.check(L.tomo_cc_surface_hist(*geo, None, 0, None, None, None, None, 0, None, None,
                                                                               _p(surf), nz, st), "tomo_cc_surface_hist"),
        "breadth_hist_whole_volume": lambda: _lib.check(L.tomo_cc_breadth_hist(*geo, None, 0, None, None, None, None, 0, None, None,
                                                                               _p(hist), nz, st), "tomo_cc_breadth_hist"),
    }
    out = {name: timed(fn, warmup, reps) for name, fn in steps.items()}
    for other in ("surface_hist_whole_volume", "breadth_hist_whole_volume"):
        out["chord_hist_over_" + other] = round(out["chord_hist"]["median_ms"] / max(out[other]["median_ms"], 1e-3), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chordtime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": lambda: porous_ellipsoid(n, a.pores, dev),
               "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8),
               "empty": lambda: torch.zeros((n, n, n), dtype=torch.uint8, device=dev)}
    rows = []
    for name, make in volumes.items():
        vol = pipeline.pack(make())
        row = {"n": n, "volume": name, "set_voxels": int(pipeline.popcount_async(vol).item())}
        row.update(device_steps(vol, a.warmup, a.reps))
        torch.cuda.empty_cache()
        c = pipeline.chord_lengths(vol)
        lengths = np.arange(c.counts.shape[1])
        if c.voxels != row["set_voxels"] or ((c.counts * lengths).sum(axis=1) != c.voxels).any():
            sys.exit("the chords do not add up to the voxels")
        total = max(int(c.chords.sum()), 1)
        inner = c.counts - c.border
        row["chords_per_direction"] = c.chords.tolist()
        row["longest_chord_voxels"] = int(lengths[c.counts.any(axis=0)].max()) if c.voxels else 0
        row["share_beyond_the_bins"] = float(c.counts[:, pipeline.CHORD_LDS_BINS:].sum() / total)
        row["share_counted_in_registers"] = float(inner[:, 1:3].sum() / total)
        row["mean_chord_voxels"] = [round(float(x), 3) for x in c.mean_chord_mm]
        if c.voxels:
            try:
                row["degree_of_anisotropy"] = c.fabric()["degree_of_anisotropy"]
            except ValueError as e:
                row["degree_of_anisotropy"] = str(e)
        for phase in pipeline.CHORD_PHASES:
            row["chord_lengths_call_" + phase] = timed(lambda: pipeline.chord_lengths(vol, phase=phase), a.warmup, a.reps)
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
