#!/usr/bin/env python3
"""The two-point covariance at n^3 (default 512), unit spacing, on the two volumes of tools/chordtime.py, resident as BitVolumes:
the benchmark's ellipsoid with a few hundred spherical pores -- half of its words are empty, the zero-word skip has something to
skip -- and seeded noise at 50 % -- no word is empty.  For max_lag 8, 16 and 32 (the kernel's variants of 17, 33 and 65 lags a
plane; --lags 63 for the fourth), HIP events around warmed-up repeats, median / min / max, of
  * tomo_two_point (the table zeroed by the call),
  * the whole of pipeline.two_point (the launch, one host read, the host arithmetic of the dataclass),
and, once per volume in the same run,
  * tomo_chord_hist, the other whole-structure pass,
  * the comparator a user would otherwise write: the zero-padded float64 torch.fft.rfftn autocorrelation of the unpacked volume
    on the same device, cropped to the box and rounded (not part of the package; --no-fft leaves it out, it takes 8 bytes a
    padded voxel twice over).  Its table is compared with the kernel's.
From the sizes: words * lags, the workgroups and the global atomics of the call at the most (one per workgroup and lag of the
box), and the achieved rate words * lags / time.
There is no time bar: the parent commit has no such path.

    python tools/twopointtime.py [--n 512] [--lags 8 16 32] [--warmup 2] [--reps 5] [--density 0.5] [--pores 300] [--no-fft] [--out t.json]
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

GRID, CHUNK_MAX, THREADS = 8192, 1 << 24, 256                    # csrc/two_point.hip: TWO_POINT_GRID, _CHUNK_MAX, _THREADS


def launch_shape(shape, box):
    """(planes, chunks) of tomo_two_point's grid: the launcher's arithmetic, repeated."""
    nz, ny, nx = shape
    words = nz * ny * ((nx + 63) // 64)
    planes = (min(box[0], nz - 1) + 1) * (2 * min(box[1], ny - 1) + 1)
    chunks = min(max(-(-GRID // planes), -(-words // CHUNK_MAX)), -(-words // THREADS), 65535)
    chunk = -(-(-(-words // chunks)) // THREADS) * THREADS
    return planes, -(-words // chunk)


def fft_pairs(vol, box):
    """The comparator: the zero-padded float64 autocorrelation of the unpacked volume, cropped to the box, rounded -> int64."""
    rz, ry, rx = box
    v = pipeline.unpack(vol).to(torch.float64)
    size = tuple(n + r for n, r in zip(vol.shape, box))
    f = torch.fft.rfftn(v, s=size)
    del v
    c = torch.fft.irfftn(f * f.conj(), s=size)
    del f
    z = torch.arange(rz + 1, device=c.device)
    y = torch.arange(-ry, ry + 1, device=c.device) % size[1]
    x = torch.arange(-rx, rx + 1, device=c.device) % size[2]
    return torch.round(c[z[:, None, None], y[None, :, None], x[None, None, :]]).to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--lags", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--no-fft", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("twopointtime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": lambda: porous_ellipsoid(n, a.pores, dev),
               "noise": lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8)}
    L, st = _lib.lib(), _stream()
    rows = []
    for name, make in volumes.items():
        vol = pipeline.pack(make())
        nz, ny, nx = vol.shape
        words = nz * ny * ((nx + 63) // 64)
        geo = (_p(vol.bits), nz, ny, nx)
        row = {"n": n, "volume": name, "set_voxels": int(pipeline.popcount_async(vol).item()), "words": words,
               "empty_words": int((vol.bits == 0).sum().item())}
        lmax = max(vol.shape)
        cells = pipeline.CHORD_DIRECTIONS * (lmax + 1)
        tables = torch.zeros(3 * cells, dtype=torch.int64, device=dev)
        tab = torch.from_numpy(pipeline.chord_steps_q(pipeline.chord_steps(None, nz))).to(dev)
        row["chord_hist"] = timed(lambda: _lib.check(L.tomo_chord_hist(*geo, _p(tab), lmax, _p(tables), _p(tables[cells:]),
                                                                       _p(tables[2 * cells:]), st), "tomo_chord_hist"), a.warmup, a.reps)
        del tables
        for r in a.lags:
            box = pipeline.two_point_box(r)
            lags = (box[0] + 1) * (2 * box[1] + 1) * (2 * box[2] + 1)
            out = torch.empty(lags, dtype=torch.int64, device=dev)
            k = timed(lambda: _lib.check(L.tomo_two_point(*geo, *box, _p(out), st), "tomo_two_point"), a.warmup, a.reps)
            planes, chunks = launch_shape(vol.shape, box)
            got = out.cpu().numpy().reshape(box[0] + 1, 2 * box[1] + 1, 2 * box[2] + 1)
            if got[0, box[1], box[2]] != row["set_voxels"] or not np.array_equal(got[0], got[0, ::-1, ::-1]):
                sys.exit("N(0) is not the popcount, or the plane hz = 0 is not symmetric")
            one = {"max_lag": r, "lags": lags, "word_lags": words * lags, "workgroups": planes * chunks,
                   "global_atomics_at_most": planes * chunks * (2 * box[2] + 1), "kernel": k,
                   "word_lags_per_ns": round(words * lags / (k["median_ms"] * 1e6), 3),
                   "call": timed(lambda: pipeline.two_point(vol, box), a.warmup, a.reps),
                   "kernel_over_chord_hist": round(k["median_ms"] / max(row["chord_hist"]["median_ms"], 1e-3), 2)}
            if not a.no_fft:
                torch.cuda.empty_cache()
                one["fft"] = timed(lambda: fft_pairs(vol, box), 1, max(2, a.reps // 2))
                one["fft_over_kernel"] = round(one["fft"]["median_ms"] / max(k["median_ms"], 1e-3), 2)
                one["fft_equals_the_kernel"] = bool(np.array_equal(fft_pairs(vol, box).cpu().numpy(), got))
                torch.cuda.empty_cache()
            row["max_lag_%d" % r] = one
            del out
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
