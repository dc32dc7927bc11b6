#!/usr/bin/env python3
"""Components across Z-slabs at n^3 (default 512 and 1024): the speckled ellipsoid of tools/componentstime.py, cut into equal
slabs for 2, 4 and 8 rank THREADS that share this card (slab.ThreadComm), every rank on a stream of its own.  Per rank: HIP-event
time of SlabComponents(...).keep(min_voxels), split at the marks the class records (local labelling | seam steps: the three
collective steps and the merge | filter), and the bytes the rank handed to the communicator.  The yardstick, same volume, same
run: pipeline.keep_components of the whole volume.  Rank threads on one card share its CUs and copy messages inside device
memory: the numbers say what the protocol costs in kernels and host reads and NOTHING about link time.

    python tools/slabcomponentstime.py [--n 512 1024] [--worlds 2 4 8] [--warmup 1] [--reps 5] [--min-voxels 64] [--out x.json]
"""
import argparse
import json
import os
import sys
import threading

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomography_3d_reconstructor_amd import pipeline, slab  # noqa: E402
from tomography_3d_reconstructor_amd.slab_components import SlabComponents  # noqa: E402
from componentstime import timed  # noqa: E402


def on_ranks(comms, fn, timeout=600):
    out, errs = [None] * len(comms), []

    def target(c):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                out[c.rank] = fn(c)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            raise
    ts = [threading.Thread(target=target, args=(c,)) for c in comms]
    [t.start() for t in ts]
    [t.join(timeout) for t in ts]
    if any(t.is_alive() for t in ts) or errs:
        raise RuntimeError("a rank failed or is still waiting: %r" % (errs,))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--speckle", type=float, default=0.001)
    ap.add_argument("--min-voxels", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slabcomponentstime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.n:
        mask = pipeline.ellipsoid_mask(n, n, n, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        mask = (mask.view(torch.bool) ^ (torch.rand((n, n, n), device=dev, generator=gen) < a.speckle)).view(torch.uint8)
        vol = pipeline.close_ends(pipeline.pack(mask), inplace=True)
        del mask
        whole = pipeline.keep_components(vol, a.min_voxels)
        row = {"n": n, "components": int(pipeline.component_sizes(vol).shape[0]), "min_voxels": a.min_voxels,
               "pipeline.keep_components(whole)": timed(lambda: pipeline.keep_components(vol, a.min_voxels), a.warmup, a.reps)}
        for world in a.worlds:
            cuts = [n * k // world for k in range(world + 1)]
            vols = [pipeline.BitVolume(vol.bits[z0:z1], (z1 - z0, n, n)) for z0, z1 in zip(cuts, cuts[1:])]
            comms = slab.ThreadComm.make(world)

            def one(c, vols=vols):
                ev = []
                sc = SlabComponents(vols[c.rank], c, events=ev)
                kept = sc.keep(a.min_voxels)
                torch.cuda.current_stream().synchronize()
                t = {k: e for k, e in ev}
                ms = {"local_ms": t["start"].elapsed_time(t["local"]), "seam_ms": t["local"].elapsed_time(t["merge"]),
                      "filter_ms": t["filter_start"].elapsed_time(t["filter"]), "total_ms": t["start"].elapsed_time(t["filter"])}
                return ms, sc.bytes_published, sc.n, kept
            for _ in range(a.warmup):
                on_ranks(comms, one)
            reps = [on_ranks(comms, one) for _ in range(a.reps)]
            same = torch.equal(torch.cat([r[3].bits for r in reps[-1]]), whole.bits)
            per_rank = []
            for r in range(world):
                med = {k: round(float(np.median([rep[r][0][k] for rep in reps])), 3) for k in reps[0][r][0]}
                med["bytes_published"] = reps[0][r][1]
                per_rank.append(med)
            row["world_%d" % world] = {"equal_to_whole_volume": bool(same), "n": reps[0][0][2], "ranks": per_rank}
            del reps, vols
        del vol, whole
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
