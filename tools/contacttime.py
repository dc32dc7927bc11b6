#!/usr/bin/env python3
"""The contact table between zones at n^3 (default 512), unit spacing, on the two cases of tools/zonetime.py, resident as
BitVolumes: the benchmark's ellipsoid with a few hundred spherical pores separated at --radius, and seeded noise at 50 %
separated at --noise-radius.  The zones and their distance map are pipeline.geodesic_zones of the ball erosion, the value map is
pipeline.distance_transform.  For each volume and each connectivity of the zones, in ONE run
  * pipeline.zone_contacts taken apart into its five steps -- tomo_contact_count, tomo_contact_insert, the host plumbing in torch
    (occupied slots, sort, row of slot, offsets, the one host read), tomo_contact_hist, tomo_contact_finish -- each with HIP
    events, and N (contact pairs), P (zone pairs), the slots and the load P / slots of the hash table;
  * tomo_zone_cut on the same bits and the same map: it reads the same bytes in the same pattern, so it is the yardstick of a
    walk.  walk_over_cut is the time of each of the three walks over the cut's: written down, not promised;
  * the whole of pipeline.zone_contacts (host reads included), with and without the value and distance maps.
HIP events, median / min / max of --reps after --warmup calls.  There is no time bar: the parent commit has no such path.

    python tools/contacttime.py [--n 512] [--warmup 1] [--reps 3] [--radius 8] [--noise-radius 1] [--out t.json]
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
from tomography_3d_reconstructor_amd.pipeline import _download, _p, _stream  # noqa: E402


def steps(vol, zones, values, dist, warmup, reps):
    """pipeline._zone_contacts step by step -> the row.  Every step is timed on the buffers the step before it left."""
    L, dev = _lib.lib(), vol.device
    nz, ny, nx = vol.shape
    head = (_p(vol.bits), _p(zones), nz, ny, nx)
    tables = pipeline._geodesic_tables(vol.shape, None, 1.0, 1.0)
    F = torch.from_numpy(pipeline.surface_factors(None, nz)).to(dev)
    wxy, wz = torch.from_numpy(tables.wxy).to(dev), torch.from_numpy(np.ascontiguousarray(tables.wz)).to(dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)

    def run_count():
        _lib.check(L.tomo_contact_count(*head, _p(count), _stream()), "tomo_contact_count")
    row = {"count": timed(run_count, warmup, reps)}
    pairs = int(count.item())
    row["contact_pairs"] = pairs
    if pairs == 0:
        return row
    cap = pipeline._contact_capacity(pairs)
    keys, total, first = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(3))
    z_lo, z_hi, top, path = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(4))
    counters = torch.zeros(2, dtype=torch.int64, device=dev)

    def run_insert():
        _lib.check(L.tomo_contact_insert(*head, _p(values), _p(dist), _p(wxy), _p(wz), cap, _p(keys), _p(total), _p(z_lo), _p(z_hi),
                                         _p(first), _p(top), _p(path), _p(counters), _stream()), "tomo_contact_insert")
    row["insert"] = timed(run_insert, warmup, reps)
    laid = {}

    def run_host():
        taken = keys != 0
        span = (z_hi - z_lo + 1).to(torch.int64) * taken                   # an empty slot counts for nothing
        rows, lost, entries = _download(torch.stack([taken.sum(), counters[0], span.sum()]))
        slots = taken.nonzero_static(size=rows).reshape(-1)
        order = keys[slots].sort()[1]
        slot_of_row = slots[order].to(torch.int32)
        row_of_slot = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        row_of_slot[slot_of_row.long()] = torch.arange(rows, dtype=torch.int32, device=dev)
        length = span[slot_of_row.long()]
        laid.update(rows=rows, lost=lost, entries=entries, slot_of_row=slot_of_row, row_of_slot=row_of_slot,
                    offset=(length.cumsum(0) - length).contiguous())
    row["host_plumbing"] = timed(run_host, warmup, reps)
    rows, entries = laid["rows"], laid["entries"]
    row.update(zone_pairs=rows, slots=cap, load=round(rows / cap, 6), slot_bytes=cap * pipeline.CONTACT_SLOT_BYTES,
               slice_entries=entries, overflowed=bool(laid["lost"]))
    if laid["lost"] or entries * pipeline.CONTACT_ENTRY_BYTES > pipeline.COMPONENT_HIST_BUDGET:
        return row
    hist = torch.empty(entries * pipeline.SURFACE_CLASSES, dtype=torch.int64, device=dev)
    where = torch.empty(rows, dtype=torch.int64, device=dev)

    def run_hist():
        _lib.check(L.tomo_contact_hist(*head, _p(values), cap, _p(keys), _p(laid["row_of_slot"]), _p(z_lo), _p(top), _p(laid["offset"]),
                                       rows, _p(hist), entries, _p(where), _p(counters), _stream()), "tomo_contact_hist")
    row["hist"] = timed(run_hist, warmup, reps)
    out = torch.empty(rows * pipeline.CONTACT_COLUMNS, dtype=torch.int64, device=dev)

    def run_finish():
        _lib.check(L.tomo_contact_finish(rows, _p(laid["slot_of_row"]), cap, _p(keys), _p(total), _p(z_lo), _p(z_hi), _p(first), _p(top),
                                         _p(path), _p(where), _p(laid["offset"]), _p(hist), entries, _p(F), nz, 13, _p(out), _p(counters),
                                         _stream()), "tomo_contact_finish")
    row["finish"] = timed(run_finish, warmup, reps)
    row["pairs_without_a_row"] = int(counters[1].item())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--pores", type=int, default=300)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--noise-radius", type=float, default=1.0)
    ap.add_argument("--connectivities", type=int, nargs="+", default=[6, 26])
    ap.add_argument("--volumes", nargs="+", default=["porous_ellipsoid", "noise"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("contacttime needs a GPU: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    n = a.n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    volumes = {"porous_ellipsoid": (a.radius, lambda: porous_ellipsoid(n, a.pores, dev)),
               "noise": (a.noise_radius, lambda: (torch.rand((n, n, n), device=dev, generator=gen) < a.density).view(torch.uint8))}
    rows = []
    for name in a.volumes:
        radius, make = volumes[name]
        vol = pipeline.pack(make())
        vol = pipeline.BitVolume(vol.bits.contiguous(), vol.shape)
        markers = pipeline.offset_volume(vol, -radius)
        values = pipeline.distance_transform(vol)
        for conn in a.connectivities:
            zones, dist = pipeline.geodesic_zones(vol, markers, connectivity=conn)
            row = {"n": n, "volume": name, "radius_mm": radius, "connectivity": conn, "set_voxels": int(pipeline.popcount_async(vol).item()),
                   "zones": int(torch.unique(zones).numel()) - 1}
            row.update(steps(vol, zones, values, dist, a.warmup, a.reps))
            cleared = torch.zeros(1, dtype=torch.int64, device=dev)
            out = torch.empty_like(vol.bits)

            def cut():
                cleared.zero_()
                _lib.check(_lib.lib().tomo_zone_cut(_p(vol.bits), _p(zones), *vol.shape, conn, _p(out), _p(cleared), _stream()), "tomo_zone_cut")
            row["cut"] = timed(cut, a.warmup, a.reps)
            row["walk_over_cut"] = {k: round(row[k]["median_ms"] / row["cut"]["median_ms"], 3) for k in ("count", "insert", "hist") if k in row}
            del out
            for key, fn in (("zone_contacts", lambda: pipeline.zone_contacts(vol, zones, connectivity=conn, values=values, dist=dist)),
                            ("zone_contacts_bare", lambda: pipeline.zone_contacts(vol, zones, connectivity=conn))):
                try:
                    row[key] = timed(fn, a.warmup, a.reps)
                except _lib.TomoError as e:
                    row[key] = {"error": str(e)[:200]}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del zones, dist
            torch.cuda.empty_cache()
        del vol, markers, values
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
