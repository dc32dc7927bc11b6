#!/usr/bin/env python3
"""GLB export at n^3 (default 1024): GLBExporter.export_to_glb host to host, split into upload, device work (edge table,
orientation check, pack), download and write; the device work alone on the fast path and on the same mesh with 30 % of
its faces reversed (the union-find path); the same with the optional NORMAL attribute (vertex normals, the normals contract
of include/tomo_hip.h); create_layer_colors on the device next to the reference's NumPy passes.

    python tools/glbtime.py [--n 1024] [--reps 5] [--out glbtime.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomography_3d_reconstructor_amd import pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.glb_exporter import GLBExporter  # noqa: E402


def numpy_layer_colors(vertices, slice_depths, first, last, t=1.0):
    """glb_exporter.py:52-91 as written (the NumPy passes being replaced)."""
    colors = np.full((len(vertices), 4), [200, 200, 200, 255], dtype=np.uint8)
    cum = np.cumsum(np.concatenate([[0], slice_depths]))
    if first < len(cum) - 1:
        s = cum[first]
        colors[(vertices[:, 0] >= s) & (vertices[:, 0] <= s + t)] = [255, 0, 0, 255]
    if last < len(cum) - 1:
        s = cum[last]
        colors[(vertices[:, 0] >= s) & (vertices[:, 0] <= s + t)] = [0, 0, 255, 255]
    return colors


def ms(fn, reps):
    best = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(best), 3), "median_ms": round(float(np.median(best)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.n
    mask = pipeline.ellipsoid_mask(n, n, n, dev)
    sm = pipeline.smooth(pipeline.close_ends(pipeline.pack(mask)), 3, True)
    del mask
    depths = np.full(n, 1.0)
    v, f = pipeline.extract_surface(sm, depths, 1.0, 1.0)
    del sm
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    nv, nf = len(vn), len(fn)
    first, last = n // 8, n - n // 8 - 1
    g = GLBExporter()
    colors = g.create_layer_colors(vn, depths, first, last)
    assert np.array_equal(colors, numpy_layer_colors(vn, depths, first, last))
    res = {"n": n, "n_vertices": nv, "n_faces": nf, "bin_bytes": pipeline.glb_layout_bytes(nv, nf, 4)}
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "m.glb")

    # host to host through the class, and the same steps one by one
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        g.export_to_glb(vn, fn, path, colors)                                   # warm (pinned cache, code objects)
        res["export_to_glb"] = ms(lambda: g.export_to_glb(vn, fn, path, colors), a.reps)
    split = {"upload": [], "device": [], "download": [], "write": []}
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vt, ft, ct = (torch.from_numpy(x).to(dev) for x in (vn, fn, colors))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        p = pipeline.glb_pack(vt, ft, ct)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host = pipeline.glb_download(p)
        t3 = time.perf_counter()
        pipeline.glb_write(path, p, host)
        t4 = time.perf_counter()
        for k, d in zip(split, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            split[k].append(d * 1e3)
        del p, host, vt, ft, ct
    res["split_ms_median"] = {k: round(float(np.median(x)), 3) for k, x in split.items()}
    res["file_bytes"] = os.path.getsize(path)
    g.include_normals = True                                                    # the same call with NORMAL in the file
    with contextlib.redirect_stdout(io.StringIO()):
        g.export_to_glb(vn, fn, path, colors)
        res["export_to_glb_normals"] = ms(lambda: g.export_to_glb(vn, fn, path, colors), a.reps)
    res["file_bytes_normals"] = os.path.getsize(path)
    g.include_normals = False

    # device work alone: fast path, and the same mesh with 30 % of the faces reversed (union-find)
    res["device_fast"] = ms(lambda: pipeline.glb_pack(v, f, None), a.reps)
    res["device_fast_normals"] = ms(lambda: pipeline.glb_pack(v, f, None, True), a.reps)
    oriented = f.flip(1).contiguous()
    res["vertex_normals_alone"] = ms(lambda: pipeline.vertex_normals(v, oriented, oriented=True), a.reps)
    del oriented
    fs = fn.copy()
    sel = np.random.default_rng(30).random(nf) < 0.30
    fs[sel] = fs[sel][:, ::-1]
    fst = torch.from_numpy(fs).to(dev)
    res["device_general"] = ms(lambda: pipeline.glb_pack(v, fst, None), a.reps)
    out, st = pipeline.orient_faces(v, fst)
    assert torch.equal(out, f.flip(1)), "scrambled mesh did not come back as fliplr"
    res["general_stats"] = {k: x for k, x in st.items()}
    res["fast_stats"] = pipeline.orient_faces(v, f)[1]

    # layer colours: device kernel (on resident vertices) vs the NumPy passes of the reference
    res["layer_colors_device"] = ms(lambda: pipeline.layer_colors(v, depths, first, last), a.reps)
    res["layer_colors_class_host_to_host"] = ms(lambda: g.create_layer_colors(vn, depths, first, last), a.reps)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        numpy_layer_colors(vn, depths, first, last)
        t.append((time.perf_counter() - t0) * 1e3)
    res["layer_colors_numpy"] = {"min_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3)}
    os.remove(path)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
