#!/usr/bin/env python3
"""Fixtures of the GLB export, from the reference itself:

    python3.9 tests/golden/make_glb_golden.py <directory of the reference's sources>

(run with the reference's own interpreter and NumPy; importing its glb_exporter works without trimesh).

  * tests/golden/layer_colors.npz: GLBExporter.create_layer_colors (glb_exporter.py:52-91) of the reference on the cases
    below -- per case k: v<k> vertices (absent where
    they are the `verts` of ellipsoid_64x128x128.npz), d<k> slice depths, i<k> [first, last], t<k> thickness, c<k> the colours it returned;
  * tests/golden/reference_api_glb.json: the signatures of the reference's GLBExporter, read from the source text with ast
    exactly as make_reference_api.py does (no source text is stored).

NumPy 1.x compares a float32 column with a float64 bound in float32, NumPy 2 in float64.  Every float32 case here has bounds
that float32 holds exactly, so its colours are the same under either rule (checked below): the fixture does not depend on
the NumPy it was made with.
"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_api import signatures  # noqa: E402


def cases():
    e = np.load(os.path.join(HERE, "ellipsoid_64x128x128.npz"))
    v, d = e["verts"], e["depths"]
    s0, s1, _ = (int(x) for x in e["sides"])
    first, last = s0, s0 + s1 - 1
    out = [
        (v, d, first, last, 1.0),                    # the orchestrator's call (tomography_3d_reconstruction.py:252-261)
        (v, d, first, last, 0.0),                    # thickness 0: only vertices exactly on the start
        (v, d, 20, 20, 1.0),                         # first == last: blue over red everywhere
        (v, d, first, len(d), 1.0),                  # last at len(slice_depths): the blue zone is skipped
        (v, d, len(d) + 3, last, 1.0),               # first past the end: the red zone is skipped
        (v, d, 10, 11, 2.0),                         # overlapping zones
    ]
    # vertices exactly on a zone bound and either side of it (float32; bounds float32 holds exactly)
    d2 = np.full(16, 0.5)
    zs = []
    for b in (2.0, 3.0, 3.5, 4.5):
        zs += [b, np.nextafter(np.float32(b), np.float32(-10)), np.nextafter(np.float32(b), np.float32(10))]
    z = np.array(zs, np.float32)
    v2 = np.stack([z, np.arange(len(z), dtype=np.float32), -z], 1).astype(np.float32)
    out.append((v2, d2, 4, 7, 1.0))
    # float64 vertices, bounds float32 cannot hold, a negative index (NumPy indexing from the end, as the reference does)
    rng = np.random.default_rng(11)
    d3 = np.full(40, 0.1)
    cum = np.cumsum(np.concatenate([[0], d3]))
    edges = np.concatenate([cum[[3, 9, 30, 39]], cum[[3, 9, 30, 39]] + 0.7])
    z3 = np.concatenate([rng.uniform(-0.2, 4.3, 3000), edges, np.nextafter(edges, -1), np.nextafter(edges, 9)])
    v3 = np.stack([z3, rng.random(len(z3)), rng.random(len(z3))], 1)
    out += [(v3, d3, 3, 9, 0.7), (v3, d3, -10, 39, 0.7), (v3, d3, 9, 3, 0.7)]
    return out


def main():
    ref = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ref)
    GLBExporter = importlib.import_module("glb_exporter").GLBExporter
    g = GLBExporter()
    arrays = {}
    cs = cases()
    for k, (v, d, first, last, t) in enumerate(cs):
        c = g.create_layer_colors(v, d, first, last, t)
        assert c.dtype == np.uint8 and c.shape == (len(v), 4)
        if v.dtype == np.float32:               # the same colours with float64 comparisons (NumPy 2's rule)
            c64 = g.create_layer_colors(v.astype(np.float64), d, first, last, t)
            assert np.array_equal(c, c64), k
        if v is not cs[0][0]:
            arrays["v%d" % k] = v
        arrays.update({"d%d" % k: d, "i%d" % k: np.array([first, last], np.int64), "t%d" % k: np.float64(t),
                       "c%d" % k: c})
        print(k, v.dtype, "grey %d red %d blue %d" % tuple(int((c[:, :3] == x).all(1).sum()) for x in
                                                         ([200, 200, 200], [255, 0, 0], [0, 0, 255])))
    arrays["n_cases"] = np.int64(len(cs))
    arrays["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(os.path.join(HERE, "layer_colors.npz"), **arrays)
    api = {"signatures": {"glb_exporter.py:GLBExporter": signatures(os.path.join(ref, "glb_exporter.py"), "GLBExporter")}}
    with open(os.path.join(HERE, "reference_api_glb.json"), "w") as fh:
        json.dump(api, fh, indent=1)
        fh.write("\n")
    print("wrote layer_colors.npz, reference_api_glb.json")


if __name__ == "__main__":
    main()
