#!/usr/bin/env python3
"""Record the reference's public API as DATA for tests/test_boundary_conformance.py: tests/golden/reference_api.json.

    python tests/golden/make_reference_api.py <directory of the reference's sources>

Everything is read from the source TEXT with ast; nothing of the reference runs.  What is stored:
  * `signatures`: for each class the drop-in replaces, {method name: str(inspect.Signature)} of every method, in the order of
    the class body (a stub class with the same `def` lines and `pass` bodies is compiled, so modules that need cv2 work too);
  * `orchestrator`: the module-level `from X import Y` lines of tomography_3d_reconstruction.py and the components its
    constructor makes (`self.attr = Class(...)`: attribute, class, number of positional arguments).
No source text is stored.
"""
import ast
import inspect
import json
import os
import sys
import typing

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_api.json")
CLASSES = [  # (reference file, class)
    ("voxel_processor.py", "VoxelProcessor"),
    ("surface_extractor.py", "SurfaceExtractor"),
    ("volume_calculator.py", "VolumeCalculator"),
    ("obj_exporter.py", "OBJExporter"),
    ("image_loader.py", "ImageLoader"),
    ("ellipsoid_slice_generator.py", "EllipsoidSliceGenerator"),
]
ORCHESTRATOR = ("tomography_3d_reconstruction.py", "Tomography3DReconstruction")


def signatures(path, cls):
    """{method name: str(inspect.Signature)} of class `cls` in the file at `path`, from its source text."""
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    stubs = [ast.FunctionDef(name=f.name, args=f.args, body=[ast.Pass()], decorator_list=[], returns=f.returns, type_comment=None)
             for f in node.body if isinstance(f, ast.FunctionDef)]
    mod = ast.fix_missing_locations(ast.Module(body=[ast.ClassDef(name=cls, bases=[], keywords=[], body=stubs, decorator_list=[])],
                                               type_ignores=[]))
    ns = {k: getattr(typing, k) for k in ("Optional", "Tuple", "List", "Dict", "Union", "Any")}
    ns["np"] = np
    exec(compile(mod, path, "exec"), ns)
    return {name: str(inspect.signature(fn)) for name, fn in vars(ns[cls]).items() if inspect.isfunction(fn)}


def orchestrator(path, cls):
    tree = ast.parse(open(path).read())
    imports = [[n.module, a.name] for n in tree.body if isinstance(n, ast.ImportFrom) for a in n.names]
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    init = next(f for f in node.body if isinstance(f, ast.FunctionDef) and f.name == "__init__")
    components = []
    for st in ast.walk(init):
        if (isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Attribute)
                and isinstance(st.value, ast.Call) and isinstance(st.value.func, ast.Name)):
            components.append([st.targets[0].attr, st.value.func.id, len(st.value.args)])
    return {"file": os.path.basename(path), "class": cls, "imports": imports, "components": components}


def main():
    ref = sys.argv[1]
    out = {"signatures": {"%s:%s" % (f, c): signatures(os.path.join(ref, f), c) for f, c in CLASSES},
           "orchestrator": orchestrator(os.path.join(ref, ORCHESTRATOR[0]), ORCHESTRATOR[1])}
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
