"""Drop-in for the reference's glb_exporter.py (GLBExporter, glb_exporter.py:20-91): the same class, methods and console
lines, with the work of trimesh (fix_normals, export as GLB) and of create_layer_colors done by HIP kernels on the MI355X
(csrc/glb.hip; pipeline.layer_colors / glb_pack underneath).  The file is a valid glTF 2.0 binary with the orientation of
the contract in include/tomo_hip.h; it is not byte-identical to a trimesh-written file.  trimesh is not
needed.  No CPU fallback.

Optional, beyond the reference: with `include_normals` set (an instance attribute; TOMO_GLB_NORMALS=1 in the environment
turns it on for every new exporter, so the reference's unchanged orchestrator gets it too) the file also carries NORMAL,
the area-weighted vertex normals of the normals contract in include/tomo_hip.h.  Off by default: the file is then byte for
byte what it was.
"""
import os
from typing import Optional

import numpy as np
import torch

from . import pipeline
from .voxel_processor import _device


def _host_vertices(vertices):
    v = np.asarray(vertices)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (v.shape,))
    return v


def _upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_device())


class GLBExporter:
    """Handles exporting 3D models to GLB file format (reference: glb_exporter.py:20)."""

    def __init__(self):
        self.include_normals = os.environ.get("TOMO_GLB_NORMALS", "0") not in ("", "0")

    def export_to_glb(self, vertices: np.ndarray, faces: np.ndarray,
                      filename: str = "tomography_model.glb",
                      vertex_colors: Optional[np.ndarray] = None) -> bool:
        """glb_exporter.py:26-49: True and "Model exported: ..." on success, False and "Export failed: ..." otherwise.  Only
        a missing GPU / library raises."""
        try:
            v = _host_vertices(vertices)
            f = np.asarray(faces)
            if f.ndim != 2 or f.shape[1] != 3:
                raise ValueError("faces must be (F, 3), got %s" % (f.shape,))
            if f.dtype.kind not in "iu":
                raise TypeError("faces must be integer, got %s" % f.dtype)
            cc = 0
            if vertex_colors is not None:
                c = np.asarray(vertex_colors)
                if c.dtype != np.uint8 or c.ndim != 2 or c.shape[0] != len(v) or c.shape[1] not in (3, 4):
                    raise ValueError("vertex colours must be uint8 (V, 3) or (V, 4), got %s %s" % (c.dtype, c.shape))
                cc = c.shape[1]
            normals = bool(self.include_normals)
            pipeline.glb_check_sizes(len(v), len(f), cc, normals)    # from the shapes, before anything is copied
            if v.dtype not in (np.float32, np.float64):
                v = v.astype(np.float64)
            vt, ft = _upload(v), _upload(f.astype(np.int64, copy=False))
            ct = _upload(c) if cc else None
            pipeline.export_glb(filename, vt, ft, ct, normals)
            print(f"Model exported: {filename}")
            return True
        except pipeline._lib.TomoUnavailable:
            raise
        except Exception as e:
            print(f"Export failed: {e}")
            return False

    def create_layer_colors(self, vertices: np.ndarray, slice_depths: np.ndarray,
                            first_section1_slice: int, last_section1_slice: int,
                            highlight_thickness_mm: float = 1.0) -> np.ndarray:
        """glb_exporter.py:52-91: RGBA uint8 (V, 4), grey / red / blue by the depth column, bit-exact against the reference."""
        v = np.asarray(vertices)
        if len(v) == 0:
            return np.full((0, 4), [200, 200, 200, 255], dtype=np.uint8)
        if v.dtype not in (np.float32, np.float64):
            v = v.astype(np.float64)
        z = _upload(v[:, 0])[:, None]
        return pipeline.layer_colors(z, slice_depths, first_section1_slice, last_section1_slice,
                                     highlight_thickness_mm).cpu().numpy()
