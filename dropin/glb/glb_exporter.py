"""Put this directory on sys.path too (after dropin/, opt-in) and `from glb_exporter import GLBExporter` (the reference's
GLB writer, glb_exporter.py:20) binds the native exporter of the MI355X build.  Its files are glTF 2.0 but not trimesh's bytes."""
from tomography_3d_reconstructor_amd.glb_exporter import GLBExporter  # noqa: F401
