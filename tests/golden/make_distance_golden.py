"""Writes tests/golden/distance.npz: scipy.ndimage.distance_transform_edt's answers for the volumes of
tests/edt_reference.fixtures().

    python tests/golden/make_distance_golden.py        (needs SciPy; written with SciPy 1.15.3)

Per volume NAME: shape_NAME, bits_NAME (the voxels, bit-packed as BitVolume holds them) and, for the spacings S = unit and
uniform (edt_reference.UNIFORM), SciPy's float32 answer distance_transform_edt(np.pad(v, 1), sampling)[1:-1, 1:-1, 1:-1]:
edt_S_NAME for volumes of up to STORED voxels, sha_S_NAME (SHA-256 of the float32 bytes, as uint8[32]) and max_S_NAME above.
The script asserts that the helper's float32 array equals SciPy's for every case and, with unit spacing, that the helper's d2
is integral; a case that differs is printed before the assertion stops the run, so nothing unequal is ever written."""
import hashlib
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt_reference as E  # noqa: E402

STORED = 100000              # voxels up to which the answer itself is stored


def main():
    out = {}
    for name, vol in E.fixtures().items():
        out["shape_" + name] = np.array(vol.shape, dtype=np.int64)
        out["bits_" + name] = E.pack(vol)
        for kind in ("unit", "uniform"):
            depths, mm_y, mm_x = E.spacing(kind, vol.shape[0])
            sampling = (1.0 if depths is None else float(depths[0]), mm_y, mm_x)
            ref = ndimage.distance_transform_edt(np.pad(vol, 1), sampling=sampling)[1:-1, 1:-1, 1:-1].astype(np.float32)
            mine = E.edt(vol, *E.positions(vol.shape, depths, mm_y, mm_x), True)
            same = np.array_equal(ref, mine)
            if kind == "unit":
                d2 = E.edt_squared(vol, *E.positions(vol.shape), True)
                assert np.array_equal(d2, np.rint(d2)) and d2.max() < 4e6, name
            if vol.size <= STORED or not same:
                out["edt_%s_%s" % (kind, name)] = ref
            else:
                out["sha_%s_%s" % (kind, name)] = np.frombuffer(hashlib.sha256(ref.tobytes()).digest(), dtype=np.uint8)
                out["max_%s_%s" % (kind, name)] = np.float32(ref.max())
            print("%-10s %-16s %-8s max %.6f  helper %s" % (name, vol.shape, kind, ref.max(),
                                                             "identical" if same else "DIFFERS (stored)"))
            assert same, (name, kind, int((ref != mine).sum()))
    path = os.path.join(HERE, "distance.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
