"""Writes tests/golden/components.npz: scipy.ndimage.label's answers for the volumes of tests/components_reference.fixtures().

    python tests/golden/make_components_golden.py        (needs SciPy; written with SciPy 1.15.3)

Per volume NAME: shape_NAME, bits_NAME (the voxels, bit-packed as BitVolume holds them), and for connectivity C in 6, 26:
nC_NAME (components), sizesC_NAME (np.bincount(labels.ravel())[1:], int64) and -- up to components_reference.LABELLED voxels --
labelsC_NAME (int32).  The script also checks what the numbering rests on: the first occurrences of labels 1..n ascend."""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_reference as C  # noqa: E402


def main():
    out = {}
    for name, vol in C.fixtures().items():
        out["shape_" + name] = np.array(vol.shape, dtype=np.int64)
        out["bits_" + name] = C.pack(vol)
        for conn in C.CONNECTIVITIES:
            labels, n = ndimage.label(vol, ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
            labels = labels.astype(np.int32)
            flat = labels.reshape(-1)
            first = np.full(n + 1, flat.size, dtype=np.int64)
            np.minimum.at(first, flat, np.arange(flat.size))
            assert np.all(np.diff(first[1:]) > 0), (name, conn, "first occurrences do not ascend")
            known = C.KNOWN_COUNTS.get((name, conn))
            assert known is None or known == n, (name, conn, n, known)
            out["n%d_%s" % (conn, name)] = np.int64(n)
            out["sizes%d_%s" % (conn, name)] = np.bincount(flat, minlength=n + 1)[1:].astype(np.int64)
            if vol.size <= C.LABELLED:
                out["labels%d_%s" % (conn, name)] = labels
            print("%-16s %-14s connectivity %2d: %6d components" % (name, vol.shape, conn, n))
    path = os.path.join(HERE, "components.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
