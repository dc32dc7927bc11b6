"""Writes tests/golden/topology.npz: the answers of tests/topology_reference.py (the definitions, on SciPy's labelling) for the
volumes of topology_reference.fixtures().

    python tests/golden/make_topology_golden.py        (written with SciPy 1.15.3)

Per volume NAME: shape_NAME, bits_NAME (the voxels, bit-packed as BitVolume holds them) and, for connectivity C in 6, 26:
topoC_NAME (int64 (n, 3): euler, cavities, handles of component 1..n) and chiC_NAME (the Euler number of the whole volume,
counted on the whole volume).  The script asserts what the definitions promise: the components' Euler numbers add up to the
volume's and no handle count is negative.  The archive is written member by member, uncompressed and with a fixed time stamp,
so the same arrays give the same bytes: tests/test_topology_cpu.py regenerates the file and compares."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_reference as C  # noqa: E402
import topology_reference as T  # noqa: E402

PATH = os.path.join(HERE, "topology.npz")


def arrays():
    out = {}
    for name, vol in T.fixtures().items():
        out["shape_" + name] = np.array(vol.shape, dtype=np.int64)
        out["bits_" + name] = C.pack(vol)
        for conn in C.CONNECTIVITIES:
            _, n, table = T.components(vol, conn)
            chi = T.euler(vol, conn)
            assert int(table[:, 0].sum()) == chi, (name, conn, "the components' Euler numbers do not add up")
            assert n == 0 or int(table[:, 2].min()) >= 0, (name, conn, "a negative handle count")
            out["topo%d_%s" % (conn, name)] = table
            out["chi%d_%s" % (conn, name)] = np.int64(chi)
    return out


def encode(named):
    """An .npz archive of the arrays as bytes: stored, not deflated, every member stamped 1980-01-01."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for key, value in named.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue())
    return buf.getvalue()


def main():
    named = arrays()
    for name in T.fixtures():
        print("%-14s %-14s" % (name, tuple(int(s) for s in named["shape_" + name])), "  ".join(
            "%2d: %4d components, chi %5d, cavities %4d, handles %4d" % (
                conn, len(named["topo%d_%s" % (conn, name)]), named["chi%d_%s" % (conn, name)],
                named["topo%d_%s" % (conn, name)][:, 1].sum(), named["topo%d_%s" % (conn, name)][:, 2].sum())
            for conn in C.CONNECTIVITIES))
    with open(PATH, "wb") as f:
        f.write(encode(named))
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
