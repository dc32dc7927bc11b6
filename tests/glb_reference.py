"""Test helper for the GLB export (no GPU): the orientation contract of include/tomo_hip.h restated with NumPy and
scipy.sparse.csgraph, and a strict GLB reader."""
import json
import struct

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def edge_table(faces, nv):
    """Undirected edges of the non-degenerate faces: (stats, manifold pairs (f, g, r)) with r = 1 where f and g run their
    shared edge the same way (they must end up with opposite flips)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = len(faces)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    fid = np.repeat(np.arange(nf)[ok], 3)
    a = faces[ok].reshape(-1)
    b = faces[ok][:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    dirn = (a > b).astype(np.int64)
    key = lo * nv + hi
    order = np.argsort(key, kind="stable")               # within a key: face order (the kernels keep the first two, any order)
    key, fid, dirn = key[order], fid[order], dirn[order]
    uk, start, cnt = np.unique(key, return_index=True, return_counts=True)
    m = cnt == 2
    f, g = fid[start[m]], fid[start[m] + 1]
    r = (dirn[start[m]] == dirn[start[m] + 1]).astype(np.int64)
    stats = {"boundary_edges": int((cnt == 1).sum()), "manifold_edges": int(m.sum()), "non_manifold_edges": int((cnt >= 3).sum()),
             "inconsistent_pairs": int(r.sum()), "degenerate_faces": int((~ok).sum())}
    return stats, f, g, r


def volume_scale(verts, faces):
    """sum of |dot(v0, cross(v1, v2))| / 6: the scale the float32 rounding of the volume terms is relative to (an open mesh
    cancels most of its terms, and a reversed face's float32 term is not the exact negative of the given one's)."""
    v = np.asarray(verts, dtype=np.float64)
    return float(np.abs(np.einsum("ij,ij->i", v[faces[:, 0]], np.cross(v[faces[:, 1]], v[faces[:, 2]]))).sum() / 6.0)


def signed_volume(verts, faces):
    """sum of dot(v0, cross(v1, v2)) / 6 with float32 terms, as calculate_mesh_volume (surface_extractor.py:128-135) and the
    kernels form them, summed in float64."""
    v = np.asarray(verts, dtype=np.float32)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    cr = np.cross(b, c)
    d = a[:, 0] * cr[:, 0] + a[:, 1] * cr[:, 1] + a[:, 2] * cr[:, 2]
    return float((d.astype(np.float64) / 6.0).sum())


def orient(verts, faces):
    """The contract: (oriented faces, stats).  Rules 1-2 on a doubled graph -- node (f, p) is face f with parity p; a pair
    (f, g, r) joins (f, p) with (g, p ^ r) -- so face f's parity to its component's lowest face R is which of (R, 0) / (R, 1)
    it shares a component with, and a component conflicts exactly when (R, 0) and (R, 1) are joined.  Rule 3 on the signed
    volume of the result."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = len(faces)
    stats, f, g, r = edge_table(faces, len(verts))
    nc, lab = connected_components(coo_matrix((np.ones(len(f)), (f, g)), shape=(nf, nf)), directed=False)
    root = np.full(nc, nf, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(nf))
    R = root[lab]                                        # lowest-index face of each face's component
    rows = np.concatenate([2 * f, 2 * f + 1])
    cols = np.concatenate([2 * g + r, 2 * g + (1 - r)])
    _, lab2 = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(2 * nf, 2 * nf)), directed=False)
    parity = (lab2[2 * np.arange(nf)] != lab2[2 * R]).astype(np.int64)
    conflict_root = lab2[2 * root] == lab2[2 * root + 1]
    conflict = conflict_root[lab]
    flip = (parity == 1) & ~conflict
    out = faces.copy()
    out[flip] = out[flip][:, ::-1]
    vol = signed_volume(verts, out)
    inverted = vol < 0
    if inverted:
        out = out[:, ::-1].copy()
    stats.update({"components": int(nc), "conflicts": int(conflict_root.sum()), "inverted": bool(inverted),
                  "signed_volume": -vol if inverted else vol, "flip": flip})
    return out, stats


def read_glb(path):
    """Strict GLB 2.0 reader: header magic / version / length, chunk types, lengths and padding, accessor and bufferView
    bounds and alignment, POSITION min / max equal to the data.  Returns (gltf json, positions f32 (V,3), indices (F,3),
    colours uint8 (V, 3|4) or None)."""
    data = open(path, "rb").read()
    assert len(data) >= 12 + 8, "too short"
    magic, version, length = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and length == len(data), (magic, version, length, len(data))
    jl, jt = struct.unpack_from("<II", data, 12)
    assert jt == 0x4E4F534A and jl % 4 == 0 and 20 + jl <= len(data)
    jbytes = data[20:20 + jl]
    assert jbytes == jbytes.rstrip(b" ") + b" " * (len(jbytes) - len(jbytes.rstrip(b" ")))
    gl = json.loads(jbytes.decode("utf-8"))
    off = 20 + jl
    bl, bt = struct.unpack_from("<II", data, off)
    assert bt == 0x004E4942 and bl % 4 == 0 and off + 8 + bl == len(data)
    binc = data[off + 8: off + 8 + bl]
    assert gl["asset"]["version"] == "2.0"
    assert len(gl["buffers"]) == 1 and "uri" not in gl["buffers"][0]
    blen = gl["buffers"][0]["byteLength"]
    assert blen <= bl and bl - blen < 4 and binc[blen:] == b"\0" * (bl - blen)
    assert gl["scenes"][gl["scene"]]["nodes"] == [0] and gl["nodes"] == [{"mesh": 0}] and len(gl["meshes"]) == 1
    prims = gl["meshes"][0]["primitives"]
    assert len(prims) == 1 and prims[0]["mode"] == 4
    sizes = {5126: (4, np.float32), 5125: (4, np.uint32), 5121: (1, np.uint8)}
    ncomp = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}

    def accessor(i):
        a = gl["accessors"][i]
        bv = gl["bufferViews"][a["bufferView"]]
        csize, dt = sizes[a["componentType"]]
        k = ncomp[a["type"]]
        elem = csize * k
        stride = bv.get("byteStride", elem)
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and stride % 4 == 0 and stride >= elem
        aoff = a.get("byteOffset", 0)
        assert aoff % csize == 0
        need = aoff + stride * (a["count"] - 1) + elem if a["count"] else 0
        assert need <= bv["byteLength"] and bv["byteOffset"] + bv["byteLength"] <= blen
        raw = np.frombuffer(binc, np.uint8, bv["byteLength"], bv["byteOffset"])
        rows = np.lib.stride_tricks.as_strided(raw[aoff:], (a["count"], elem), (stride, 1)) if a["count"] else raw[:0].reshape(0, elem)
        return a, bv, np.ascontiguousarray(rows).view(dt).reshape(a["count"], k)

    attrs = prims[0]["attributes"]
    pa, pbv, pos = accessor(attrs["POSITION"])
    assert pa["type"] == "VEC3" and pa["componentType"] == 5126 and pbv.get("target") == 34962
    assert np.array_equal(np.float32(pa["min"]), pos.min(0)) and np.array_equal(np.float32(pa["max"]), pos.max(0))
    ia, ibv, idx = accessor(prims[0]["indices"])
    assert ia["type"] == "SCALAR" and ia["componentType"] == 5125 and ia["count"] % 3 == 0 and ibv.get("target") == 34963
    idx = idx.reshape(-1, 3).astype(np.int64)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < len(pos))
    col = None
    if "COLOR_0" in attrs:
        ca, cbv, col = accessor(attrs["COLOR_0"])
        assert ca["componentType"] == 5121 and ca["normalized"] is True and ca["count"] == len(pos) and cbv.get("target") == 34962
    return gl, pos, idx, col


# ---- hand-made meshes -------------------------------------------------------------------------------------------------------
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)          # outward: signed volume +1/6


def tetra_one_reversed():
    f = TET_F.copy()
    f[2] = f[2, ::-1]
    return TET_V.copy(), f


def two_bodies():
    """An outward tetrahedron with a face reversed, and an inward one twice its size (the larger body decides rule 3)."""
    v = np.concatenate([TET_V, TET_V * 2 + 5]).astype(np.float32)
    fa = TET_F.copy()
    fa[3] = fa[3, ::-1]
    return v, np.concatenate([fa, TET_F[:, ::-1] + 4])


def moebius(n=12):
    """A triangulated Moebius strip (non-orientable: a conflicting component), some faces reversed."""
    t = np.arange(n) * 2 * np.pi / n
    v = []
    for ti in t:
        for s in (-0.3, 0.3):
            v.append([(1 + s * np.cos(ti / 2)) * np.cos(ti), (1 + s * np.cos(ti / 2)) * np.sin(ti), s * np.sin(ti / 2)])
    f = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)          # the half twist
        f += [[a, c, b], [b, c, d]]
    f = np.array(f, np.int64)
    f[[3, 8, 15]] = f[[3, 8, 15]][:, ::-1]
    return np.array(v, np.float32), f


def fin():
    """Three faces on one edge (non-manifold), plus a free face."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [3, 3, 3], [4, 3, 3], [3, 4, 3]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 7]], np.int64)


def with_degenerate():
    v, f = tetra_one_reversed()
    return v, np.concatenate([f[:2], [[0, 0, 1], [2, 3, 3]], f[2:], [[1, 1, 1]]])


HAND_MADE = {"tetra_one_reversed": tetra_one_reversed, "two_bodies": two_bodies, "moebius": moebius, "fin": fin,
             "degenerate": with_degenerate}
