"""Test helper for the NORMAL attribute of the GLB export (no GPU): the normals contract of include/tomo_hip.h restated with
NumPy, a reader that wraps glb_reference.read_glb and additionally returns and checks NORMAL, and hand-made meshes."""
import struct

import numpy as np

import glb_reference as R


def face_vectors(pos_f32, faces):
    """Rule 1: g = (p1 - p0) x (p2 - p0) in float64 from the float32 positions.  Every product and difference is a NumPy
    operation of its own, so nothing is fused."""
    pos_f32 = np.asarray(pos_f32)
    assert pos_f32.dtype == np.float32, "the contract starts from POSITION as the file stores it"
    p = pos_f32.astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = p[faces[:, 1]] - p[faces[:, 0]]
        w = p[faces[:, 2]] - p[faces[:, 0]]
        return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1],
                         u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                         u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def vertex_sums(pos_f32, faces):
    """Rule 2: float64 sums per vertex.  np.bincount adds its weights one after the other in input order, and the corners
    are listed face after face, so every vertex receives its faces in ascending face index, starting from +0.0."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    g = face_vectors(pos_f32, faces)
    corners = faces.reshape(-1)
    with np.errstate(all="ignore"):
        return np.stack([np.bincount(corners, weights=np.repeat(g[:, k], 3), minlength=len(pos_f32)) for k in range(3)], 1)


def vertex_normals(pos_f32, oriented_faces):
    """The contract: (float32 (V, 3), number of vertices that got the default (0, 0, 1))."""
    s = vertex_sums(pos_f32, oriented_faces)
    with np.errstate(all="ignore"):
        q = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]
        ok = np.isfinite(q) & (q > 0)
        n = np.zeros((len(s), 3), np.float32)
        n[:, 2] = 1.0
        n[ok] = (s[ok] / np.sqrt(q[ok])[:, None]).astype(np.float32)
    return n, int((~ok).sum())


def read_glb(path):
    """glb_reference.read_glb, and NORMAL on top: VEC3 float32, one row per vertex, a 4-byte aligned view inside the buffer
    with target 34962, every row finite with | |n|^2 - 1 | <= 1e-6 (10x the float32 rounding bound of a unit vector).
    Returns (gltf json, positions, indices, colours or None, normals f32 (V, 3))."""
    gl, pos, idx, col = R.read_glb(path)
    data = open(path, "rb").read()
    jl = struct.unpack_from("<I", data, 12)[0]
    binc = data[20 + jl + 8:]
    attrs = gl["meshes"][0]["primitives"][0]["attributes"]
    assert "NORMAL" in attrs, sorted(attrs)
    a = gl["accessors"][attrs["NORMAL"]]
    bv = gl["bufferViews"][a["bufferView"]]
    assert a["type"] == "VEC3" and a["componentType"] == 5126 and a["count"] == len(pos) and not a.get("normalized", False)
    stride = bv.get("byteStride", 12)
    aoff = a.get("byteOffset", 0)
    assert bv["buffer"] == 0 and bv.get("target") == 34962 and bv["byteOffset"] % 4 == 0 and aoff % 4 == 0
    assert stride % 4 == 0 and stride >= 12
    need = aoff + stride * (a["count"] - 1) + 12 if a["count"] else 0
    assert need <= bv["byteLength"] and bv["byteOffset"] + bv["byteLength"] <= gl["buffers"][0]["byteLength"] <= len(binc)
    raw = np.frombuffer(binc, np.uint8, bv["byteLength"], bv["byteOffset"])
    rows = np.lib.stride_tricks.as_strided(raw[aoff:], (a["count"], 12), (stride, 1))
    nrm = np.ascontiguousarray(rows).view(np.float32).reshape(a["count"], 3)
    assert np.isfinite(nrm).all()
    q = (nrm.astype(np.float64) ** 2).sum(1)
    assert (np.abs(q - 1.0) <= 1e-6).all(), float(np.abs(q - 1.0).max())
    return gl, pos, idx, col, nrm


# ---- hand-made meshes -------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=2):
    """A unit icosphere, outward winding, float32 positions."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int64)


def fan(n=4096, seed=11):
    """A cone of n faces around vertex 0 (the apex), the faces listed in a shuffled order: one vertex with a list of n."""
    a = np.arange(n) * 2 * np.pi / n
    r = 1.0 + 0.25 * np.sin(5 * a)                                   # not a circle: the face vectors differ in size
    v = np.concatenate([[[0.0, 0.0, 1.0]], np.stack([r * np.cos(a), r * np.sin(a), 0.1 * np.cos(3 * a)], 1)]).astype(np.float32)
    i = np.arange(n)
    f = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1)
    return v, f[np.random.default_rng(seed).permutation(n)]


def with_unreferenced():
    """The tetrahedron with vertices no face names in front of, between and behind its own."""
    v = np.array([[9, 9, 9], [0, 0, 0], [1, 0, 0], [8, 8, 8], [0, 1, 0], [0, 0, 1], [7, 7, 7], [6, 6, 6]], np.float32)
    remap = np.array([1, 2, 4, 5])
    return v, remap[R.TET_F]


def cancelling():
    """Two coincident faces of opposite winding (the sums of their three vertices cancel exactly) and an isolated vertex."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    return v, np.array([[0, 1, 2], [2, 1, 0]], np.int64)
