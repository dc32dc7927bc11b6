"""Host reference for the connected-component tests: scipy.ndimage.label's result without SciPy (the GPU machine may not
have it), in plain NumPy, for small dense arrays.

label(): union-find over the set voxels.  Voxels get compact ids in raster order, every pair of neighbouring set voxels (3
half-neighbours under connectivity 6 = generate_binary_structure(3, 1), 13 under 26 = (3, 3)) is an edge, the larger root of
an edge is hooked under the smaller one and the trees are flattened until no edge joins two trees.  The root of a component
is then its first voxel in raster order, and the second pass numbers the roots 1..n in ascending order: SciPy's numbering
(tests/test_components_cpu.py holds it against tests/golden/components.npz and, where it imports, against SciPy itself).

fixtures(): the volumes of the tests, by name.  tests/golden/make_components_golden.py stores them bit-packed next to SciPy's
answers, so the tests on a machine without SciPy use the very same voxels."""
import itertools

import numpy as np

CONNECTIVITIES = (6, 26)


def half_neighbours(connectivity):
    """The offsets (dz, dy, dx) > (0, 0, 0) of the structuring element: each undirected neighbour pair once."""
    if connectivity == 6:
        return [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    if connectivity == 26:
        return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]
    raise ValueError("connectivity must be 6 or 26")


def _window(n, d):
    """Slices of an axis of length n for a voxel and its neighbour at offset d."""
    return (slice(0, n - d), slice(d, n)) if d >= 0 else (slice(-d, n), slice(0, n + d))


def label(vol, connectivity=6):
    """-> (labels int32 like vol, n) as scipy.ndimage.label(vol, generate_binary_structure(3, 1 or 3))."""
    a = np.asarray(vol) != 0
    if a.ndim != 3:
        raise ValueError("volume must be 3-D")
    offsets = half_neighbours(connectivity)
    flat = np.flatnonzero(a)
    ids = np.full(a.shape, -1, dtype=np.int64)
    ids.reshape(-1)[flat] = np.arange(len(flat))
    us, vs = [], []
    for dz, dy, dx in offsets:
        (z0, z1), (y0, y1), (x0, x1) = _window(a.shape[0], dz), _window(a.shape[1], dy), _window(a.shape[2], dx)
        p, q = ids[z0, y0, x0], ids[z1, y1, x1]
        both = (p >= 0) & (q >= 0)
        us.append(p[both])
        vs.append(q[both])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(len(flat))
    while len(u):
        pu, pv = parent[u], parent[v]                            # roots: the trees are flat here
        open_ = pu != pv
        if not open_.any():
            break
        u, v, pu, pv = u[open_], v[open_], pu[open_], pv[open_]  # an edge inside one tree stays inside it
        np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    is_root = parent == np.arange(len(flat))
    number = np.cumsum(is_root)                                  # roots ascend in raster order of the first voxel
    out = np.zeros(a.shape, dtype=np.int32)
    out.reshape(-1)[flat] = number[parent]
    return out, int(is_root.sum())


def sizes(labels, n):
    """Voxels of component 1..n -> int64 (n,)."""
    return np.bincount(np.asarray(labels).reshape(-1), minlength=n + 1)[1:n + 1].astype(np.int64)


def keep_from(vol, labels, n, min_voxels=0, largest=False):
    """The keep rule given a labelling: components of at least min_voxels voxels; largest: only the largest of those, the
    lowest label among equals."""
    sz = sizes(labels, n)
    ok = sz >= min_voxels
    if largest:
        only = np.zeros(n, dtype=bool)
        if ok.any():
            only[int(np.argmax(np.where(ok, sz, -1)))] = True    # argmax returns the first maximum
        ok = only
    return np.concatenate([[False], ok])[labels] & (np.asarray(vol) != 0)


def keep(vol, min_voxels=0, largest=False, connectivity=6):
    labels, n = label(vol, connectivity)
    return keep_from(vol, labels, n, min_voxels, largest)


def pack(vol):
    """A bool volume as BitVolume.bits holds it: int64 (nz, ny, words), bit b of word w = voxel 64 w + b, tail bits zero."""
    a = np.asarray(vol) != 0
    nz, ny, nx = a.shape
    wx = (nx + 63) // 64
    by = np.zeros((nz, ny, wx * 8), dtype=np.uint8)
    pb = np.packbits(a, axis=2, bitorder="little")
    by[:, :, :pb.shape[2]] = pb
    return by.view("<u8").astype(np.uint64).view(np.int64).reshape(nz, ny, wx)


def unpack(bits, shape):
    by = np.ascontiguousarray(bits).view(np.uint8).reshape(shape[0], shape[1], -1)
    return np.unpackbits(by, axis=2, bitorder="little")[:, :, :shape[2]].astype(bool)


# ----------------------------------------------------------------------------- the volumes of the tests
WORD_NX = (1, 20, 63, 64, 65, 70, 130)
NOISE = (("noise_010", (13, 37, 130), 0.1), ("noise_031", (13, 37, 130), 0.31), ("noise_090", (13, 37, 130), 0.9),
         ("noise_big", (40, 96, 200), 0.25))
# what the issue lists for these volumes (scipy.ndimage.label, SciPy 1.15.3); test_components_cpu.py holds the golden file to it
KNOWN_COUNTS = {("checkerboard", 6): 65536, ("checkerboard", 26): 1, ("serpentine", 6): 1, ("edge", 6): 2, ("edge", 26): 1,
                ("corner", 6): 2, ("corner", 26): 1, ("empty", 6): 0, ("empty", 26): 0, ("full", 6): 1, ("full", 26): 1,
                ("noise_010", 6): 4563, ("noise_031", 6): 3832, ("noise_090", 6): 2, ("noise_big", 6): 59298}
LABELLED = 70000             # voxels up to which the golden file stores SciPy's label array as well


def _word_geometry(nx):
    """Rows whose runs sit on the word boundaries a width allows, in a bed of noise."""
    rng = np.random.default_rng(100 + nx)
    v = rng.random((3, 6, nx)) < 0.55
    v[0, 0, :] = True                                            # a full row
    v[0, 1, :] = False
    v[2, 5, :] = False
    if nx >= 64:
        v[1, 1, :] = False
        v[1, 1, 40:64] = True                                    # a run that ends at bit 63
    if nx > 64:
        v[1, 2, :] = False
        v[1, 2, 64:nx] = True                                    # a run that starts at bit 0 of the second word ...
        v[1, 3, 63] = False                                      # ... and one below a clear bit 63
        v[1, 3, 64:min(nx, 67)] = True
    if nx >= 130:
        v[2, 2, :] = False
        v[2, 2, 60:130] = True                                   # a run across three words
        v[2, 3, :] = False
        v[2, 3, 0:64] = True                                     # exactly one word
    return v


def _serpentine():
    """(6, 9, 70): full rows at even y, joined alternately at either end; the ends swap from slice to slice.  2 124 voxels."""
    v = np.zeros((6, 9, 70), dtype=bool)
    v[:, 0::2, :] = True
    for z in range(6):
        for k, y in enumerate(range(1, 9, 2)):
            v[z, y, 69 if (k + z) % 2 == 0 else 0] = True
    return v


def _snake3d():
    """One voxel-thin path through (7, 9, 70): a serpentine in every even slice, ONE corner voxel in every odd slice: the
    equivalence chain runs through every run of the volume, forwards and backwards in raster order."""
    v = np.zeros((7, 9, 70), dtype=bool)
    for z in range(0, 7, 2):
        v[z, 0::2, :] = True
        for k, y in enumerate(range(1, 9, 2)):
            v[z, y, 69 if k % 2 == 0 else 0] = True
    for k, z in enumerate(range(1, 7, 2)):
        v[z, 8 if k % 2 == 0 else 0, 69 if k % 2 == 0 else 0] = True
    return v


def _comb():
    """Prongs (every other column, all slices, all rows) that meet only in the last row of the last slice."""
    v = np.zeros((4, 7, 70), dtype=bool)
    v[:, :, 0::2] = True
    v[3, 6, :] = True
    return v


def _cubes(kind):
    """Two 2x2x2 cubes on either side of a word boundary that share only an edge / only a corner."""
    v = np.zeros((5, 6, 70), dtype=bool)
    v[0:2, 0:2, 62:64] = True
    if kind == "edge":
        v[0:2, 2:4, 64:66] = True
    else:
        v[2:4, 2:4, 64:66] = True
    return v


def _tie():
    """Two equal cubes (27 voxels each) and a speck: the largest component is a tie, the first cube wins it."""
    v = np.zeros((8, 10, 70), dtype=bool)
    v[1:4, 1:4, 3:6] = True
    v[4:7, 5:8, 60:63] = True
    v[0, 9, 69] = True
    return v


def fixtures():
    """name -> bool volume, in a fixed order."""
    out = {}
    for nx in WORD_NX:
        out["words_%d" % nx] = _word_geometry(nx)
    rng = np.random.default_rng(11)
    out["one_slice"] = rng.random((1, 9, 70)) < 0.5
    out["one_row"] = rng.random((5, 1, 70)) < 0.5
    out["one_voxel"] = np.ones((1, 1, 1), dtype=bool)
    out["one_voxel_clear"] = np.zeros((1, 1, 1), dtype=bool)
    out["empty"] = np.zeros((3, 4, 70), dtype=bool)
    out["full"] = np.ones((3, 4, 70), dtype=bool)
    out["edge"] = _cubes("edge")
    out["corner"] = _cubes("corner")
    z, y, x = np.indices((32, 64, 64))
    out["checkerboard"] = (z + y + x) % 2 == 0
    out["serpentine"] = _serpentine()
    out["snake3d"] = _snake3d()
    out["comb"] = _comb()
    out["tie"] = _tie()
    rng = np.random.default_rng(3)                               # ONE generator, drawn in this order
    for name, shape, density in NOISE:
        out[name] = rng.random(shape) < density
    return out
