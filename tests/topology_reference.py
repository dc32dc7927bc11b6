"""Host reference for the topology measurements (pipeline.euler_number / component_topology / volume_topology): the
definitions, literally, in NumPy / SciPy -- for small dense arrays.

Foreground connectivity k is 6 or 26, the background has the complementary k' = 32 - k, everything outside the stack is
background (one virtual layer: every mask is padded by one voxel first).

euler():      k = 26: the union of the closed unit cubes of the set voxels, chi = V - E + F - C with a lattice cell present if
              ANY of the voxels incident to it is set (shifted ORs).  k = 6: the dual complex, chi = N0 - N1 + N2 - N3 with a
              cell present if ALL of its voxels are set (shifted ANDs).  A cell of dimension d of either complex is a set S of d
              axes along which the mask is combined with itself shifted by one.
cavities():   components of the padded complement under k', minus the outside.
components(): per component c of the labelling under k: chi and cavities of the mask `labels == c`, handles = 1 - chi +
              cavities -> (labels, n, int64 (n, 3)).  The mask is cut to the component's box first (the padding puts the
              outside back; what the cut removes was background of one piece with it).
The labelling is scipy.ndimage.label where SciPy imports and components_reference.label (the same numbering, held against SciPy
by tests/test_components_cpu.py) where it does not."""
import itertools

import numpy as np

import components_reference as C

try:
    from scipy import ndimage
except ImportError:                                              # pragma: no cover
    ndimage = None

COLUMNS = ("euler", "cavities", "handles")


def label(mask, k):
    if k not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    if ndimage is None:
        return C.label(mask, k)
    labels, n = ndimage.label(mask, ndimage.generate_binary_structure(3, 1 if k == 6 else 3))
    return labels.astype(np.int32), int(n)


def _cells(p, axes, combine):
    """Number of cells spanned along `axes`: p combined with itself shifted by one along each of them."""
    for ax in axes:
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        p = combine(p[tuple(lo)], p[tuple(hi)])
    return int(np.count_nonzero(p))


def cell_counts(mask, k):
    """k = 26 -> (V, E, F, C) of the cubical complex; k = 6 -> (N0, N1, N2, N3) of the dual complex."""
    if k not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    p = np.pad(np.asarray(mask) != 0, 1)
    combine = np.logical_or if k == 26 else np.logical_and
    by_size = [sum(_cells(p, s, combine) for s in itertools.combinations(range(3), d)) for d in range(4)]
    return tuple(by_size[::-1]) if k == 26 else tuple(by_size)   # OR over d axes is a cell of dimension 3 - d


def euler(mask, k):
    a, b, c, d = cell_counts(mask, k)
    return a - b + c - d


def cavities(mask, k):
    mask = np.asarray(mask) != 0
    return label(~np.pad(mask, 1), 32 - k)[1] - 1


def _boxes(labels, n):
    lo = np.full((n, 3), np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full((n, 3), -1, dtype=np.int64)
    idx = np.nonzero(labels)
    c = labels[idx].astype(np.int64) - 1
    for ax, a in enumerate(idx):
        np.minimum.at(lo[:, ax], c, a)
        np.maximum.at(hi[:, ax], c, a)
    return lo, hi


def components(vol, k):
    """-> (labels, n, table int64 (n, 3): euler, cavities, handles of component 1..n)."""
    vol = np.asarray(vol) != 0
    labels, n = label(vol, k)
    out = np.zeros((n, 3), dtype=np.int64)
    lo, hi = _boxes(labels, n)
    for c in range(n):
        box = tuple(slice(int(a), int(b) + 1) for a, b in zip(lo[c], hi[c]))
        mask = labels[box] == c + 1
        out[c, 0] = euler(mask, k)
        out[c, 1] = cavities(mask, k)
    out[:, 2] = 1 - out[:, 0] + out[:, 1]
    return labels, n, out


def volume(table):
    """pipeline.volume_topology's dict from the table of components()."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
    return {"components": int(len(table)), "cavities": int(table[:, 1].sum()), "handles": int(table[:, 2].sum()),
            "euler": int(table[:, 0].sum())}


# ----------------------------------------------------------------------------- the volumes of the tests
def ball(n=11, r=4.2):
    z, y, x = np.indices((n, n, n)) - n // 2
    return z * z + y * y + x * x <= r * r


def shell(n=11, r=4.2, hole=2.2):
    z, y, x = np.indices((n, n, n)) - n // 2
    d = z * z + y * y + x * x
    return (d <= r * r) & (d > hole * hole)


def torus(n=15, big=4.5, small=1.6):
    z, y, x = np.indices((5, n, n)).astype(np.float64)
    z -= 2
    y -= n // 2
    x -= n // 2
    return (np.sqrt(y * y + x * x) - big) ** 2 + z * z <= small * small


def corner_pair():
    v = np.zeros((2, 2, 2), dtype=bool)
    v[0, 0, 0] = v[1, 1, 1] = True
    return v


def diamond():
    """Four voxels of a 1 x 3 x 3 slice that meet only at corners."""
    v = np.zeros((1, 3, 3), dtype=bool)
    v[0, 0, 1] = v[0, 1, 0] = v[0, 1, 2] = v[0, 2, 1] = True
    return v


def pierced_cube():
    """A 3 x 3 x 3 cube without its centre and one corner: under 6 the centre drains through the corner."""
    v = np.ones((3, 3, 3), dtype=bool)
    v[1, 1, 1] = v[0, 0, 0] = False
    return v


def nested():
    """11^3: a shell that holds an island with a void of its own."""
    v = np.zeros((11, 11, 11), dtype=bool)
    v[1:10, 1:10, 1:10] = True
    v[2:9, 2:9, 2:9] = False
    v[4:7, 4:7, 4:7] = True
    v[5, 5, 5] = False
    return v


def open_void():
    """A box whose void reaches the face z = 0 of the stack."""
    v = np.ones((4, 5, 6), dtype=bool)
    v[0:3, 2, 2:4] = False
    return v


def word_edges(nx):
    """(4, 5, nx): a slab of full rows with voids punched where the width allows -- single voxels either side of the word
    seams, and for nx = 130 a cavity across the seam at 64 / a handle through the slab; the border rows and columns stay."""
    v = np.ones((4, 5, nx), dtype=bool)
    for x in (1, 31, 62, 63, 64, 65, 127, 128):
        if 0 < x < nx - 1:
            v[1 + x % 2, 2, x] = False                           # one-voxel cavities (under 6 and 26: they share no corner)
    if nx >= 130:
        v[:, 3, 100] = False                                     # a tunnel through the slab in z: one handle
        v[1:3, 1, 60:70] = False                                 # a cavity across the word seam
    return v


def cavity_at_64():
    """A cavity whose first run in raster order starts at x = 64: the voxel left of it is bit 63 of the word before."""
    v = np.zeros((5, 5, 70), dtype=bool)
    v[1:4, 1:4, 60:69] = True
    v[2, 2, 64:67] = False
    return v


def straddle():
    """ny = 5, nz = 20: the 64 rows of a wave lie in 13 slices.  Two bodies with a tunnel and a cavity each."""
    v = np.zeros((20, 5, 9), dtype=bool)
    v[0:9, :, 0:4] = True
    v[2:7, 2, 1] = False                                         # a cavity
    v[:9, 3, 2] = False                                          # a tunnel open at z = 0
    v[0:9, 2, 2] = True
    v[10:20, :, 3:9] = True
    v[10:20, 2, 6] = False                                       # a tunnel, both ends open
    v[12:18, 1:4, 4] = True
    v[14, 3, 7] = False                                          # a one-voxel cavity
    return v


def sponge():
    """(20, 20, 130), 400 rows = more than one workgroup: one block with a lattice of one-voxel cavities, tunnels along x that
    are open at both ends, and a plate next to it that is joined to the block by two bridges (one more handle)."""
    v = np.zeros((20, 20, 130), dtype=bool)
    v[1:19, 1:15, :] = True
    v[2:18:4, 3:14:4, 2:128:4] = False
    v[8, 4:14:6, :] = False
    v[1:19, 17:19, 5:125] = True
    v[4, 15:17, 20] = v[12, 15:17, 100] = True
    return v


def noise(density, shape=(6, 9, 70), seed=7):
    return np.random.default_rng(seed).random(shape) < density


NOISE_DENSITIES = (0.3, 0.5, 0.8)


def fixtures():
    """name -> bool volume, in a fixed order."""
    out = {"ball": ball(), "shell": shell(), "torus": torus(), "corner_pair": corner_pair(), "diamond": diamond(),
           "pierced_cube": pierced_cube(), "nested": nested(), "open_void": open_void(), "full": np.ones((3, 4, 70), dtype=bool),
           "empty": np.zeros((3, 4, 70), dtype=bool), "one_voxel": np.ones((1, 1, 1), dtype=bool)}
    for nx in (1, 63, 64, 65, 130):
        out["words_%d" % nx] = word_edges(nx)
    out["cavity_at_64"] = cavity_at_64()
    out["straddle"] = straddle()
    out["sponge"] = sponge()
    for d in NOISE_DENSITIES:
        out["noise_%03d" % round(100 * d)] = noise(d)
    return out
