"""NumPy reference of the homotopic thinning (include/tomo_hip.h, "Homotopic thinning of the bit volume"): sub-passes over the
whole volume, every voxel tested in every sub-pass, the simple test by flood on the 26-neighbour picture, memoised per picture.

The picture of a voxel is a 27-bit integer, bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1); bit 13 is the voxel itself.  The floods
here walk explicit adjacency lists of the 27 cells, cell by cell -- another formulation than the shifts of the kernel."""
import numpy as np

CELLS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
CENTRE = 13
DIRECTIONS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # -z +z -y +y -x +x


def _adjacency(steps):
    """Per cell the bit mask of the cells of the cube (centre excluded) at most `steps` unit steps away, one per axis at most."""
    adj = []
    for a in CELLS:
        m = 0
        for i, b in enumerate(CELLS):
            d = [abs(p - q) for p, q in zip(a, b)]
            if i != CENTRE and max(d) == 1 and sum(d) <= steps:
                m |= 1 << i
        adj.append(m)
    return adj


ADJ26 = _adjacency(3)
ADJ6 = _adjacency(1)
N6 = sum(1 << i for i, c in enumerate(CELLS) if sum(map(abs, c)) == 1)
N18 = sum(1 << i for i, c in enumerate(CELLS) if sum(map(abs, c)) in (1, 2))
N26 = (1 << 27) - 1 - (1 << CENTRE)


def _flood(seed, inside, adj):
    reached, front = seed, seed
    while front:
        grown = 0
        while front:
            low = front & -front
            grown |= adj[low.bit_length() - 1]
            front ^= low
        front = grown & inside & ~reached
        reached |= front
    return reached


def t26(m):
    """The number of 26-connected components of the cells m (a subset of the 26 neighbours)."""
    n = 0
    while m:
        m &= ~_flood(m & -m, m, ADJ26)
        n += 1
    return n


def t6(m):
    """The number of 6-connected components of m inside N18 that contain a face neighbour of the centre."""
    m &= N18
    faces, n = m & N6, 0
    while faces:
        faces &= ~_flood(faces & -faces, m, ADJ6)
        n += 1
    return n


_SIMPLE = {26: {}, 6: {}}


def is_simple(picture, connectivity=26):
    """Is the centre of the 27-bit picture a simple point?  (The centre bit itself is ignored.)"""
    memo = _SIMPLE[connectivity]
    x = int(picture) & N26
    r = memo.get(x)
    if r is None:
        c = ~x & N26
        r = memo[x] = (t26(x) == 1 and t6(c) == 1) if connectivity == 26 else (t6(x) == 1 and t26(c) == 1)
    return r


def pictures(padded, idx):
    """The pictures of the voxels idx = (z, y, x) arrays of a volume padded by one zero voxel on every side."""
    z, y, x = (i + 1 for i in idx)
    pic = np.zeros(len(z), dtype=np.int64)
    for i, (dz, dy, dx) in enumerate(CELLS):
        pic |= padded[z + dz, y + dy, x + dx].astype(np.int64) << i
    return pic


def neighbour_counts(vol):
    """Per voxel the number of set 26-neighbours."""
    vol = np.asarray(vol, dtype=bool)
    p = np.pad(vol, 1).astype(np.int32)
    nz, ny, nx = vol.shape
    n = np.zeros(vol.shape, dtype=np.int32)
    for dz, dy, dx in CELLS:
        if (dz, dy, dx) != (0, 0, 0):
            n += p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    return n


def skeleton(vol, curve=True, connectivity=26, anchors=None):
    """-> (the thinned bool volume, the iterations run, the last one -- which cleared nothing -- included)."""
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    if curve and connectivity == 6:
        raise ValueError("curve thinning is defined under connectivity 26 only")
    vol = np.asarray(vol, dtype=bool)
    keep = np.zeros(vol.shape, dtype=bool) if anchors is None else np.asarray(anchors, dtype=bool)
    padded = np.pad(vol, 1)
    inner = padded[1:-1, 1:-1, 1:-1]
    nz, ny, nx = vol.shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    field = 4 * (zz & 1) + 2 * (yy & 1) + (xx & 1)
    iterations = 0
    while True:
        iterations += 1
        cleared = 0
        for dz, dy, dx in DIRECTIONS:
            for s in range(8):
                towards = padded[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
                idx = np.nonzero(inner & ~keep & (field == s) & ~towards)
                if not len(idx[0]):
                    continue
                pic = pictures(padded, idx)
                uniq, inv = np.unique(pic, return_inverse=True)
                gone = np.array([is_simple(u, connectivity) and not (curve and bin(int(u) & N26).count("1") == 1) for u in uniq],
                                dtype=bool)[inv]
                inner[idx[0][gone], idx[1][gone], idx[2][gone]] = False
                cleared += int(gone.sum())
        if not cleared:
            return inner.copy(), iterations


def nodes(skel):
    """-> dict: ends, junctions (bool volumes), voxels, end_points, junction_voxels, isolated."""
    skel = np.asarray(skel, dtype=bool)
    n = neighbour_counts(skel)
    ends, junctions = skel & (n == 1), skel & (n >= 3)
    return dict(ends=ends, junctions=junctions, voxels=int(skel.sum()), end_points=int(ends.sum()),
                junction_voxels=int(junctions.sum()), isolated=int((skel & (n == 0)).sum()))


# ------------------------------------------------------------------------------------------------ shapes
def ball(shape, centre, radius):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius * radius


def torus(shape, centre, major, minor):
    """A torus around the z axis through `centre`."""
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    rho = np.sqrt((y - centre[1]) ** 2.0 + (x - centre[2]) ** 2.0)
    return (rho - major) ** 2 + (z - centre[0]) ** 2.0 <= minor * minor


def shell(shape, centre, outer, inner):
    return ball(shape, centre, outer) & ~ball(shape, centre, inner)


def noise(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density
