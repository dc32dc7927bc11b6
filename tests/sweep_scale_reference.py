"""Host side of the scale tier of the tiled fixed-point sweeps (tests/test_gpu_sweep_scale.py): geodesic distance, geodesic
zones and their cut, grey reconstruction and homotopic thinning on volumes of more than 2560 tiles of 8 x 8 x 64 voxels -- more
workgroups than the card keeps resident, so that a sweep drains in several waves and a writer marks tiles that have not started,
have finished or run beside it.  The per-voxel Python references of the feature tiers (geodesic_reference.dijkstra,
zones_reference.zones, reconstruct_reference.flood) do not reach that size; three devices stand in for them, all exact:

1. Certificates, one pass of NumPy over the volume.  distance_defects(): a float32 map d is THE geodesic map iff it is +inf at
   unset voxels, 0.0 at set seeds, d(p) == min over the set neighbours q of fl32(d(q) + w(q, p)) at every other set voxel, and
   every finite fl32(d(q) + w) formed is > d(q).  The strictness makes the solution unique: take the voxels in the order of d;
   the smallest non-seed value is the sum over a strictly smaller neighbour, which is a seed's, and so on upwards -- and a map
   with a self-supporting plateau of finite values in a component without a seed is caught by reach_defects(), which holds
   isfinite(d) to the components of a CPU labelling that hold a seed.  zone_defects(): given such a d, zone is 0 where d is
   +inf, the marker's label at a marker voxel and elsewhere the minimum of zone(q) over the tight edges q -> p; d rises
   strictly along a tight edge, so the tight graph is acyclic and this is unique as well.  The cut is pointwise:
   zones_reference.cut is whole-volume already.
2. Level sets, for a reconstruction whose maps hold a handful of values: g(p) = max(m'(p), max{L <= f(p) : the component of p
   in {set and f >= L} holds a voxel with m' >= L}), L over the values of f and m'.  One labelling per distinct set
   {set and f >= L} (scipy.ndimage.label through topology_reference.label), kept in a small cache keyed by the set's bits.
3. Mosaics.  All four operators are local to a 26-connected component, so a large volume assembled from the small fixtures of
   the feature tiers, their boxes two clear voxels apart, has the assembled small references as its reference.  Every offset is
   even (thinning's subfields are parities: at odd offsets the skeleton of a block is another one); the distance weights of a
   block at slice z0 are the rows z0 .. of the large volume's table, so a spacing that changes along z stays exact.

The volumes are seeded and pinned by the SHA-256 of their packed bits, as in scale_reference.py.  Nothing here calls the
product; tests/test_sweep_scale_reference_cpu.py holds every device above to the per-feature references on the small fixtures."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import geodesic_reference as G  # noqa: E402
import reconstruct_reference as R  # noqa: E402
import skeleton_reference as S  # noqa: E402
import topology_reference as T  # noqa: E402
import zones_reference as Z  # noqa: E402

F32 = np.float32
INF = np.float32(np.inf)
INF_BITS = 0x7f800000
TILE = (8, 8, 64)
RESIDENT = 2048                      # workgroups of 256 threads an MI355X holds at once: 256 CUs x 4 SIMDs x 8 waves / 4
FLOOR = 2560                         # the least tile count of a volume of this tier
SHAPE = (66, 130, 1030)              # 9 x 17 x 17 = 2601 tiles, 8.8 M voxels; a ragged last word, ragged last tile rows in y and z
NOISE_SEED, NOISE_DENSITY = 7, 0.6
LATTICE_SEED, LATTICE_PITCH, LATTICE_BAR, LATTICE_KNOCK, LATTICE_BALL = 11, 12, 4, 0.02, 24
SHARE = 0.8                          # of the set voxels, at least, lie in the components that hold a seed

# SHA-256 of components_reference.pack(volume).tobytes()
SHA256 = {"noise": "c0d7a667d85827114a0988fd0194533020702b2e626d6f2a56032ebe2b974763",
          "lattice": "1a9c8f011a6251fbf854546be4c8bf975e144bea17c9c6ed198c7e0c74adc1dc",
          # the assembled volumes of the three mosaics: a change of a fixture or of layout() shows here
          "geo": "fd3276844559c1be3340b6193d28f8caea2fa2cfee3b243c633cdc3d4eb83fe8",
          "recon": "2386bd55291bb1c92b42b113206befdb300980ed4b66bfa1a2e13c2e2ba0cb18",
          "thin": "c5de3fd4b2a0841b0a96e20f4a4b6d4011bec1d9227d9663ec5b82a1c56af053"}
VOXELS = {"noise": 5301349, "lattice": 2427805, "geo": 392674, "recon": 1136539, "thin": 728844}
BLOCKS = {"geo": 72, "recon": 104, "thin": 68}
# (name, connectivity) -> components, measured with topology_reference.label
COUNTS = {("noise", 6): 24803, ("noise", 26): 1, ("lattice", 6): 2, ("lattice", 26): 1}

_volumes = {}


def tile_grid(shape):
    """-> (tile rows in z, in y, words per row, tiles)."""
    tz, ty, wx = -(-shape[0] // TILE[0]), -(-shape[1] // TILE[1]), -(-shape[2] // TILE[2])
    return tz, ty, wx, tz * ty * wx


def tile_of(p):
    return tuple(int(a) // t for a, t in zip(p, TILE))


def noise(shape=SHAPE, seed=NOISE_SEED, density=NOISE_DENSITY):
    return np.random.default_rng(seed).random(shape) < density


def lattice(shape=SHAPE, seed=LATTICE_SEED, radius=LATTICE_BALL):
    """Bars LATTICE_BAR voxels thick on a pitch of LATTICE_PITCH along all three axes, LATTICE_KNOCK of the voxels knocked out,
    and a solid ball in the middle: its tiles keep working for many iterations while the lattice's tiles rest."""
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    a, b, c = (z % LATTICE_PITCH) < LATTICE_BAR, (y % LATTICE_PITCH) < LATTICE_BAR, (x % LATTICE_PITCH) < LATTICE_BAR
    v = ((a & b) | (a & c) | (b & c)) & ~(np.random.default_rng(seed).random(shape) < LATTICE_KNOCK)
    return v | S.ball(shape, tuple(s // 2 for s in shape), radius)


MAKERS = {"noise": noise, "lattice": lattice}


def volume(name):
    """The bool volume, generated once and held to its pinned hash."""
    if name not in _volumes:
        v = MAKERS[name]()
        assert digest(C.pack(v)) == SHA256[name], "np.random.default_rng draws another volume here: %s is not the pinned one" % name
        v.setflags(write=False)
        _volumes[name] = v
    return _volumes[name]


def digest(bits):
    return hashlib.sha256(np.ascontiguousarray(bits).tobytes()).hexdigest()


def seeded_share(v, seeds, labels):
    """The share of the set voxels that lie in the components (of the CPU labelling `labels`) that hold a set seed."""
    v = np.asarray(v) != 0
    return float(reached(v, seeds, labels).sum()) / max(1, int(v.sum()))


def reached(v, seeds, labels):
    """The union of the components of `labels` that hold a set seed -> bool volume."""
    v = np.asarray(v) != 0
    touched = np.zeros(int(labels.max()) + 1, dtype=bool)
    touched[labels[G.seeds_mask(v.shape, seeds) & v]] = True
    touched[0] = False
    return touched[labels]


# ----------------------------------------------------------------------------- 1. certificates
def _padded(a, fill):
    out = np.full(tuple(s + 2 for s in a.shape), fill, dtype=a.dtype)
    out[1:-1, 1:-1, 1:-1] = a
    return out


def _at(padded, off, shape):
    """The view b[p] = a[p + off] of a volume padded by one voxel."""
    return padded[1 + off[0]:1 + off[0] + shape[0], 1 + off[1]:1 + off[1] + shape[1], 1 + off[2]:1 + off[2] + shape[2]]


def _column(wxy, wz, nz, off):
    """Per slice k of p the float32 weight of the step between p and p + off; +inf where p + off leaves the stack in z."""
    return np.array([G.step_weight(wxy, wz, k, off) if 0 <= k + off[0] < nz else np.inf for k in range(nz)], dtype=F32)[:, None, None]


def _describe(at, shape, d, best, offs, pad, cols):
    z, y, x = (int(a) for a in at)
    rows = []
    for off, col in zip(offs, cols):
        q = (z + off[0], y + off[1], x + off[2])
        dq = pad[q[0] + 1, q[1] + 1, q[2] + 1]
        if np.isfinite(dq):
            rows.append("%s in tile %s: %r + %r = %r" % (q, tile_of(q), dq, col[z, 0, 0], F32(dq + col[z, 0, 0])))
    side = ("the voxel is stale: a neighbour's lower value has not arrived" if not d[at] <= best[at] else
            "the voxel is lower than any neighbour supports")
    return "voxel %s in tile %s holds %r, its neighbours give %r (%s); finite neighbours: %s" % (
        (z, y, x), tile_of(at), d[at], best[at], side, "; ".join(rows) or "none")


def distance_defects(v, seeds, d, wxy, wz, connectivity):
    """None when the float32 map d is the geodesic map of the seeds inside v under the weights (bit patterns compared), else a
    sentence about the first bad voxel: its tile, its neighbours' values and which side is stale.  isfinite(d) against the
    components is reach_defects()'s part."""
    v = np.asarray(v) != 0
    d = np.asarray(d)
    if d.dtype != np.float32 or d.shape != v.shape:
        return "the map is %s %s, not float32 %s" % (d.dtype, d.shape, v.shape)
    d = np.ascontiguousarray(d)
    bits = d.view(np.uint32)
    seeds = G.seeds_mask(v.shape, seeds) & v
    bad = ~v & (bits != INF_BITS)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d unset voxels are not +inf, the first %s in tile %s holds %r" % (bad.sum(), at, tile_of(at), d[at])
    bad = seeds & (bits != 0)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d seeds are not 0.0, the first %s in tile %s holds %r" % (bad.sum(), at, tile_of(at), d[at])
    pad = _padded(d, INF)
    best = np.full(v.shape, INF, dtype=F32)
    offs = G.offsets(connectivity)
    cols = [_column(wxy, wz, v.shape[0], off) for off in offs]
    for off, col in zip(offs, cols):
        dq = _at(pad, off, v.shape)
        cand = dq + col                                              # float32 + float32: one rounded addition
        np.minimum(best, cand, out=best)
        loose = np.isfinite(cand) & ~(cand > dq) & v
        if loose.any():
            at = tuple(np.argwhere(loose)[0])
            return "the sum %r + %r into voxel %s in tile %s does not exceed its left operand: the map is not certified" % (
                dq[at], col[at[0], 0, 0], at, tile_of(at))
    bad = v & ~seeds & (best.view(np.uint32) != bits)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d voxels are no minimum over their neighbours; %s" % (bad.sum(), _describe(at, v.shape, d, best, offs, pad, cols))
    return None


def reach_defects(v, seeds, d, labels):
    """None when isfinite(d) is the union of the components of the CPU labelling `labels` that hold a set seed."""
    want = reached(v, seeds, labels)
    bad = np.isfinite(np.asarray(d)) != want
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d voxels are finite where no seed reaches or +inf where one does, the first %s in tile %s holds %r" % (
            bad.sum(), at, tile_of(at), np.asarray(d)[at])
    return None


def zone_defects(v, markers, dist, zone, wxy, wz, connectivity):
    """None when the int32 map `zone` is the zone map of the int32 marker map over the CERTIFIED distance map `dist`."""
    v = np.asarray(v) != 0
    zone, dist = np.asarray(zone), np.ascontiguousarray(dist)
    if zone.dtype != np.int32 or zone.shape != v.shape:
        return "the map is %s %s, not int32 %s" % (zone.dtype, zone.shape, v.shape)
    m = np.asarray(markers).astype(np.int64)
    seeds = v & (m > 0)
    finite = v & np.isfinite(dist)
    bad = (~finite & (zone != 0)) | (finite & (zone <= 0))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d voxels: a zone where dist is +inf or none where it is finite, the first %s in tile %s: zone %d, dist %r" % (
            bad.sum(), at, tile_of(at), zone[at], dist[at])
    bad = seeds & (zone != m)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return "%d marker voxels lost their label, the first %s in tile %s: zone %d, marker %d" % (bad.sum(), at, tile_of(at), zone[at], m[at])
    pad, zpad = _padded(dist, INF), _padded(zone.astype(np.int64), Z.NONE)
    best = np.full(v.shape, Z.NONE, dtype=np.int64)
    for off in G.offsets(connectivity):
        cand = _at(pad, off, v.shape) + _column(wxy, wz, v.shape[0], off)
        tight = finite & (cand == dist)                              # +inf + w is no finite dist
        np.minimum(best, np.where(tight, _at(zpad, off, v.shape), Z.NONE), out=best)
    bad = finite & ~seeds & (best != zone)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        side = "the voxel is stale: a lower label has not arrived" if zone[at] > best[at] else "the voxel is below every tight neighbour"
        return "%d voxels are no minimum over their tight edges, the first %s in tile %s: zone %d, the tight neighbours give %d (%s)" % (
            bad.sum(), at, tile_of(at), zone[at], best[at], side)
    return None


# ----------------------------------------------------------------------------- 2. reconstruction by level sets
LEVELS = 8                           # distinct labellings one call may ask for
_LABELLINGS = {}                     # (connectivity, digest of the packed set) -> (labels, n); the oldest goes first
LABELLINGS_KEPT = 12


def _labelled(region, connectivity):
    key = (connectivity, region.shape, digest(np.packbits(region)))
    if key not in _LABELLINGS:
        while len(_LABELLINGS) >= LABELLINGS_KEPT:
            _LABELLINGS.pop(next(iter(_LABELLINGS)))
        _LABELLINGS[key] = T.label(region, connectivity)
    return _LABELLINGS[key]


def reconstruct(v, mask, marker, connectivity=26):
    """reconstruct_reference.reconstruct by another definition, for maps with few values: g >= L at p exactly when m'(p) >= L, or
    f(p) >= L and the component of p in {set and f >= L} holds a voxel with m' >= L.  L runs over the values of f and m' on the
    set voxels; the sets {f >= L} differ only from one value of f to the next: at most LEVELS labellings."""
    v = np.asarray(v) != 0
    f = R.canon(mask)
    with np.errstate(invalid="ignore"):
        m = np.where(v, np.minimum(R.canon(marker), f), R.NEG).astype(F32)
    flevels = np.unique(f[v])
    assert len(flevels) <= LEVELS, "the mask holds %d values: this reference is for maps with at most %d" % (len(flevels), LEVELS)
    g = m.copy()
    for level in np.unique(np.concatenate([flevels, m[v]])):
        if not (flevels >= level).any():
            continue                                                 # above every ceiling (cannot happen: m' <= f)
        region = v & (f >= level)
        labels, n = _labelled(region, connectivity)
        holds = np.zeros(n + 1, dtype=bool)
        holds[labels[region & (m >= level)]] = True
        holds[0] = False
        g = np.where(holds[labels] & (g < level), F32(level), g).astype(F32)
    return np.where(v, g, F32(0.0)).astype(F32)


def h_maxima(v, values, h, connectivity=26):
    return R.h_maxima(v, values, h, connectivity, how=reconstruct)


def regional_maxima(v, values, connectivity=26):
    return R.regional_maxima(v, values, connectivity, how=reconstruct)


def extended_maxima(v, values, h, connectivity=26):
    return R.extended_maxima(v, values, h, connectivity, how=reconstruct)


ZERO_LEVELS = np.array([-1.0, -0.0, 0.0, 1.0, 2.0, 3.0], dtype=F32)      # five values: the two zeros are one


def level_map(shape, seed):
    """A random map over ZERO_LEVELS: five levels, zeros of both signs among them."""
    return ZERO_LEVELS[np.random.default_rng(seed).integers(0, len(ZERO_LEVELS), shape)]


def sparse_marker(shape, seed, share=0.001):
    """-1 nearly everywhere, a level of ZERO_LEVELS at `share` of the voxels."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < share, ZERO_LEVELS[rng.integers(0, len(ZERO_LEVELS), shape)], F32(-1.0)).astype(F32)


# ----------------------------------------------------------------------------- 3. mosaics
def _even(a):
    return a + (a & 1)


def layout(shape, sizes, seed, gap=2):
    """Shelf packing of blocks of the given sizes, taken in turn until the volume is full -> [(index into sizes, (z0, y0, x0))].
    Layers in z, rows in y, blocks along x; every cursor and every jitter is even; boxes are at least `gap` clear voxels apart.
    The jitter in z depends on the layer and the kind of block only, so that blocks of one kind in one layer share the rows of
    the z weights; in y and x it is drawn from the generator."""
    rng = np.random.default_rng(seed)
    out, i, z, layer = [], 0, 0, 0
    while z < shape[0]:
        y, top_z = 0, z
        while y < shape[1]:
            x, top_y = 0, y
            while x < shape[2]:
                jy, jx = 2 * int(rng.integers(0, 4)), 2 * int(rng.integers(0, 32))
                for k in [(i + t) % len(sizes) for t in range(len(sizes))]:
                    bz, by, bx = sizes[k]
                    for z0, y0, x0 in ((z + 2 * ((layer + k) % 4), y + jy, x + jx), (z, y, x + jx), (z, y, x)):
                        if z0 + bz <= shape[0] and y0 + by <= shape[1] and x0 + bx <= shape[2]:
                            break
                    else:
                        continue
                    break
                else:
                    break                                            # nothing fits at this x: the row is full
                out.append((k, (z0, y0, x0)))
                i += 1
                x = _even(x0 + bx + gap)
                top_y, top_z = max(top_y, _even(y0 + by + gap)), max(top_z, _even(z0 + bz + gap))
            if top_y == y:
                break                                                # an empty row: the layer is full
            y = top_y
        if top_z == z:
            break
        z, layer = top_z, layer + 1
    return out


RULES = ("inside", "even", "apart", "residues", "boundary")


def layout_defects(shape, sizes, placed, gap=2, x_residues=16, rules=RULES):
    """None when the placement keeps the named rules of the tier (all of them by default), else the rule it breaks."""
    lo = np.array([p for _, p in placed], dtype=np.int64)
    hi = lo + np.array([sizes[k] for k, _ in placed], dtype=np.int64)
    if "inside" in rules and (not len(placed) or (lo < 0).any() or (hi > np.array(shape)).any()):
        return "a block leaves the volume, or there is none"
    if "even" in rules and (lo & 1).any():
        return "an odd offset"
    apart = ((lo[:, None, :] - hi[None, :, :] >= gap) | (lo[None, :, :] - hi[:, None, :] >= gap)).any(axis=2)
    np.fill_diagonal(apart, True)
    if "apart" in rules and not apart.all():
        return "two boxes are less than %d clear voxels apart" % gap
    for axis, need in ((0, 4), (1, 4), (2, x_residues)):
        if "residues" in rules and len(set((lo[:, axis] % TILE[axis]).tolist())) < need:
            return "the offsets cover fewer than %d residues modulo %d on axis %d" % (need, TILE[axis], axis)
    for axis in range(3):
        if "boundary" in rules and not (lo[:, axis] // TILE[axis] != (hi[:, axis] - 1) // TILE[axis]).any():
            return "no block lies across a tile boundary on axis %d" % axis
    return None


def assemble(shape, parts, placed, fill, dtype=None):
    """The volume-sized array that holds parts[i] at the offset of placed[i] and `fill` elsewhere."""
    out = np.full(shape, fill, dtype=dtype if dtype is not None else np.asarray(parts[0]).dtype)
    for part, (_, (z0, y0, x0)) in zip(parts, placed):
        bz, by, bx = part.shape
        out[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] = part
    return out


def block_weights(wz, z0, nz):
    """The rows of the large volume's z weights a block of nz slices at slice z0 sees, in the form geodesic_reference takes."""
    rows = wz[z0:z0 + nz - 1]
    return rows.copy() if len(rows) else np.zeros((1, 4), dtype=F32)


def shifted_labels(m, offset):
    """The marker map with `offset` added to its positive entries: order-preserving inside the block."""
    m = np.asarray(m).astype(np.int64)
    out = np.where(m > 0, m + int(offset), m)
    assert out.max() <= np.iinfo(np.int32).max
    return out.astype(np.int32)


# ----------------------------------------------------------------------------- the parts of the three mosaics
MOSAIC_SEEDS = {"geo": 41, "recon": 42, "thin": 43}
_parts = {}


def geo_parts():
    """name -> (volume, int32 marker map): the fixtures of the geodesic and zone tiers, scattered labels, entries on unset
    voxels and negative entries among them; the thin paths carry a marker at each end."""
    if "geo" not in _parts:
        fx = G.fixtures()
        out = {}
        for name, every in (("noise_tiles", 97), ("noise_words", 97), ("noise_031", 61)):
            out[name] = (fx[name], Z.scattered_markers(fx[name], every))
        out["dumbbell"] = (Z.dumbbell(), Z.scattered_markers(Z.dumbbell(), 211))
        for name in ("weave", "coil", "ring"):
            out[name] = (fx[name], Z.end_markers(fx[name]))
        _parts["geo"] = out
    return _parts["geo"]


def recon_parts():
    """name -> (volume, mask, marker, reference function): float maps on noise, the inside distance of the scene of balls with a
    marker 2.5 below it, and the corridor through every tile of its block with a bottleneck in the middle."""
    if "recon" not in _parts:
        out = {}
        for i, (shape, density) in enumerate(((R.SHAPES[0], 0.7), (R.SHAPES[2], 0.3), (R.SHAPES[2], 0.7))):
            out["float%d" % i] = (R.noise(shape, density, 50 + i), R.float_map(shape, 60 + i, signed=True),
                                  R.float_map(shape, 70 + i, signed=True), R.reconstruct)
        scene = R.scene()
        f = R.unit_distance(scene)
        out["scene"] = (scene, f, R.h_marker(f, 2.5), R.reconstruct)
        v, path = R.corridor()
        f = np.full(v.shape, 5.0, dtype=F32)
        f[path[len(path) // 2]] = 2.0
        m = np.full(v.shape, -1.0, dtype=F32)
        m[path[0]] = 9.0
        out["corridor"] = (v, f, m, R.flood)                         # one sweep a voxel: the whole-volume sweeps would take hours
        _parts["recon"] = out
    return _parts["recon"]


def thin_parts():
    """name -> (volume, anchors or None): noise of three densities (anchored), a ball, a torus, a shell and the scene of balls."""
    if "thin" not in _parts:
        out = {}
        for i, density in enumerate((0.3, 0.5, 0.7)):
            shape = (19, 21, 150) if i else (11, 13, 70)
            out["noise%d" % int(10 * density)] = (S.noise(shape, density, int(100 * density)), S.noise(shape, 0.02, 7 + i))
        out["ball"] = (S.ball((25, 25, 30), (12, 12, 14), 10), None)
        out["torus"] = (S.torus((9, 31, 31), (4, 15, 15), 10, 3), None)
        out["shell"] = (S.shell((15, 15, 15), (7, 7, 7), 6, 3), None)
        out["grains"] = (np.ascontiguousarray(R.scene()), None)
        _parts["thin"] = out
    return _parts["thin"]


PARTS = {"geo": geo_parts, "recon": recon_parts, "thin": thin_parts}


def mosaic(family, shape=SHAPE):
    """-> (names of the parts, [(index into the names, offset)]) of the family's mosaic; layout_defects() holds it to the rules."""
    parts = PARTS[family]()
    names = list(parts)
    return names, layout(shape, [parts[n][0].shape for n in names], MOSAIC_SEEDS[family])


def corner_seed(v, labels):
    """The first set voxel in raster order whose component holds at least SHARE of the set voxels -> int64 (1, 3), or None."""
    sizes = np.bincount(labels.reshape(-1))
    big = np.flatnonzero(sizes[1:] >= SHARE * sizes[1:].sum()) + 1
    if not len(big):
        return None
    at = int(np.argmax(labels.reshape(-1) == big[0]))
    return np.array([np.unravel_index(at, labels.shape)], dtype=np.int64)


def every_tile_seeds(v, every=97):
    """geodesic_reference.default_seeds and the first set voxel of every tile that holds one: the first sweep finds every tile
    dirty -> int64 (n, 3), some rows on unset voxels (ignored)."""
    v = np.asarray(v) != 0
    on = np.argwhere(v)
    _, ty, wx, _ = tile_grid(v.shape)
    tile = ((on[:, 0] // TILE[0]) * ty + on[:, 1] // TILE[1]) * wx + on[:, 2] // TILE[2]
    _, first = np.unique(tile, return_index=True)
    return np.concatenate([G.default_seeds(v, every), on[first]]).astype(np.int64)
