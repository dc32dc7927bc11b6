"""Host side of the scale tier (tests/test_gpu_scale.py): volumes whose run tables, component tables and point-cloud tiles
cross 2^20 entries -- where the one-workgroup middle step of every scan (cc_scan1_kernel, pc_scan_kernel) takes a second turn
of its loop -- and references that stay cheap at a million components.

The volumes are np.random.default_rng(seed).random(shape) < p; nothing is stored.  SHA256 pins the packed bits and COUNTS what
components_reference.label finds in them, so that a NumPy whose generator differs fails loudly instead of moving a volume off
its boundary.

The helpers of the per-feature references that do not scale (component_props_reference.slice_counts builds a dense (n, nz)
array, topology_reference.components loops over every component) have sparse counterparts here; tests/test_scale_reference_cpu.py
holds every one of them to the helper it stands in for, on the small fixtures, with ==.

slice_entries():  the non-zero entries of component_props_reference.slice_counts, sorted by component, then slice.
volume_of():      component_props_reference.volume_of over those entries: the same float64 additions, ascending z per component.
properties():     component_props_reference.properties for given rows, from those sums.
crop():           the mask `labels == c` inside the component's box plus one voxel of margin: the existing per-component
                  references (topology_reference.euler / cavities, surface_reference.counts) then run on a few hundred
                  selected components only.
topology_rows():  topology_reference.components' rows for selected components.
surface_counts(): surface_reference.component_counts' rows for ONE component, as (first slice, counts of the crop's slices).
owners():         cavities_reference.owners_of from two label arrays."""
import hashlib

import numpy as np

import cavities_reference as R
import component_props_reference as P
import components_reference as C
import surface_reference as S
import topology_reference as T

EDGE = 2 ** 20               # CC_SCAN_TILE * 1024 entries: one turn of cc_scan1_kernel's loop
PC_TILE = 2048               # words per tile of the point cloud (csrc/volume.hip)

# name -> (shape, density, seed, complemented)
VOLUMES = {"rows_edge": ((1024, 1024, 3), 0.4, 21, False),
           "rows_past": ((1030, 1024, 3), 0.4, 22, False),
           "runs_past": ((64, 128, 512), 0.5, 5, False),
           "comps_past": ((160, 128, 640), 0.15, 5, False),
           "dense": ((160, 128, 640), 0.15, 5, True)}
# SHA-256 of components_reference.pack(volume).tobytes()
SHA256 = {"rows_edge": "5fff37aa91dca8cdf6f67297a3e7858da9ac8420fd30d297ea1e18695b617181",
          "rows_past": "d613fceb506a3772aff58e9d311741e7327c28302cfa995338c051ed036aba72",
          "runs_past": "6d2a552a954336f4513b817f244d9b3dde1733a60b6c075ea374050a9f902a06",
          "comps_past": "2272eda20ebcbef57fd45c88c53c90a9f41e599859b44003dc983a691027f895",
          "dense": "395d02c741405225d5fe00edefb18a8627bf6210b612c4e6b5403e244d5e08ba"}
# runs of each volume, and (name, connectivity) -> components, measured with components_reference.label
RUNS = {"rows_edge": 922053, "rows_past": 927673, "runs_past": 1050755, "comps_past": 1670896, "dense": 1685186}
COUNTS = {("rows_edge", 6): 135040, ("rows_edge", 26): 166, ("rows_past", 6): 135509, ("rows_past", 26): 179,
          ("runs_past", 6): 39669, ("runs_past", 26): 1, ("comps_past", 6): 1106315, ("comps_past", 26): 47498,
          ("dense", 6): 153, ("dense", 26): 1}
# comps_past under 6: the largest component, the components of at least 12 voxels, those of them with a 0-based index >= 2^20
COMPS_PAST_LARGEST, COMPS_PAST_GE12, COMPS_PAST_GE12_LATE = 41, 4820, 169
DENSE_CAVITIES = 1063875          # enclosed components of the complement of `dense` under 6: its cavities under foreground 26

_volumes = {}


def volume(name):
    """The bool volume, generated once."""
    if name not in _volumes:
        shape, p, seed, complemented = VOLUMES[name]
        v = np.random.default_rng(seed).random(shape) < p
        _volumes[name] = ~v if complemented else v
    return _volumes[name]


def digest(bits):
    return hashlib.sha256(np.ascontiguousarray(bits).tobytes()).hexdigest()


def packed(name):
    """components_reference.pack of the volume, held to the pinned hash."""
    bits = C.pack(volume(name))
    assert digest(bits) == SHA256[name], "np.random.default_rng(%d) draws another volume here: %s is not the pinned one" % (
        VOLUMES[name][2], name)
    return bits


def count_runs(v):
    """Maximal runs of set voxels along x."""
    v = np.asarray(v) != 0
    return int(np.count_nonzero(v[:, :, 0])) + int(np.count_nonzero(v[:, :, 1:] & ~v[:, :, :-1]))


# ----------------------------------------------------------------------------- voxels per component and slice, sparse
def slice_entries(labels, n):
    """-> (c, z, count), int64 each: the non-zero entries of P.slice_counts(labels, n)[c, z], sorted by c, then z."""
    nz = labels.shape[0]
    idx = np.flatnonzero(labels)
    key = (labels.reshape(-1)[idx].astype(np.int64) - 1) * nz + idx // (labels.shape[1] * labels.shape[2])
    key, count = np.unique(key, return_counts=True)
    return key // nz, key % nz, count.astype(np.int64)


def volume_of(entries, n, mm_x, mm_y, slice_depths):
    """P.volume_of for all n components from slice_entries(): (volume, moment), float64 (n,).  Round k adds the k-th entry of
    every component that has one: per component the additions of P.volume_of in ascending z, without the slices that add 0.0."""
    c, z, count = entries
    slice_depths = np.asarray(slice_depths, dtype=np.float64)
    zc = P.slice_centres(slice_depths)
    inside = z < len(slice_depths)
    c, z, count = c[inside], z[inside], count[inside]
    first = np.searchsorted(c, c)                                # where the entries of an entry's component start
    turn = np.arange(len(c)) - first
    v = count * (mm_x * mm_y * slice_depths)[z]
    w = v * zc[z]
    total, moment = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    order = np.argsort(turn, kind="stable")
    bounds = np.searchsorted(turn[order], np.arange(int(turn.max()) + 2 if len(turn) else 1))
    for a, b in zip(bounds, bounds[1:]):
        at = order[a:b]                                          # one entry per component at most
        total[c[at]] += v[at]
        moment[c[at]] += w[at]
    return total, moment


def properties(tab, sums, mm_y, mm_x, pick):
    """P.properties' dict for the 0-based rows `pick` (ascending); sums: volume_of() of all components."""
    pick = np.asarray(pick, dtype=np.int64)
    rows = tab[pick]
    vol, moment = sums[0][pick], sums[1][pick]
    cidx = rows[:, 7:10] / rows[:, 0][:, None]
    cmm = np.stack([moment / vol, cidx[:, 1] * mm_y, cidx[:, 2] * mm_x], axis=1) if len(pick) else np.zeros((0, 3))
    return {"labels": pick + 1, "voxels": rows[:, 0], "index_box": rows[:, 1:7], "index_sums": rows[:, 7:10],
            "volume_mm3": vol, "centroid_index": cidx, "centroid_mm": cmm}


# ----------------------------------------------------------------------------- one component at a time
def crop(labels, table_row, c):
    """-> (mask, box): `labels == c` (c 1-based) inside the inclusive index box of its measurement-table row plus one voxel of
    margin, cut at the faces of the stack; box: the three slices of that window."""
    lo, hi = table_row[1:7:2], table_row[2:7:2]
    box = tuple(slice(max(int(a) - 1, 0), min(int(b) + 2, s)) for a, b, s in zip(lo, hi, labels.shape))
    return labels[box] == c, box


def topology_rows(labels, tab, pick, k):
    """T.components' rows (euler, cavities, handles) for the 0-based components `pick` -> int64 (len(pick), 3)."""
    out = np.zeros((len(pick), 3), dtype=np.int64)
    for i, c in enumerate(pick):
        mask, _ = crop(labels, tab[c], int(c) + 1)
        out[i, 0], out[i, 1] = T.euler(mask, k), T.cavities(mask, k)
    out[:, 2] = 1 - out[:, 0] + out[:, 1]
    return out


def surface_counts(labels, tab, c):
    """S.component_counts(labels, n)[c] for the 0-based component c -> (z0, int64 (slices of the crop, 11)): the rows of every
    other slice are zero.  Where the margin was cut at a face, S.counts' own padding stands for the outside of the stack."""
    mask, box = crop(labels, tab[c], int(c) + 1)
    return box[0].start, S.counts(mask, labels[box] != 0)


def owners(fg_labels, bg_labels, n_bg):
    """R.owners_of from the label arrays of a volume and of its complement."""
    flat = bg_labels.reshape(-1)
    idx = np.flatnonzero(flat)
    first = np.zeros(n_bg + 1, dtype=np.int64)
    first[flat[idx][::-1]] = idx[::-1]                           # the last write is the lowest index
    first = first[1:]
    nx = bg_labels.shape[2]
    return np.where(first % nx > 0, fg_labels.reshape(-1)[np.maximum(first - 1, 0)], 0).astype(np.int64)


def cavity_rule(tab, shape, lo=0, hi=None):
    """bool (n_bg,): the components of a complement that are cavities inside the size window."""
    return R.enclosed(tab, shape) & R.window(tab[:, 0], lo, hi)


# ----------------------------------------------------------------------------- the point cloud past 1024 tiles
CLOUD_SHAPE = (130, 1024, 1024)
CLOUD_VOXELS = 50000
CLOUD_LATE = 1500            # of them drawn beyond word 1024 * PC_TILE


def cloud():
    """-> (linear voxel indices int64, ascending = raster order; bit words int64 (nz, ny, nx / 64)).  The first and the last
    voxel of the stack are set; no dense volume is made."""
    nz, ny, nx = CLOUD_SHAPE
    total = nz * ny * nx
    rng = np.random.default_rng(8)
    late = 64 * 1024 * PC_TILE
    lin = np.unique(np.concatenate([[0, total - 1], rng.integers(0, total, CLOUD_VOXELS - CLOUD_LATE),
                                    rng.integers(late, total, CLOUD_LATE)]).astype(np.int64))
    words = np.zeros(total // 64, dtype=np.uint64)
    np.bitwise_or.at(words, lin >> 6, np.uint64(1) << (lin & 63).astype(np.uint64))
    return lin, words.view(np.int64).reshape(nz, ny, nx // 64)
