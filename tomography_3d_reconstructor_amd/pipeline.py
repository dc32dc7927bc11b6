"""Device-resident pipeline: mask stack -> bit volume -> field -> marching cubes -> final mesh.

Everything here operates on torch tensors that live in HBM and launches the hand-written HIP
kernels of libtomo_hip.so on torch's current stream.  The two drop-in classes
(voxel_processor.py / surface_extractor.py) are thin host adapters over these functions; bench.py
times these functions directly with the inputs already resident.

Reference lines each function replaces are given in its docstring.
"""
import itertools
import math
import os
import threading
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib


# which way the size hints and the unique stage of the surfaces of this process went (tests and tools read the deltas)
COUNTERS = dict.fromkeys(("na_hint_hit", "na_hint_miss", "mc3_hint_hit", "mc3_hint_miss", "mc3_sort_fused", "mc3_sort_library",
                          "mc3_exact", "mc3_general_unique", "mc3_degenerate", "components_label", "components_expand",
                          "components_filter", "slab_components_label", "slab_components_seam", "slab_components_merge",
                          "slab_components_expand", "slab_components_filter", "distance_transform", "distance_offset",
                          "components_measure", "components_zhist", "components_moments", "components_euler",
                          "components_cavities", "local_thickness", "opening_volume", "components_surface", "components_fill",
                          "components_cavity_owners", "component_thickness", "components_value", "components_levels", "component_caliper",
                          "geodesic_calls", "geodesic_sweeps", "component_geodesic", "zone_calls", "zone_sweeps", "zone_cuts",
                          "separate_components", "zone_contacts", "contact_launches", "recon_calls", "recon_sweeps",
                          "thin_calls", "thin_iterations", "thin_passes", "thin_nodes", "component_skeleton",
                          "skeleton_branches", "branch_split", "skeleton_branches_hist", "branch_attach", "branch_lookup", "branch_clear",
                          "prune_rounds", "components_profile", "branch_profile", "prune_relative", "components_breadth",
                          "chord_lengths", "two_point"), 0)
NA_HINTS = os.environ.get("TOMO_NA_HINTS", "1") not in ("", "0")   # marching_cubes: launch ahead of the first count download
_NA_HINT = {}
LIST_LIMIT = 2 ** 31        # active-voxel list entries / vertices / triangles one pass can index (int32 offsets in mc.hip, mesh.hip);
MESH_LIMIT = 2 ** 31        # beyond them marching_cubes raises TomoError (the drop-in class then returns None, as the reference would)
PACK_CLOSE_FUSED = os.environ.get("TOMO_PACK_CLOSE", "1") not in ("", "0")   # pack_closed: one pass over the mask (A/B switch)
FIELD_FROM_BITS = True      # False: materialise the extended bit volume first (tomo_extend_bits + tomo_field_fill)
# extract_surface: do not materialise the parts of the float field that marching cubes cannot read (same mesh, ~0.4 ms less
# per 1024^3 pass).  Off by default: the reference's path, and bench.py's roofline, speak of a dense per-voxel field.
FIELD_SPARSE = os.environ.get("TOMO_FIELD_SPARSE", "0") not in ("", "0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


@dataclass
class BitVolume:
    """Bit-packed boolean volume on the device: int64 words (nz, ny, wx), bit b of word w = voxel 64w+b."""
    bits: torch.Tensor
    shape: tuple  # (nz, ny, nx)

    @property
    def device(self):
        return self.bits.device


@dataclass
class Field:
    """float32 field (Nz, Ny, pitch); padded column X is stored at column xorg + X."""
    data: torch.Tensor
    Nz: int
    Ny: int
    Nx: int
    pitch: int
    xorg: int
    signs: torch.Tensor = None     # sign records (Nz, S, NyP, 4) int64 for `signs_level`, or None
    signs_level: float = 0.5
    gcls: torch.Tensor = None      # class of every 16-row group of records (Nz, NyP / 16, S) uint8: 0 / 1 constant, 2 stored
    sparse: bool = False           # data holds floats only where marching cubes at signs_level reads them

    def dense(self):
        return self.data[:, :, self.xorg:self.xorg + self.Nx]


@dataclass
class RawMesh:
    """Output of marching cubes before finalisation."""
    vkey: torch.Tensor     # (V,) int64 vertex keys, ascending
    vpos: torch.Tensor     # (V,3) float32 (z,y,x) as skimage returns them
    faces32: torch.Tensor  # (F,3) int32 provisional vertex indices, triangle order = reference order


# ----------------------------------------------------------------------------- binary stages
def _mask_u8(mask: torch.Tensor) -> torch.Tensor:
    """A (nz, ny, nx) bool / uint8 mask stack as the contiguous uint8 tensor the pack kernels read."""
    if mask.dim() != 3:
        raise ValueError("mask must be (nz, ny, nx)")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise TypeError("mask must be bool or uint8")
    return mask.contiguous()


def pack(mask: torch.Tensor, out: torch.Tensor = None) -> BitVolume:
    """np.stack(mask_images) (voxel_processor.py:46) as a device uint8/bool tensor -> BitVolume (into `out`, a contiguous
    int64 (nz, ny, words) tensor -- e.g. the middle of a halo-extended buffer -- when given)."""
    mask = _mask_u8(mask)
    nz, ny, nx = mask.shape
    L = _lib.lib()
    wx = L.tomo_words_per_row(nx)
    if out is None:
        bits = torch.empty((nz, ny, wx), dtype=torch.int64, device=mask.device)
    else:
        if tuple(out.shape) != (nz, ny, wx) or out.dtype != torch.int64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous int64 (nz, ny, words) tensor")
        bits = out
    _lib.check(L.tomo_pack_bits(_p(mask), _p(bits), nz, ny, nx, _stream()), "tomo_pack_bits")
    return BitVolume(bits, (nz, ny, nx))


def unpack(vol: BitVolume) -> torch.Tensor:
    nz, ny, nx = vol.shape
    out = torch.empty((nz, ny, nx), dtype=torch.uint8, device=vol.device)
    _lib.check(_lib.lib().tomo_unpack_bits(_p(vol.bits), _p(out), nz, ny, nx, _stream()), "tomo_unpack_bits")
    return out.view(torch.bool)


def popcount_async(vol: BitVolume) -> torch.Tensor:
    """np.sum(voxel_data) (voxel_processor.py:51) -> 1-element int64 device tensor."""
    nz, ny, nx = vol.shape
    cnt = torch.zeros(1, dtype=torch.int64, device=vol.device)
    _lib.check(_lib.lib().tomo_popcount(_p(vol.bits), nz, ny, nx, _p(cnt), _stream()), "tomo_popcount")
    return cnt


def pack_threshold(grey: torch.Tensor, threshold) -> BitVolume:
    """`img >= threshold` (image_loader.py:108) of a device uint8 (nz, ny, nx) grey stack, straight to a BitVolume.
    For integer grey levels g >= t is g >= ceil(t), so a fractional threshold is rounded UP (199.5 -> 200)."""
    if grey.dim() != 3 or grey.dtype != torch.uint8:
        raise TypeError("grey stack must be uint8 (nz, ny, nx)")
    grey = grey.contiguous()
    nz, ny, nx = grey.shape
    L = _lib.lib()
    bits = torch.empty((nz, ny, L.tomo_words_per_row(nx)), dtype=torch.int64, device=grey.device)
    _lib.check(L.tomo_pack_threshold(_p(grey), _p(bits), nz, ny, nx, int(math.ceil(threshold)), _stream()), "tomo_pack_threshold")
    return BitVolume(bits, (nz, ny, nx))


def slice_counts(vol: BitVolume) -> torch.Tensor:
    """np.sum(voxel_data[z]) for every z (volume_calculator.py:33) -> int64 (nz,) device tensor."""
    nz, ny, nx = vol.shape
    counts = torch.empty(nz, dtype=torch.int64, device=vol.device)
    _lib.check(_lib.lib().tomo_slice_popcounts(_p(vol.bits), nz, ny, nx, _p(counts), _stream()), "tomo_slice_popcounts")
    return counts


def bounding_box(vol: BitVolume):
    """min / max of np.where(voxel_data) per axis (volume_calculator.py:40-44, 62-72) -> (zmin, zmax, ymin, ymax,
    xmin, xmax) as Python ints, or None for an empty volume."""
    nz, ny, nx = vol.shape
    box = torch.empty(6, dtype=torch.int32, device=vol.device)
    _lib.check(_lib.lib().tomo_bbox(_p(vol.bits), nz, ny, nx, _p(box), _stream()), "tomo_bbox")
    b = [int(x) for x in box.cpu()]
    return None if b[1] < 0 else tuple(b)


# ----------------------------------------------------------------------------- point cloud
def point_cloud_z_table(slice_depths, nz, z0=0) -> np.ndarray:
    """The z column of generate_point_cloud (voxel_processor.py:110-119) for slices z0 .. z0 + nz - 1 -> float64 (nz,), on the
    host: the centre of slice z while z < len(slice_depths), the total depth beyond.  The kernel only looks it up."""
    d = np.asarray(slice_depths, dtype=np.float64)
    cum = np.cumsum(np.concatenate([[0], d]))
    z = np.arange(int(z0), int(z0) + int(nz))
    if len(d):
        zc = np.minimum(z, len(d) - 1)
        return np.where(z < len(d), cum[zc] + d[zc] / 2, cum[-1])
    return np.full(len(z), cum[-1])


def point_cloud_step(subsample_factor) -> int:
    """k of the rank rule: voxel_processor.py:104-105 subsamples only when the factor is > 1."""
    return int(subsample_factor) if subsample_factor > 1 else 1


def point_cloud_rows(n, k, rank_base=0):
    """The rows of n set voxels whose ranks start at rank_base, every k-th rank kept: (row_first, rows) -- this run is rows
    [row_first, row_first + rows) of the array of the whole stack.  Python ints."""
    n, k, rank_base = int(n), int(k), int(rank_base)
    row_first = -(-rank_base // k)
    return row_first, -(-(rank_base + n) // k) - row_first


class PointCloudPlan:
    """The counting half of the point cloud of one BitVolume: tile offsets on the device and, after ONE host read, the
    number of set voxels.  rows(a, b) then writes any window of the run, so a cloud larger than device memory can be
    fetched piece by piece.  z_mm: point_cloud_z_table of the volume's slices."""

    def __init__(self, vol: BitVolume, z_mm, mm_per_pixel_y, mm_per_pixel_x, k=1, rank_base=0):
        nz, ny, nx = vol.shape
        L = _lib.lib()
        self.k, self.rank_base = int(k), int(rank_base)
        if self.k < 1 or self.rank_base < 0:
            raise ValueError("k must be >= 1 and rank_base >= 0")
        z_mm = np.ascontiguousarray(z_mm, dtype=np.float64)
        if z_mm.shape != (nz,):
            raise ValueError("z_mm must hold one float64 per slice")
        self.vol, self.bits = vol, vol.bits.contiguous()
        self.z_mm = torch.from_numpy(z_mm).to(vol.device)
        self.mm_y, self.mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
        blocks = int(L.tomo_point_cloud_blocks(nz, ny, nx))
        self.blk_off = torch.empty(blocks + 1, dtype=torch.int64, device=vol.device)
        _lib.check(L.tomo_point_cloud_count(_p(self.bits), nz, ny, nx, self.rank_base, _p(self.blk_off), _stream()),
                   "tomo_point_cloud_count")
        self.n = int(self.blk_off[-1].item()) - self.rank_base           # the one host read: it sizes the output
        self.row_first, self.n_rows = point_cloud_rows(self.n, self.k, self.rank_base)

    def rows(self, a=0, b=None, out=None) -> torch.Tensor:
        """Rows [a, b) of this run (clipped to it) -> (b - a, 3) float64 device tensor."""
        a = max(0, int(a))
        b = self.n_rows if b is None else min(self.n_rows, int(b))
        cap = max(0, b - a)
        if out is None:
            out = torch.empty((cap, 3), dtype=torch.float64, device=self.vol.device)
        elif tuple(out.shape) != (cap, 3) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 (rows, 3) tensor")
        if cap:
            nz, ny, nx = self.vol.shape
            _lib.check(_lib.lib().tomo_point_cloud_rows(_p(self.bits), nz, ny, nx, _p(self.blk_off), self.k, _p(self.z_mm),
                                                        self.mm_y, self.mm_x, self.row_first + a, cap, _p(out), _stream()),
                       "tomo_point_cloud_rows")
        return out


def point_cloud(vol: BitVolume, slice_depths, mm_per_pixel_x, mm_per_pixel_y, subsample_factor=1, rank_base=0, z0=0,
                window=None) -> torch.Tensor:
    """generate_point_cloud (voxel_processor.py:99-127) of a resident volume -> (rows, 3) float64 device tensor, byte for byte
    the reference's rows (z_mm, y * mm_per_pixel_y, x * mm_per_pixel_x).  rank_base / z0: the set voxels and the slices in
    front of this volume when it is one Z-slab of a stack -- the result is then this slab's run of the stack's array.
    window = (a, b): rows [a, b) of the run only."""
    nz = vol.shape[0]
    plan = PointCloudPlan(vol, point_cloud_z_table(slice_depths, nz, z0), mm_per_pixel_y, mm_per_pixel_x,
                          point_cloud_step(subsample_factor), rank_base)
    return plan.rows() if window is None else plan.rows(window[0], window[1])


# ----------------------------------------------------------------------------- connected components
CONNECTIVITIES = (6, 26)     # generate_binary_structure(3, 1) -- the cross of voxel_processor.py:88,91 -- and (3, 3)
RUN_LIMIT = 2 ** 31          # run ids are 32-bit in csrc/components.hip
TABLE_COLUMNS = 10           # voxels, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x (tomo_cc_measure)
# bytes component_properties / component_moments / component_surface may take for the per-slice entries of the selected components
# (8 bytes an entry for the voxel counts, 48 for the six moment sums, 88 for the surface counters, 144 for the section counters
# of the mean breadth); one component (at most nz
# entries) is always granted
COMPONENT_HIST_BUDGET = 1 << 30
MOMENT_SUMS = 6              # uint64 per component and slice: N, sum j', sum i', sum j'^2, sum i'^2, sum j' i' (tomo_cc_moment_hist)
MOMENT_COLUMNS = 22          # float64 per row of tomo_cc_moments: W, centre (3), covariance (6), variances (3), axes (9)
TOPOLOGY_COLUMNS = 3         # euler, cavities, handles (tomo_cc_cavities)
SURFACE_COUNTERS = 11        # uint64 per component and slice: x, y, xy, then z, xz, yz, xyz upwards and downwards (tomo_cc_surface_hist)
SURFACE_CLASSES = 7          # direction classes: x, y, xy, z, xz, yz, xyz
BREADTH_WORDS = 18           # uint64 per component and slice: six raw in-slice counts, twelve signed cross parts (tomo_cc_breadth_hist)
BREADTH_FAMILIES = 13        # families of lattice planes: the columns of section_euler (breadth_normals)
BREADTH_COLUMNS = 26         # float64 per slice of breadth_factors: the families in the slice, then towards slice k + 1
PROFILE_COLUMNS = 7          # label, voxels, min bits, max bits, sum_q, min index, max index (tomo_profile_rows)
PROFILE_ADMITTED = 0x49800000    # float32 bit patterns below it are admitted by tomo_profile_stats: 0.0 <= v < 2^20
PROFILE_F_VALUE = 8          # bit of the flag word: tomo_profile_stats met a set voxel whose value is not admitted
_PROFILE_VALUE_ERROR = "values: a set voxel holds an entry outside 0.0 <= v < 2^20 (NaN, negative, -0.0 or infinite)"


def _check_connectivity(connectivity) -> int:
    if connectivity not in CONNECTIVITIES:
        raise ValueError("connectivity must be 6 or 26")
    return int(connectivity)


NO_MAX_VOXELS = 2 ** 63 - 1  # max_voxels=None as the kernels take it


def _keep_rule(min_voxels=0, largest=False, max_voxels=None, enclosed=False) -> tuple:
    """The normalised keep rule (min_voxels, largest, max_voxels, enclosed): what ComponentRuns.select compares and runs.
    A negative min_voxels is 0; max_voxels=None is no upper bound, a negative one a ValueError; largest goes with neither
    max_voxels nor enclosed (ValueError: the largest cavity is an argmax over the returned table)."""
    rule = (max(0, int(min_voxels)), bool(largest), None if max_voxels is None else int(max_voxels), bool(enclosed))
    if rule[2] is not None and rule[2] < 0:
        raise ValueError("max_voxels must be non-negative or None")
    if rule[1] and (rule[2] is not None or rule[3]):
        raise ValueError("largest cannot be combined with max_voxels or enclosed")
    return rule


def _whole_size(v, name) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a non-negative whole number" % name)
    if not (math.isfinite(v) and v >= 0 and int(v) == v):
        raise ValueError("%s must be a non-negative whole number" % name)
    return int(v)


def _check_size_window(min_voxels, max_voxels):
    """The size window of the cavity calls -> (min_voxels, max_voxels) as ints (max_voxels=None stays None); a size that is
    negative or no whole number is a ValueError.  min_voxels > max_voxels selects nothing and is no error."""
    return _whole_size(min_voxels, "min_voxels"), None if max_voxels is None else _whole_size(max_voxels, "max_voxels")


@dataclass(frozen=True)
class _Measurement:
    """What tells one per-component measurement from the next in ComponentRuns._rows: a histogram per slice of every selected
    component's box, then one thread per component.  A measurement without a histogram (topology) fills in name and results."""
    name: str                    # the public function, in the error texts
    results: tuple               # (dtype, trailing shape) per result tensor of m rows, in the order the finishing entry point takes them
    columns: object = None       # the columns of the measurement table that ride along in the download, in front of the labels
    words: int = 0               # uint64 per histogram entry
    what: str = ""               # those entries in the words of the budget error
    hist: str = ""               # the histogram entry point ...
    counter: str = ""            # ... and its COUNTERS key
    finish: str = ""             # the finishing entry point
    tables: int = 1              # the host table is that many tables of equal length, handed over one pointer each

    def empty(self):
        """The download of no selected component: zero-row host arrays of the declared dtypes and shapes, in its order."""
        ride = [] if self.columns is None else [np.zeros((0, TABLE_COLUMNS), dtype=np.int64)[:, self.columns], np.zeros(0, dtype=np.int64)]
        return ride + [torch.zeros((0, *shape), dtype=dtype).numpy() for dtype, shape in self.results]


_PROPERTIES = _Measurement("component_properties", ((torch.float64, (2,)),), slice(None), 1, "voxels-per-slice counters",
                           "tomo_cc_zhist", "components_zhist", "tomo_cc_zsums", 2)
_MOMENTS = _Measurement("component_moments", ((torch.float64, (MOMENT_COLUMNS,)),), 0, MOMENT_SUMS, "moment sums per slice",
                        "tomo_cc_moment_hist", "components_moments", "tomo_cc_moments", 2)
_SURFACE = _Measurement("component_surface", ((torch.float64, ()), (torch.int64, (SURFACE_CLASSES,))), 0, SURFACE_COUNTERS,
                        "surface counters per slice", "tomo_cc_surface_hist", "components_surface", "tomo_cc_surface")
_BREADTH = _Measurement("component_breadth", ((torch.float64, ()), (torch.int64, (BREADTH_FAMILIES,))), 0, BREADTH_WORDS,
                        "section counters per slice", "tomo_cc_breadth_hist", "components_breadth", "tomo_cc_breadth")
_TOPOLOGY = _Measurement("component_topology", ((torch.int64, (2 + TOPOLOGY_COLUMNS,)),))
_BRANCHES = _Measurement("skeleton_branches", ((torch.float64, ()), (torch.int64, (SURFACE_CLASSES,))), 0, SURFACE_COUNTERS,
                         "step counters per slice", "tomo_branch_hist", "skeleton_branches_hist", "tomo_cc_surface")


@dataclass
class ComponentSelection:
    """ComponentRuns.select's answer: device tensors over the n components, and the two counts read from the device.  The
    ComponentRuns that made it owns it: its counter block holds total and m for the finishing kernels, so it is good until
    that object selects under another rule -- and the measuring methods take the rule, never one of these."""
    table: torch.Tensor          # int64 (n, 10): the measurement table the rule was applied to (ComponentRuns.table)
    sel: torch.Tensor            # uint8 (n,): 1 where the component is selected
    off: torch.Tensor            # int64 (n + 1,): where the per-slice entries of a component start, one per slice of its box
    slot: torch.Tensor           # int32 (n,): the row of a selected component in the results = its rank among the selected
    total: int                   # per-slice entries of all selected components
    m: int                       # selected components


class ComponentRuns:
    """The run tables of one BitVolume under one connectivity: scipy.ndimage.label's components, held per X-RUN (a maximal
    run of set bits in a row) and never per voxel.  Two host reads: the number of runs (it sizes the tables) and the
    counters after the labelling.  n = components; labels() / sizes() / keep() read the tables.
    One object serves every per-component measurement of its volume: properties(), moments(), topology_rows(), surface(),
    thickness(), caliper(), geodesic(), skeleton() and branch_rows() share the labelling, the measurement table and ONE selection,
    which the object owns (select); label_at() answers which component a voxel lies in, clear() removes flagged components from
    a volume.  background() is the same
    kind of object for the complement: its enclosed components are the cavities of this volume (cavity_owners)."""

    def __init__(self, vol: BitVolume, connectivity=6):
        connectivity = _check_connectivity(connectivity)
        nz, ny, nx = vol.shape
        L, dev, st = _lib.lib(), vol.device, _stream()
        self.vol, self.bits, self.connectivity = vol, vol.bits.contiguous(), connectivity
        nrows = nz * ny
        self.tot = torch.empty(8, dtype=torch.int64, device=dev)
        self.row_off = torch.empty(nrows + 1, dtype=torch.int32, device=dev)
        blk = torch.empty(L.tomo_cc_scan_blocks(nrows + 1), dtype=torch.int64, device=dev)
        geo = (_p(self.bits), nz, ny, nx)
        _lib.check(L.tomo_cc_count_runs(*geo, _p(self.row_off), _p(blk), _p(self.tot), st), "tomo_cc_count_runs")
        self.runs = _download(self.tot)[0]                       # the one read that sizes the tables
        self.n = 0
        self._table = None
        self._topology = None
        self._background = self._owners = None
        self._rule = self._picked = None
        COUNTERS["components_label"] += 1
        if self.runs == 0:
            return
        if self.runs >= RUN_LIMIT:
            raise _lib.TomoError("too many runs for 32-bit run ids")
        cap = self.runs
        self.parent = torch.empty(cap, dtype=torch.int32, device=dev)
        self.rank = torch.empty(cap, dtype=torch.int32, device=dev)
        self._sizes = torch.empty(cap, dtype=torch.int64, device=dev)
        blk = torch.empty(L.tomo_cc_scan_blocks(cap), dtype=torch.int64, device=dev)
        _lib.check(L.tomo_cc_label_runs(*geo, self.connectivity, _p(self.row_off), cap, _p(self.parent), _p(self.rank), _p(self._sizes),
                                        _p(blk), _p(self.tot), st), "tomo_cc_label_runs")

    def _tables(self):
        return _p(self.row_off), self.runs, _p(self.parent), _p(self.rank)

    def _checked(self):
        """The counters after the work enqueued so far -> n; raises when a guard of the kernels fired."""
        host = self.host = _download(self.tot)
        if host[2] or host[0] != self.runs:
            raise _lib.TomoError("component labelling: the run tables do not fit the volume (flags %d)" % host[2])
        self.n = host[1]
        return self.n

    def sizes(self) -> torch.Tensor:
        """Voxels of component 1..n -> int64 (n,) device tensor (a view of the table)."""
        if self.runs == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.vol.device)
        return self._sizes[:self._checked()]

    def _measure(self) -> torch.Tensor:
        """The measurement table, enqueued once per object; its guards are read with the next _checked()."""
        if self._table is None:
            dev = self.vol.device
            n = self._checked() if self.runs else 0
            if n == 0:
                self._table = torch.zeros((0, TABLE_COLUMNS), dtype=torch.int64, device=dev)
            else:
                nz, ny, nx = self.vol.shape
                table = torch.empty((n, TABLE_COLUMNS), dtype=torch.int64, device=dev)
                COUNTERS["components_measure"] += 1
                _lib.check(_lib.lib().tomo_cc_measure(_p(self.bits), nz, ny, nx, *self._tables(), _p(self.tot), _p(table), n,
                                                      _stream()), "tomo_cc_measure")
                self._table = table
        return self._table

    def table(self) -> torch.Tensor:
        """Per component 1..n: voxels, zmin, zmax, ymin, ymax, xmin, xmax (inclusive indices), sum of z, of y, of x over its
        voxels -> int64 (n, 10) device tensor, computed once and kept.  Column 0 is sizes()."""
        fresh = self._table is None
        table = self._measure()
        if fresh and table.shape[0]:
            self._checked()
        return table

    def select(self, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False):
        """The keep rule of keep() on the measurement table: the components of at least min_voxels voxels -- largest: only the
        largest of those, the lowest label among equals -- in ascending label -> ComponentSelection, or None when there is no
        component or none is selected.  max_voxels: at most that many voxels as well; enclosed: only the components whose index
        box touches no face of the stack -- on the ComponentRuns of a complement (background()) those are the cavities.  Neither
        goes with largest (ValueError, before anything is launched).  One host read: the counters, with the guards of everything
        enqueued so far.
        The object keeps ONE selection: the kernel leaves its entry total and row count in the counter block, where every
        finishing kernel reads them, so the answer (None too) is kept for as long as the normalised rule stays the one last
        run, and replaced -- every ComponentSelection handed out before is then void -- when another rule is asked for."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        if rule == self._rule:
            return self._picked
        table = self._measure()
        n = table.shape[0]
        picked = None
        if n:
            L, dev = _lib.lib(), self.vol.device
            sel = torch.empty(n, dtype=torch.uint8, device=dev)
            off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            slot = torch.empty(n, dtype=torch.int32, device=dev)
            blk = torch.empty(2 * L.tomo_cc_scan_blocks(n), dtype=torch.int64, device=dev)
            self._rule = None                                           # the counter block is about to change hands
            _lib.check(L.tomo_cc_select(_p(table), n, _p(self.tot), rule[0], NO_MAX_VOXELS if rule[2] is None else rule[2], int(rule[1]),
                                        int(rule[3]), *self.vol.shape, _p(sel), _p(off), _p(slot), _p(blk), _stream()), "tomo_cc_select")
            self._checked()                                             # ... and the guards of the measuring pass
            total, m = self.host[4], self.host[5]
            picked = ComponentSelection(table, sel, off, slot, total, m) if m else None
        self._rule, self._picked = rule, picked
        return picked

    def hist_head(self, picked: ComponentSelection):
        """The leading arguments of every histogram entry point (tomo_cc_zhist, tomo_cc_moment_hist, tomo_cc_surface_hist): bits,
        geometry, run tables, tot, table, n, sel, off; the histogram and its capacity follow."""
        return (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(picked.table), picked.table.shape[0],
                _p(picked.sel), _p(picked.off))

    def finish_head(self, picked: ComponentSelection):
        """The leading arguments of every finishing entry point (tomo_cc_zsums, tomo_cc_moments, tomo_cc_surface): table, n, tot,
        sel, off, slot; the histogram and its capacity follow."""
        return _p(picked.table), picked.table.shape[0], _p(self.tot), _p(picked.sel), _p(picked.off), _p(picked.slot)

    def _download_checked(self, name, *tensors):
        """The tensors on the host, downloaded together with the flag word; raises when a guard of the kernels fired."""
        *host, flags = [t.cpu().numpy() for t in (*tensors, self.tot[2:3])]
        if flags[0]:
            raise _lib.TomoError("%s: the tables do not fit the volume (flags %d)" % (name, flags[0]))
        return host

    @staticmethod
    def _hist_budget(spec: _Measurement, picked: ComponentSelection):
        """TomoError where the histogram of the selection takes more than COMPONENT_HIST_BUDGET bytes; nothing is allocated here."""
        nbytes = 8 * spec.words * picked.total
        if nbytes > COMPONENT_HIST_BUDGET and picked.m > 1:         # read when called; one component is always granted
            raise _lib.TomoError("%s: %d components selected, their %s take %d bytes, more than COMPONENT_HIST_BUDGET (%d): raise "
                                 "min_voxels" % (spec.name, picked.m, spec.what, nbytes, COMPONENT_HIST_BUDGET))

    def _rows(self, spec: _Measurement, rule, host_table, *scalars, hist_args=()):
        """One measurement of the components the rule (_keep_rule's tuple) selects: spec.words uint64 per slice of every selected component's box
        from spec.hist, then spec.finish with one thread per component -> the host arrays (table columns, labels, *results),
        spec.empty() when nothing is selected.  host_table: the float64 table(s) the finishing kernel reads, uploaded here;
        scalars: its arguments between nz and the result tensors; hist_args: what spec.hist takes behind the histogram's capacity."""
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])
        if picked is None or picked.total == 0:
            return spec.empty()
        self._hist_budget(spec, picked)
        total, m = picked.total, picked.m
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        hist = torch.empty(spec.words * total, dtype=torch.int64, device=dev)
        COUNTERS[spec.counter] += 1
        _lib.check(getattr(L, spec.hist)(*self.hist_head(picked), _p(hist), total, *hist_args, st), spec.hist)
        tab = torch.from_numpy(host_table).to(dev).view(spec.tables, -1)
        results = []
        for dtype, shape in spec.results:
            results.append(torch.empty((m, *shape), dtype=dtype, device=dev))
        labels = torch.ones(m, dtype=torch.int64, device=dev)       # a valid row for the gather below even where a guard fired
        _lib.check(getattr(L, spec.finish)(*self.finish_head(picked), _p(hist), total, *map(_p, tab), self.vol.shape[0], *scalars,
                                           *map(_p, results), _p(labels), m, st), spec.finish)
        ride = picked.table[:, spec.columns].index_select(0, labels - 1)
        return self._download_checked(spec.name, ride, labels, *results)

    def properties(self, tables, mm_y, mm_x, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False) -> "ComponentProperties":
        """component_properties of this volume; tables: _slice_weights' (2 nz,).  The rule: select's."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        return _component_properties_from(*self._rows(_PROPERTIES, rule, tables), float(mm_y), float(mm_x))

    def moments(self, tables, mm_y, mm_x, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False) -> "ComponentMoments":
        """component_moments of this volume; tables: _slice_weights' (2 nz,).  The rule: select's."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        return _component_moments_from(*self._rows(_MOMENTS, rule, tables, float(mm_y), float(mm_x)))

    def surface(self, factors, directions, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False) -> "ComponentSurface":
        """component_surface of this volume; factors: surface_factors' (nz, 11) for the same directions.  The rule: select's."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        voxels, labels, area, counts = self._rows(_SURFACE, rule, factors, int(directions))
        return _component_surface_from(voxels, labels, counts, area)

    def breadth(self, factors, directions, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False) -> "ComponentBreadth":
        """component_breadth of this volume; factors: breadth_factors' (nz, 26) for the same directions.  The rule: select's."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        voxels, labels, breadth, euler = self._rows(_BREADTH, rule, factors, int(directions))
        return _component_breadth_from(voxels, labels, euler, breadth)

    def topology_rows(self, min_voxels=0, largest=False, *, max_voxels=None, enclosed=False) -> "ComponentTopology":
        """component_topology of this volume: the rows of topology() the rule (select's) selects."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        topo = self.topology()
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3]) if topo.shape[0] else None
        if picked is None:
            return _component_topology_from(*_TOPOLOGY.empty())
        rows = torch.empty((picked.m, *_TOPOLOGY.results[0][1]), dtype=torch.int64, device=self.vol.device)
        _lib.check(_lib.lib().tomo_cc_topology_rows(_p(picked.table), _p(topo), topo.shape[0], _p(self.tot), _p(picked.sel), _p(picked.slot),
                                                    _p(rows), picked.m, _stream()), "tomo_cc_topology_rows")
        return _component_topology_from(*self._download_checked(_TOPOLOGY.name, rows))

    def value_max(self, values: torch.Tensor, min_voxels=0) -> np.ndarray:
        """The largest entry of a float32 map per component of at least min_voxels voxels and the first voxel that attains it ->
        host int64 (m, 4): label, voxels, the float32 bit pattern, the flat index: the value passes of thickness() on a map of
        the caller's (thickness() keeps its own lines: its transform sits between the selection and the passes).  The entries
        are value_profile's: one that is not admitted on a set voxel is a ValueError."""
        values = _profile_values(self.vol, values)
        picked = self.select(min_voxels)
        if picked is None:
            return np.zeros((0, 4), dtype=np.int64)
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        n = picked.table.shape[0]
        best = torch.empty(n, dtype=torch.int32, device=dev)
        first = torch.empty(n, dtype=torch.int64, device=dev)
        rows = torch.empty((picked.m, 4), dtype=torch.int64, device=dev)
        head = (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(values.contiguous()), None)
        COUNTERS["components_value"] += 1
        _lib.check(L.tomo_cc_value_max(*head, _p(best), n, st), "tomo_cc_value_max")
        _lib.check(L.tomo_cc_value_first(*head, _p(best), _p(first), n, st), "tomo_cc_value_first")
        _lib.check(L.tomo_cc_value_rows(_p(picked.table), _p(best), _p(first), n, _p(self.tot), _p(picked.sel), _p(picked.slot),
                                        _p(rows), picked.m, st), "tomo_cc_value_rows")
        (rows,) = self._download_checked("value_max", rows)
        if (rows[:, 2] >= PROFILE_ADMITTED).any():          # every pattern that is not admitted lies above the admitted ones
            raise ValueError(_PROFILE_VALUE_ERROR)
        return rows

    def value_profile(self, values: torch.Tensor, min_voxels=0) -> np.ndarray:
        """What a float32 map of the volume's shape gives per component of at least min_voxels voxels, in ascending label -> host
        int64 (m, 7): label, voxels, the float32 bit patterns of the smallest and the largest entry, sum_q, and the lowest flat
        index (z * ny + y) * nx + x that attains the smallest and the largest (include/tomo_hip.h, tomo_profile_*; _profile_rows_from
        turns the rows into floats).  sum_q is the int64 sum of rint(float64(v) * 65536): the same bytes on every run.  Entries
        of unset voxels are never read; a set voxel with an entry outside 0.0 <= v < 2^20 (NaN, negative, -0.0, infinite) is a
        ValueError.  Rows are under the object's ONE selection, so they line up with every other measurement of the same rule."""
        values = _profile_values(self.vol, values)
        picked = self.select(min_voxels)
        if picked is None:
            return np.zeros((0, PROFILE_COLUMNS), dtype=np.int64)
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        n = picked.table.shape[0]
        values = values.contiguous()
        lo, hi = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        total = torch.empty(n, dtype=torch.int64, device=dev)
        lo_first, hi_first = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        rows = torch.empty((picked.m, PROFILE_COLUMNS), dtype=torch.int64, device=dev)
        head = (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(values))
        COUNTERS["components_profile"] += 1
        _lib.check(L.tomo_profile_stats(*head, _p(lo), _p(hi), _p(total), n, st), "tomo_profile_stats")
        _lib.check(L.tomo_profile_where(*head, _p(lo), _p(hi), _p(lo_first), _p(hi_first), n, st), "tomo_profile_where")
        _lib.check(L.tomo_profile_rows(_p(picked.table), _p(lo), _p(hi), _p(total), _p(lo_first), _p(hi_first), n, _p(self.tot),
                                       _p(picked.sel), _p(picked.slot), _p(rows), picked.m, st), "tomo_profile_rows")
        host, flags = rows.cpu().numpy(), int(self.tot[2:3].cpu().numpy()[0])
        if flags & PROFILE_F_VALUE:                         # the one flag that speaks of the caller's map, not of the tables
            self.tot[2:3].bitwise_and_(~PROFILE_F_VALUE)    # the object stays usable
            flags &= ~PROFILE_F_VALUE
            if not flags:
                raise ValueError(_PROFILE_VALUE_ERROR)
        if flags:
            raise _lib.TomoError("value_profile: the tables do not fit the volume (flags %d)" % flags)
        return host

    def thickness(self, slice_depths, mm_y, mm_x, radii_mm=None, min_voxels=0, largest=False, *, max_voxels=None,
                  enclosed=False) -> "ComponentThickness":
        """component_thickness of this volume.  The rule: select's.  ONE transform of the whole volume (distance and local
        thickness are local to a component), then reductions over the run tables: the value passes for the inscribed sphere
        and, with radii_mm, the level histogram behind the driver of the other measurements.  On background() with
        enclosed=True the rows are the cavities: their pore sizes."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        radii, weights = _component_thickness_args(self.vol.shape, slice_depths, mm_y, mm_x, radii_mm)
        COUNTERS["component_thickness"] += 1
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])
        if picked is None:
            return _component_thickness_from(self.vol.shape, slice_depths, mm_y, mm_x, np.zeros((0, 4), dtype=np.int64), radii)
        spec = None if radii is None else _thickness_measurement(len(radii))
        if spec is not None:
            self._hist_budget(spec, picked)                             # before the transform allocates anything
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        plan = _DistancePlan(BitVolume(self.bits, self.vol.shape), slice_depths, mm_y, mm_x)
        n = picked.table.shape[0]
        dist = d2 = None
        if radii is None:                                               # 4 B per voxel, no d2
            dist = torch.empty(self.vol.shape, dtype=torch.float32, device=dev)
            _lib.check(L.tomo_edt_distance(*plan.head(), 1, _p(dist), *plan.tail()), "tomo_edt_distance")
        else:                                                           # one float64 transform serves both parts
            d2 = torch.empty(self.vol.shape, dtype=torch.float64, device=dev)
            _lib.check(L.tomo_edt_squared(*plan.head(), 1, _p(d2), *plan.tail()), "tomo_edt_squared")
        best = torch.empty(n, dtype=torch.int32, device=dev)
        first = torch.empty(n, dtype=torch.int64, device=dev)
        rows = torch.empty((picked.m, 4), dtype=torch.int64, device=dev)
        head = (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(dist), _p(d2))
        COUNTERS["components_value"] += 1
        _lib.check(L.tomo_cc_value_max(*head, _p(best), n, st), "tomo_cc_value_max")
        _lib.check(L.tomo_cc_value_first(*head, _p(best), _p(first), n, st), "tomo_cc_value_first")
        _lib.check(L.tomo_cc_value_rows(_p(picked.table), _p(best), _p(first), n, _p(self.tot), _p(picked.sel), _p(picked.slot),
                                        _p(rows), picked.m, st), "tomo_cc_value_rows")
        levels = None
        if spec is not None:
            r2 = radii * radii
            live = int(np.searchsorted(r2, float(d2.max().item()), side="right"))
            level_map = torch.zeros(self.vol.shape, dtype=torch.int32, device=dev)
            eroded = torch.empty_like(plan.bits) if live else None
            _thickness_levels(plan, d2, r2, live, level_map, eroded)
            del d2
            levels = self._rows(spec, rule, weights, len(radii), hist_args=(_p(level_map), len(radii)))
        (host,) = self._download_checked("component_thickness", rows)
        return _component_thickness_from(self.vol.shape, slice_depths, mm_y, mm_x, host, radii, levels)

    def caliper(self, slice_depths, mm_y, mm_x, directions=None, extent="voxels", oriented=False, min_voxels=0, largest=False, *,
                max_voxels=None, enclosed=False) -> "ComponentCaliper":
        """component_caliper of this volume.  The rule: select's.  One row pass per batch of directions over the run tables, the
        two ends of every run; with oriented, moments() runs first under the same rule -- the one selection, so the rows line
        up -- and one more pass measures every component along its own principal axes.  On background() with enclosed=True
        the rows are the cavities."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        dirs, tabs = _caliper_args(self.vol.shape, slice_depths, mm_y, mm_x, directions, extent)
        COUNTERS["component_caliper"] += 1
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])
        if picked is None:
            return _component_caliper_from(dirs, oriented=bool(oriented))
        M, m = len(dirs), picked.m
        nbytes = 16 * M * m
        if nbytes > COMPONENT_HIST_BUDGET and m > 1:                    # read when called; one component is always granted
            raise _lib.TomoError("component_caliper: %d components selected, their extremes along %d directions take %d bytes, more "
                                 "than COMPONENT_HIST_BUDGET (%d): raise min_voxels" % (m, M, nbytes, COMPONENT_HIST_BUDGET))
        q = None
        if oriented:                                                    # the same rule: the selection stays, the rows line up
            q = self.moments(_slice_weights(slice_depths, self.vol.shape[0], mm_y, mm_x), mm_y, mm_x, rule[0], rule[1], max_voxels=rule[2],
                             enclosed=rule[3])
            if len(q) != m:
                raise _lib.TomoError("component_caliper: the rows of the moments are not the rows of the selection")
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        n = picked.table.shape[0]
        head = (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(picked.sel), _p(picked.slot), n)

        def rows_of(count, launch):
            """hi / lo keys of `count` directions filled by launch(hi, lo), then decoded -> device (rows, hi, lo, width, ext)"""
            hi = torch.empty((m, count), dtype=torch.float64, device=dev)
            lo = torch.empty((m, count), dtype=torch.float64, device=dev)
            width = torch.empty((m, count), dtype=torch.float64, device=dev)
            rows = torch.empty((m, 4), dtype=torch.int64, device=dev)
            ext = torch.empty((m, 2), dtype=torch.float64, device=dev)
            launch(hi, lo)
            _lib.check(L.tomo_cc_caliper_rows(_p(picked.table), n, _p(self.tot), _p(picked.sel), _p(picked.slot), _p(hi), _p(lo), count,
                                              _p(width), _p(rows), _p(ext), m, st), "tomo_cc_caliper_rows")
            return rows, hi, lo, width, ext

        shared = torch.from_numpy(np.concatenate([t.reshape(-1) for t in (tabs.pz, tabs.py, tabs.px, tabs.h) if t is not None])).to(dev)
        nz, ny, nx = self.vol.shape
        ptr = [shared.data_ptr() + 8 * M * o for o in (0, nz, nz + ny, nz + ny + nx)]
        out = rows_of(M, lambda hi, lo: _lib.check(L.tomo_cc_caliper(*head, ptr[0], ptr[1], ptr[2], None if tabs.h is None else ptr[3], M,
                                                                    _p(hi), _p(lo), m, st), "tomo_cc_caliper"))
        own = None
        if oriented:
            axes = torch.from_numpy(np.ascontiguousarray(q.principal_axes).reshape(-1)).to(dev)
            pos = torch.from_numpy(np.concatenate([tabs.zc, tabs.yt, tabs.xt, tabs.depth])).to(dev)
            at = [pos.data_ptr() + 8 * o for o in (0, nz, nz + ny, nz + ny + nx)]
            own = rows_of(3, lambda hi, lo: _lib.check(L.tomo_cc_caliper_axes(*head, _p(axes), at[0], at[1], at[2],
                                                                              at[3] if tabs.h is not None else None, float(mm_y), float(mm_x),
                                                                              _p(hi), _p(lo), m, st), "tomo_cc_caliper_axes"))
        host = self._download_checked("component_caliper", *out, *(own or ()))
        if oriented and not np.array_equal(host[5][:, 0], q.labels):
            raise _lib.TomoError("component_caliper: the rows of the moments are not the rows of the selection")
        return _component_caliper_from(dirs, host[:5], q, host[5:] if oriented else None, oriented=bool(oriented))

    def geodesic(self, slice_depths, mm_y, mm_x, sweeps=3, min_voxels=0, largest=False, *, max_voxels=None,
                 enclosed=False) -> "ComponentGeodesic":
        """component_geodesic of this volume.  The rule: select's.  The repeated farthest-point search for all selected
        components at once (propagation stays inside a component): a0 = the first voxel of the component in raster order -- the
        value kernels on an all-zero map -- then `sweeps` times: propagate from a(s - 1) inside the selected components (the
        others keep +inf, their tiles are never dirty), and tomo_cc_value_max / tomo_cc_value_first on the map give a_s, the
        farthest voxel, the lowest flat index among equals.  The steps use the connectivity of this object.  The map of the last
        search stays in last_geodesic_map.  On background() with enclosed=True the rows are the cavities."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        sweeps = _geodesic_search_sweeps(sweeps)
        tables = _geodesic_tables(self.vol.shape, slice_depths, mm_y, mm_x)
        COUNTERS["component_geodesic"] += 1
        self.last_geodesic_map = None
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])
        if picked is None:
            return _component_geodesic_from(tables, np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4), dtype=np.int64))
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        plan = _GeodesicPlan(BitVolume(self.bits, self.vol.shape), tables, self.connectivity)
        n = picked.table.shape[0]
        dist = torch.zeros(self.vol.shape, dtype=torch.float32, device=dev)
        best = torch.empty(n, dtype=torch.int32, device=dev)
        first = torch.empty(n, dtype=torch.int64, device=dev)
        head = (_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(dist), None)

        def farthest():
            COUNTERS["components_value"] += 1
            _lib.check(L.tomo_cc_value_max(*head, _p(best), n, st), "tomo_cc_value_max")
            _lib.check(L.tomo_cc_value_first(*head, _p(best), _p(first), n, st), "tomo_cc_value_first")

        farthest()                                                      # on the all-zero map: the first voxel of every component
        prev = None
        for _ in range(sweeps):
            prev = first.clone()
            dist.fill_(float("inf"))
            _lib.check(L.tomo_geo_seed_index(_p(self.bits), *self.vol.shape, _p(prev), _p(picked.sel), n, _p(dist), *plan.seed_tail(), st),
                       "tomo_geo_seed_index")
            plan.propagate(dist)
            farthest()
        rows = torch.empty((picked.m, 4), dtype=torch.int64, device=dev)
        rows_prev = torch.empty((picked.m, 4), dtype=torch.int64, device=dev)
        for b, f, out in ((best, first, rows), (best, prev, rows_prev)):
            _lib.check(L.tomo_cc_value_rows(_p(picked.table), _p(b), _p(f), n, _p(self.tot), _p(picked.sel), _p(picked.slot), _p(out),
                                            picked.m, st), "tomo_cc_value_rows")
        host, host_prev, flags = self._download_checked("component_geodesic", rows, rows_prev, plan.counters[1:2])
        if flags[0]:
            raise _lib.TomoError("component_geodesic: a seed does not lie on its component (flags %d)" % flags[0])
        self.last_geodesic_map = dist
        return _component_geodesic_from(tables, host, host_prev)

    def skeleton(self, min_voxels=0, largest=False, curve=True, anchors=None, *, max_voxels=None, enclosed=False) -> "ComponentSkeleton":
        """component_skeleton of this volume.  The rule: select's.  ONE thinning of the whole volume under the connectivity of this
        object (thinning preserves components: every component owns exactly one piece of the skeleton), one tomo_thin_nodes over
        it, then tomo_thin_count adds up the skeleton, its ends and its junctions under the ORIGINAL runs of the selected
        components.  The skeleton stays in last_skeleton.  On background() with enclosed=True the rows are the cavities."""
        rule = _keep_rule(min_voxels, largest, max_voxels, enclosed)
        curve, anchors = _skeleton_args(self.vol, curve, self.connectivity, anchors)
        COUNTERS["component_skeleton"] += 1
        self.last_skeleton = None
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])
        if picked is None:
            return _component_skeleton_from(np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int64))
        L, dev, st = _lib.lib(), self.vol.device, _stream()
        skel, _ = _skeleton(BitVolume(self.bits, self.vol.shape), curve, self.connectivity, anchors)
        nodes = _skeleton_nodes(skel)
        n = picked.table.shape[0]
        counts = torch.zeros((picked.m, 3), dtype=torch.int64, device=dev)
        for column, other in enumerate((skel, nodes.ends, nodes.junctions)):
            _lib.check(L.tomo_thin_count(_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(other.bits), _p(picked.sel),
                                         _p(picked.slot), _p(counts), column, 3, n, picked.m, st), "tomo_thin_count")
        labels = picked.sel.nonzero().reshape(-1)
        ride = torch.stack((labels + 1, picked.table[:, 0].index_select(0, labels)), dim=1)
        host, rows = self._download_checked("component_skeleton", ride, counts)
        self.last_skeleton = skel
        return _component_skeleton_from(host, rows)

    def branch_rows(self, steps, whole: BitVolume, min_voxels=0):
        """skeleton_branches' rows for this volume as the regular voxels R of `whole` (S): per branch with at least min_voxels
        voxels, in ascending label -> host arrays (voxels, labels, length_mm, step_counts (m, 7), attach (m, 2), attach_count (m,)).
        steps: branch_steps' (nz, 11).  The step histogram goes through the driver of the other measurements
        (COMPONENT_HIST_BUDGET, its error); tomo_branch_attach runs over the same selection.  attach is (-1, -1) for a cycle."""
        rule = _keep_rule(min_voxels)
        voxels, labels, length, counts = self._rows(_BRANCHES, rule, steps, 13, hist_args=(_p(whole.bits),))
        m = len(labels)
        if m == 0:
            return voxels, labels, length, counts.reshape(0, SURFACE_CLASSES), np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
        picked = self.select(rule[0], rule[1], max_voxels=rule[2], enclosed=rule[3])    # the selection _rows just made
        dev = self.vol.device
        attach = torch.empty((m, 2), dtype=torch.int64, device=dev)
        count = torch.empty(m, dtype=torch.int64, device=dev)
        COUNTERS["branch_attach"] += 1
        _lib.check(_lib.lib().tomo_branch_attach(_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(whole.bits),
                                                 _p(picked.sel), _p(picked.slot), _p(attach), _p(count), picked.table.shape[0], m,
                                                 _stream()), "tomo_branch_attach")
        attach, count = self._download_checked("skeleton_branches", attach, count)
        attach[count == 0] = -1                                         # a cycle: the entry point's (all ones, 0)
        return voxels, labels, length, counts.reshape(m, SURFACE_CLASSES), attach, count

    def label_at(self, indices) -> torch.Tensor:
        """The label (1 .. n) of the voxels at the flat indices (z * ny + y) * nx + x -> int64 device tensor of the shape of
        `indices` (an int64 tensor on the volume's device, or anything np.asarray takes); 0 where the voxel is clear and where the
        index is negative or past the volume.  One launch; its guards are read with the next _checked()."""
        dev = self.vol.device
        if not isinstance(indices, torch.Tensor):
            indices = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int64))
        if indices.dtype != torch.int64:
            raise TypeError("indices must be int64")
        q = indices.to(dev).contiguous()
        out = torch.zeros_like(q)
        if q.numel() == 0 or self.runs == 0:
            return out
        n = self.n or self._checked()
        COUNTERS["branch_lookup"] += 1
        _lib.check(_lib.lib().tomo_branch_lookup(_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), n, _p(q), q.numel(),
                                                 _p(out), _stream()), "tomo_branch_lookup")
        return out

    def clear(self, flagged: torch.Tensor, src: BitVolume) -> BitVolume:
        """A NEW volume: `src` (any volume of this shape) without the runs of the components of THIS volume whose entry of
        flagged (uint8 (n,), on the device) is set."""
        n = self._checked() if self.runs else 0
        if tuple(src.shape) != tuple(self.vol.shape) or flagged.dtype != torch.uint8 or flagged.numel() != n:
            raise ValueError("clear: one uint8 flag per component and a volume of this shape")
        bits = src.bits.contiguous()
        if n == 0:
            return BitVolume(bits.clone(), src.shape)
        out = torch.empty_like(bits)
        COUNTERS["branch_clear"] += 1
        _lib.check(_lib.lib().tomo_branch_clear(_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), _p(flagged.contiguous()), n,
                                                _p(bits), _p(out), _stream()), "tomo_branch_clear")
        self._checked()
        return BitVolume(out, src.shape)

    def topology(self) -> torch.Tensor:
        """Per component 1..n: Euler number, cavities (enclosed voids, b2) and handles (tunnels, b1 = 1 - euler + cavities) of
        the mask `labels == c` -> int64 (n, 3) device tensor, computed once and kept.  The background has the complementary
        connectivity (26 for 6, 6 for 26) and everything outside the stack is background: a void that reaches a face of the
        stack is no cavity.  The Euler pass runs over the rows of this object; the cavities come from a second ComponentRuns
        over the complement: every component of it whose box touches no face is a cavity of the component left of its first
        voxel.  That object is kept (background()).  Working memory: one more bit volume and the run tables of the complement,
        never a label array."""
        if self._topology is None:
            dev = self.vol.device
            n = self._checked() if self.runs else 0
            if n == 0:
                self._topology = torch.zeros((0, TOPOLOGY_COLUMNS), dtype=torch.int64, device=dev)
                return self._topology
            nz, ny, nx = self.vol.shape
            L, st = _lib.lib(), _stream()
            geo = (_p(self.bits), nz, ny, nx)
            euler = torch.empty(n, dtype=torch.int64, device=dev)
            COUNTERS["components_euler"] += 1
            _lib.check(L.tomo_cc_euler(*geo, self.connectivity, *self._tables(), _p(self.tot), _p(euler), n, st), "tomo_cc_euler")
            outside = torch.empty_like(self.bits)
            _lib.check(L.tomo_cc_complement(*geo, _p(outside), st), "tomo_cc_complement")
            bg = ComponentRuns(BitVolume(outside, self.vol.shape), 32 - self.connectivity)
            bg_table = bg.table()
            topo = torch.empty((n, TOPOLOGY_COLUMNS), dtype=torch.int64, device=dev)
            bg_args = (_p(outside), _p(bg.row_off), bg.runs, _p(bg.parent), _p(bg.rank), _p(bg.tot), _p(bg_table),
                       bg_table.shape[0]) if bg.runs else (None, None, 0, None, None, None, None, 0)
            COUNTERS["components_cavities"] += 1
            _lib.check(L.tomo_cc_cavities(*geo, *self._tables(), _p(self.tot), n, *bg_args, _p(euler), _p(topo), st), "tomo_cc_cavities")
            self._checked()
            self._topology, self._background = topo, bg
        return self._topology

    def background(self) -> "ComponentRuns":
        """The complement of this volume inside the stack as a ComponentRuns under the complementary connectivity 32 - k: the
        object topology() builds (it runs first if it has not), labelled once and kept.  Its components in ascending label are
        the voids of the volume in the raster order of their first voxel; select(enclosed=True) on it picks the cavities, and
        properties / moments / surface measure them like any component."""
        if self._background is None:
            self.topology()
        if self._background is None:                                    # no component here: topology() had nothing to build
            self._background = _complement_runs(BitVolume(self.bits, self.vol.shape), self.connectivity)
        return self._background

    def cavity_owners(self) -> torch.Tensor:
        """Per component 1..n_bg of background(): the label of the component of this volume that owns it -- the one holding the
        voxel left of the cavity's first run in raster order -- or 0 for a void that reaches a face of the stack -> int64 (n_bg,)
        device tensor, computed once and kept.  An island floating in a void does not own that void."""
        if self._owners is None:
            bg = self.background()
            bg_table = bg.table()
            dev, n_bg = self.vol.device, bg_table.shape[0]
            n = self._checked() if self.runs else 0
            if n == 0 or n_bg == 0:
                self._owners = torch.zeros(n_bg, dtype=torch.int64, device=dev)
            else:
                owner = torch.empty(n_bg, dtype=torch.int64, device=dev)
                COUNTERS["components_cavity_owners"] += 1
                _lib.check(_lib.lib().tomo_cc_cavity_owners(_p(self.bits), *self.vol.shape, *self._tables(), _p(self.tot), n, _p(bg.bits),
                                                            _p(bg.row_off), bg.runs, _p(bg.parent), _p(bg.rank), _p(bg.tot), _p(bg_table),
                                                            n_bg, _p(owner), _stream()), "tomo_cc_cavity_owners")
                self._checked()
                self._owners = owner
        return self._owners

    def labels(self):
        """-> (int32 (nz, ny, nx) device tensor as scipy.ndimage.label returns it, n)."""
        nz, ny, nx = self.vol.shape
        COUNTERS["components_expand"] += 1
        if self.runs == 0:
            return torch.zeros((nz, ny, nx), dtype=torch.int32, device=self.vol.device), 0
        out = torch.empty((nz, ny, nx), dtype=torch.int32, device=self.vol.device)
        _lib.check(_lib.lib().tomo_cc_expand(_p(self.bits), nz, ny, nx, *self._tables(), _p(self.tot), _p(out), _stream()),
                   "tomo_cc_expand")
        return out, self._checked()

    def keep(self, min_voxels=0, largest=False) -> BitVolume:
        """A NEW volume with the components of at least min_voxels voxels; largest: only the largest of those."""
        nz, ny, nx = self.vol.shape
        min_voxels = max(0, int(min_voxels))
        COUNTERS["components_filter"] += 1
        if self.runs == 0:
            return BitVolume(torch.zeros_like(self.bits), self.vol.shape)
        out = torch.empty_like(self.bits)
        _lib.check(_lib.lib().tomo_cc_filter(_p(self.bits), nz, ny, nx, *self._tables(), _p(self._sizes), _p(self.tot), min_voxels,
                                             int(bool(largest)), _p(out), _stream()), "tomo_cc_filter")
        self._checked()
        return BitVolume(out, self.vol.shape)


def label_components(vol: BitVolume, connectivity=6):
    """scipy.ndimage.label(volume, generate_binary_structure(3, 1 if connectivity == 6 else 3)) of a resident volume ->
    (labels int32 (nz, ny, nx) device tensor, n): components numbered 1..n in the raster order of their first voxel."""
    return ComponentRuns(vol, connectivity).labels()


def component_sizes(vol: BitVolume, connectivity=6) -> torch.Tensor:
    """np.bincount(labels.ravel())[1:] without the label array -> int64 (n,) device tensor."""
    return ComponentRuns(vol, connectivity).sizes()


def keep_components(vol: BitVolume, min_voxels=0, largest=False, connectivity=6) -> BitVolume:
    """Island removal: a new BitVolume holding the components of `vol` with at least min_voxels voxels -- with largest=True
    only the single largest of those, the first in raster order among equals.  `vol` is left untouched; an empty volume
    comes back empty.  Working memory scales with the rows and the runs: no per-voxel label array is made."""
    return ComponentRuns(vol, connectivity).keep(min_voxels, largest)


def component_table(vol: BitVolume, connectivity=6) -> torch.Tensor:
    """scipy.ndimage.find_objects + the sums behind center_of_mass without the label array -> int64 (n, 10) device tensor,
    row c - 1 for label c: voxels, zmin, zmax, ymin, ymax, xmin, xmax (inclusive), sum of z, sum of y, sum of x."""
    return ComponentRuns(vol, connectivity).table()


def _slice_weights(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x) -> np.ndarray:
    """float64 (2 nz,): the weight (mm_x * mm_y) * depth[k] of a voxel of slice k, then the slice centres zc[k] of
    distance_positions.  slice_depths=None: depth 1.0 per slice."""
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)
    depth = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    return np.concatenate([(float(mm_per_pixel_x) * float(mm_per_pixel_y)) * depth, zt[1:-1]])


@dataclass
class ComponentProperties:
    """component_properties' answer: host arrays, one row per selected component in ascending label."""
    labels: np.ndarray           # int64 (m,)
    voxels: np.ndarray           # int64 (m,)
    index_box: np.ndarray        # int64 (m, 6): zmin, zmax, ymin, ymax, xmin, xmax, inclusive
    index_sums: np.ndarray       # int64 (m, 3): sum of z, y, x over the voxels
    volume_mm3: np.ndarray       # float64 (m,)
    centroid_index: np.ndarray   # float64 (m, 3): index_sums / voxels
    centroid_mm: np.ndarray      # float64 (m, 3): z, y, x in the coordinates of distance_positions

    def __len__(self):
        return len(self.labels)


def _component_properties_from(table, labels, sums, mm_per_pixel_y, mm_per_pixel_x) -> ComponentProperties:
    """Host arithmetic on the downloaded rows: table int64 (m, 10), sums float64 (m, 2) = (volume, sum of volume * z_mm)."""
    voxels, isums = table[:, 0], table[:, 7:10]
    cidx = isums / voxels[:, None]
    cmm = np.empty((len(labels), 3), dtype=np.float64)
    cmm[:, 0] = sums[:, 1] / sums[:, 0]
    cmm[:, 1] = cidx[:, 1] * mm_per_pixel_y
    cmm[:, 2] = cidx[:, 2] * mm_per_pixel_x
    return ComponentProperties(labels, voxels.copy(), table[:, 1:7].copy(), isums.copy(), sums[:, 0].copy(), cidx, cmm)


def component_properties(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                         min_voxels=0, largest=False) -> ComponentProperties:
    """Per component of a resident volume: voxels, index box, index sums, volume in mm^3 under the slice depths, centroid in
    indices and in millimetres -> ComponentProperties, one row per component with at least min_voxels voxels (largest: only
    the largest of those, the lowest label among equals -- keep_components' rule), in ascending label.
    volume_mm3 is the float VolumeCalculator.calculate_voxel_volume_variable_depth returns for the mask `labels == c`: count *
    ((mm_x * mm_y) * depth) added slice by slice in ascending z.  centroid_mm = (sum of slice volume * zc / volume, sum y /
    voxels * mm_y, sum x / voxels * mm_x) with zc the slice centres of distance_positions: the coordinates of
    distance_transform and inscribed_sphere.  slice_depths=None: depth 1.0 per slice.
    Four host reads (the run count, the counters after the labelling, the histogram's length, the results); working memory
    scales with the runs, the components and the voxels-per-slice counters of the SELECTED components (one per slice of a
    component's box; beyond COMPONENT_HIST_BUDGET bytes for more than one component: TomoError) -- never with the voxels."""
    tables = _slice_weights(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    return ComponentRuns(vol, connectivity).properties(tables, mm_per_pixel_y, mm_per_pixel_x, min_voxels, largest)


@dataclass
class ComponentMoments:
    """component_moments' answer: host arrays, one row per selected component in ascending label; vectors in (z, y, x) order."""
    labels: np.ndarray                    # int64 (m,)
    voxels: np.ndarray                    # int64 (m,)
    volume_mm3: np.ndarray                # float64 (m,): W, bit for bit component_properties' volume_mm3
    center_of_mass_mm: np.ndarray         # float64 (m, 3)
    covariance_mm2: np.ndarray            # float64 (m, 3, 3), symmetric
    principal_variances_mm2: np.ndarray   # float64 (m, 3), descending
    principal_axes: np.ndarray            # float64 (m, 3, 3): ROWS are the unit eigenvectors in that order
    ellipsoid_axes_mm: np.ndarray         # float64 (m, 3): 2 sqrt(5 variance)

    def __len__(self):
        return len(self.labels)


def _component_moments_from(voxels, labels, rows) -> ComponentMoments:
    """Host side of the downloaded rows: rows float64 (m, 22) as tomo_cc_moments writes them."""
    m = len(labels)
    cov = np.empty((m, 3, 3), dtype=np.float64)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        cov[:, a, b] = cov[:, b, a] = rows[:, 4 + k]
    lam = rows[:, 10:13].copy()
    return ComponentMoments(labels, voxels, rows[:, 0].copy(), rows[:, 1:4].copy(), cov, lam, rows[:, 13:22].reshape(m, 3, 3).copy(),
                            2.0 * np.sqrt(5.0 * lam))


def component_moments(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                      min_voxels=0, largest=False) -> ComponentMoments:
    """Second moments and principal axes per component of a resident volume -> ComponentMoments, one row per component the
    keep rule of component_properties selects (at least min_voxels voxels; largest: only the largest of those, the lowest
    label among equals), in ascending label.
    A set voxel (k, j, i) is a point mass at p = (zc[k], j * mm_per_pixel_y, i * mm_per_pixel_x) -- zc the slice centres of
    distance_positions, the coordinates of distance_transform and inscribed_sphere -- of weight w[k] = (mm_x * mm_y) *
    depth[k], its volume.  volume_mm3 = W = sum w, bit for bit component_properties' volume_mm3 (the same additions in
    ascending z).  center_of_mass_mm = sum w p / W: in z it is component_properties' centroid_mm[:, 0]; in y and x it equals
    centroid_mm only under uniform depths, because that centroid divides by the voxel count in the plane, whatever the
    slices weigh.  covariance_mm2 = sum w (p - centre)(p - centre)^T / W, symmetric.  Voxels are points: the d^2 / 12 of a
    voxel's own extent is NOT added, a plate one voxel thick has variance 0 across itself.  principal_variances_mm2: the
    eigenvalues, descending; principal_axes: the unit eigenvectors as rows in that order, the component of largest magnitude
    positive (the first such on a tie); one voxel, or any zero matrix, has zeros and the identity.  ellipsoid_axes_mm =
    2 sqrt(5 variance): the full axes of the solid ellipsoid with the same second moments.  slice_depths=None: depth 1.0.
    The same four host reads as component_properties; working memory scales with the runs, the components and six sums per
    slice of the box of every SELECTED component (48 bytes an entry; beyond COMPONENT_HIST_BUDGET bytes for more than one
    component: TomoError) -- never with the voxels."""
    tables = _slice_weights(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    return ComponentRuns(vol, connectivity).moments(tables, mm_per_pixel_y, mm_per_pixel_x, min_voxels, largest)


# ----------------------------------------------------------------------------- Euler number, cavities and handles
@dataclass
class ComponentTopology:
    """component_topology's answer: host arrays, one row per selected component in ascending label."""
    labels: np.ndarray           # int64 (m,)
    voxels: np.ndarray           # int64 (m,)
    euler: np.ndarray            # int64 (m,): Euler number of the mask `labels == c`
    cavities: np.ndarray         # int64 (m,): enclosed voids (b2)
    handles: np.ndarray          # int64 (m,): tunnels (b1) = 1 - euler + cavities

    def __len__(self):
        return len(self.labels)


def _component_topology_from(rows) -> ComponentTopology:
    """Host side of the downloaded rows: int64 (m, 5) as tomo_cc_topology_rows writes them."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 2 + TOPOLOGY_COLUMNS)
    return ComponentTopology(*(rows[:, k].copy() for k in range(2 + TOPOLOGY_COLUMNS)))


def euler_number(vol: BitVolume, connectivity=6) -> int:
    """The Euler number of a resident volume: under connectivity 26, vertices - edges + faces - cubes of the union of the
    closed unit cubes of the set voxels; under 6, voxels - face-adjacent pairs + full 2 x 2 blocks - full 2 x 2 x 2 blocks
    (the dual complex).  Everything outside the stack is background.  It equals components - handles + cavities
    (volume_topology) without any labelling: one pass over the rows, one host read."""
    connectivity = _check_connectivity(connectivity)
    nz, ny, nx = vol.shape
    chi = torch.empty(1, dtype=torch.int64, device=vol.device)
    COUNTERS["components_euler"] += 1
    _lib.check(_lib.lib().tomo_cc_euler(_p(vol.bits.contiguous()), nz, ny, nx, connectivity, None, 0, None, None, None, _p(chi), 1,
                                        _stream()), "tomo_cc_euler")
    return int(chi.item())


def component_topology(vol: BitVolume, connectivity=6, min_voxels=0, largest=False) -> ComponentTopology:
    """Per component of a resident volume: Euler number, cavities and handles (ComponentRuns.topology) -> ComponentTopology,
    one row per component the keep rule of component_properties selects (at least min_voxels voxels; largest: only the
    largest of those, the lowest label among equals), in ascending label: the rows, in the same order, component_properties
    returns for the same arguments.  A ball reads (1, 0, 0), a hollow shell (2, 1, 0), a ring (0, 0, 1).  A void that reaches
    a face of the stack is no cavity; an island floating in a void does not split it, and the island's own voids are the
    island's.  There are no slice depths here: topology does not depend on them.  Working memory scales with the rows, the
    runs of the volume and of its complement, and the components -- never with the voxels."""
    return ComponentRuns(vol, connectivity).topology_rows(min_voxels, largest)


def volume_topology(vol: BitVolume, connectivity=6) -> dict:
    """The topology of the whole volume -> {'components', 'cavities', 'handles', 'euler'}: the number of components and the
    sums of ComponentRuns.topology's columns; euler = components - handles + cavities = euler_number(vol, connectivity)."""
    topo = ComponentRuns(vol, connectivity).topology()
    euler, cavities, handles = (int(v) for v in topo.sum(dim=0).cpu()) if topo.shape[0] else (0, 0, 0)
    return {"components": int(topo.shape[0]), "cavities": cavities, "handles": handles, "euler": euler}


# ----------------------------------------------------------------------------- cavities: closed porosity
def _complement_runs(vol: BitVolume, connectivity) -> ComponentRuns:
    """The voids of a volume: its complement inside the stack, labelled under the complementary connectivity."""
    nz, ny, nx = vol.shape
    bits = vol.bits.contiguous()
    outside = torch.empty_like(bits)
    _lib.check(_lib.lib().tomo_cc_complement(_p(bits), nz, ny, nx, _p(outside), _stream()), "tomo_cc_complement")
    return ComponentRuns(BitVolume(outside, vol.shape), 32 - connectivity)


@dataclass
class Cavities:
    """cavity_table's answer: host arrays, one row per selected cavity in ascending cavity label."""
    labels: np.ndarray           # int64 (m,): the label of the cavity among the components of the complement
    owner: np.ndarray            # int64 (m,): the label of the component of the volume that encloses it
    voxels: np.ndarray           # int64 (m,)
    index_box: np.ndarray        # int64 (m, 6): zmin, zmax, ymin, ymax, xmin, xmax, inclusive
    volume_mm3: np.ndarray       # float64 (m,)
    centroid_mm: np.ndarray      # float64 (m, 3): z, y, x in the coordinates of distance_positions
    centroid_index: np.ndarray   # float64 (m, 3)

    def __len__(self):
        return len(self.labels)


def _cavities_from(runs: ComponentRuns, p: ComponentProperties) -> Cavities:
    """The rows of background().properties(enclosed=True) with the owners of runs.cavity_owners() gathered next to them."""
    if len(p):
        owner = runs.cavity_owners().index_select(0, torch.from_numpy(p.labels - 1).to(runs.vol.device)).cpu().numpy()
    else:
        owner = np.zeros(0, dtype=np.int64)
    return Cavities(p.labels, owner, p.voxels, p.index_box, p.volume_mm3, p.centroid_mm, p.centroid_index)


def cavity_table(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                 max_voxels=None) -> Cavities:
    """The enclosed voids of a resident volume, one row each -> Cavities.  The volume has connectivity k = 6 or 26, its
    complement the complementary 32 - k, everything outside the stack is background.  A cavity is a component of the
    complement whose inclusive index box touches no face of the stack; its label is its label there (raster order of the
    first voxel), its owner the component of the volume (label under k) that holds the voxel left of the cavity's first run: an
    island floating in a void does not own that void, and is no part of its size.  Rows: the cavities with min_voxels <=
    voxels <= max_voxels (None: no upper bound; min > max selects nothing), in ascending label.  voxels, index_box, volume_mm3,
    centroid_mm and centroid_index are component_properties' numbers for the mask of the cavity, bit for bit.  One labelling
    of the volume and one of the complement; an empty or a full volume has no rows.  Arguments are checked before the first
    launch; the budget of the per-slice counters is component_properties'."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    tables = _slice_weights(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    runs = ComponentRuns(vol, connectivity)
    if runs.runs == 0:                                                  # nothing encloses anything
        return _cavities_from(runs, _component_properties_from(*_PROPERTIES.empty(), float(mm_per_pixel_y), float(mm_per_pixel_x)))
    p = runs.background().properties(tables, mm_per_pixel_y, mm_per_pixel_x, lo, max_voxels=hi, enclosed=True)
    return _cavities_from(runs, p)


def cavity_sizes(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                 max_voxels=None):
    """cavity_table and, row for row, the pore size of every cavity -> (Cavities, ComponentThickness): the inscribed sphere of
    the cavity from ComponentRuns.thickness on the complement's tables -- the inside
    transform of the COMPLEMENT, the `enclosed` rule and the size window.  A cavity touches no face of the stack, so its nearest
    virtual site outside is never closer than a solid voxel: the numbers are those of the mask of the cavity.  One labelling of
    the volume and one of the complement serve both answers.  Arguments are checked before the first launch."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    tables = _slice_weights(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    runs = ComponentRuns(vol, connectivity)
    if runs.runs == 0:                                                  # nothing encloses anything
        p = _component_properties_from(*_PROPERTIES.empty(), float(mm_per_pixel_y), float(mm_per_pixel_x))
        empty = _component_thickness_from(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, np.zeros((0, 4), dtype=np.int64))
        return _cavities_from(runs, p), empty
    bg = runs.background()
    p = bg.properties(tables, mm_per_pixel_y, mm_per_pixel_x, lo, max_voxels=hi, enclosed=True)
    return _cavities_from(runs, p), bg.thickness(slice_depths, mm_per_pixel_y, mm_per_pixel_x, None, lo, max_voxels=hi, enclosed=True)


def _cavity_map(vol: BitVolume, connectivity, min_voxels, max_voxels, solid) -> BitVolume:
    """The voxels of the selected cavities of `vol`, ORed with `vol` itself when solid: complement, one labelling under the
    complementary connectivity, one selection, one pass over the words.  No labelling of the volume."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    bits = vol.bits.contiguous()
    COUNTERS["components_fill"] += 1
    bg = _complement_runs(BitVolume(bits, vol.shape), connectivity)
    picked = bg.select(lo, max_voxels=hi, enclosed=True) if bg.runs else None
    if picked is None:                                                  # empty, full, or no cavity in the window
        return BitVolume(bits.clone() if solid else torch.zeros_like(bits), vol.shape)
    out = torch.empty_like(bits)
    _lib.check(_lib.lib().tomo_cc_fill_map(_p(bg.bits), *vol.shape, *bg._tables(), _p(bg.tot), _p(picked.sel), picked.sel.shape[0],
                                           _p(bits) if solid else None, _p(out), _stream()), "tomo_cc_fill_map")
    bg._checked()
    return BitVolume(out, vol.shape)


def cavity_volume(vol: BitVolume, connectivity=6, min_voxels=0, max_voxels=None) -> BitVolume:
    """A NEW volume holding only the voxels of the cavities of `vol` (cavity_table's definition and size window): the pore
    space as a bit volume -- local_thickness of it is the pore-size distribution.  `vol` is left untouched; an empty or a full
    volume gives an empty one."""
    return _cavity_map(vol, connectivity, min_voxels, max_voxels, False)


def fill_cavities(vol: BitVolume, connectivity=6, min_voxels=0, max_voxels=None) -> BitVolume:
    """A NEW volume: `vol` with its cavities filled (cavity_table's definition; only those inside the size window).  Without a
    window it is scipy.ndimage.binary_fill_holes(volume, generate_binary_structure(3, 1 if connectivity == 26 else 3)) -- the
    structure is the BACKGROUND's -- on the resident bits: the 3-D counterpart of the fill close_ends does in the two end
    slices.  `vol` is left untouched; an empty volume comes back empty, a full one as a copy."""
    return _cavity_map(vol, connectivity, min_voxels, max_voxels, True)


# ----------------------------------------------------------------------------- surface area (Crofton)
_SURFACE_CLASS_STEPS = ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))   # (a_z, a_y, a_x): x y xy z xz yz xyz
_CROFTON_WEIGHTS = {}


def _voronoi_cell_area(a, others):
    """Area on the unit sphere of the set of unit vectors u closer to the unit vector `a` than to any row of `others`: the
    spherical polygon the half-spaces u . (a - b) >= 0 cut out.  Its corners lie among the normalised +-cross products of pairs
    of those normals; the ones that satisfy every constraint are ordered around a, and the area is the sum of the solid angles
    of the triangles (a, v_i, v_i+1) (Van Oosterom & Strackee)."""
    normals = a[None, :] - others
    i, j = np.triu_indices(len(normals), 1)
    cand = np.cross(normals[i], normals[j])
    length = np.linalg.norm(cand, axis=1)
    cand = cand[length > 1e-12] / length[length > 1e-12, None]
    cand = np.concatenate([cand, -cand])
    cand = cand[(cand @ normals.T >= -1e-12).all(axis=1)]
    corners = []
    for v in cand:                                                  # a corner where more than three cells meet comes several times
        if not any(np.linalg.norm(v - c) < 1e-9 for c in corners):
            corners.append(v)
    corners = np.asarray(corners)
    if len(corners) < 3:
        raise ValueError("crofton_weights: the spacings are too far apart for float64")
    e1 = corners[0] - (corners[0] @ a) * a                         # a frame of the tangent plane at a
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    corners = corners[np.argsort(np.arctan2(corners @ e2, corners @ e1))]
    nxt = np.roll(corners, -1, axis=0)
    det = np.abs(np.cross(corners, nxt) @ a)
    return float(np.sum(2.0 * np.arctan2(det, 1.0 + corners @ a + nxt @ a + np.sum(corners * nxt, axis=1))))


def crofton_weights(mm_x, mm_y, h, directions=13) -> np.ndarray:
    """The direction weights of the discretised Crofton formula for a lattice of spacing (h, mm_y, mm_x) along (z, y, x) ->
    float64 (7,), one per class in the order x, y, xy, z, xz, yz, xyz.  directions=13: twice the fraction of the unit sphere
    that is closer to the class's normalised lattice direction than to any other of the 26 (the area of its spherical Voronoi
    cell over 2 pi); over the 13 directions -- 1 + 1 + 2 + 1 + 2 + 2 + 4 of the classes -- the weights sum to 1.  A cubic
    lattice gives the published 0.0915558, 0.0739613 and 0.0703913.  directions=3: 1 / 3 for x, y and z, 0 otherwise.  Only
    the ratios of the spacings matter.  Pure NumPy, remembered per argument tuple."""
    if directions not in (3, 13):
        raise ValueError("directions must be 3 or 13")
    mm_x, mm_y, h = _positive(mm_x, "mm_x"), _positive(mm_y, "mm_y"), _positive(h, "h")
    key = (mm_x, mm_y, h, directions)
    w = _CROFTON_WEIGHTS.get(key)
    if w is None:
        if directions == 3:
            w = np.array([1, 1, 0, 1, 0, 0, 0], dtype=np.float64) / 3.0
        else:
            steps = np.array([(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dz or dy or dx],
                             dtype=np.float64)
            units = steps * np.array([h, mm_y, mm_x])
            units /= np.linalg.norm(units, axis=1)[:, None]
            w = np.empty(SURFACE_CLASSES, dtype=np.float64)
            for c, step in enumerate(_SURFACE_CLASS_STEPS):
                own = (steps == np.array(step, dtype=np.float64)).all(axis=1)
                w[c] = _voronoi_cell_area(units[own][0], units[~own]) / (2.0 * math.pi)
        w.setflags(write=False)
        if len(_CROFTON_WEIGHTS) >= 64:
            _CROFTON_WEIGHTS.clear()
        _CROFTON_WEIGHTS[key] = w
    return w.copy()


def surface_factors(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, directions=13) -> np.ndarray:
    """What one count of tomo_cc_surface_hist's column c in slice k adds to the area -> float64 (nz, 11):
    F[k][c] = 2 * w * (mm_x * mm_y * h) / L with h the lattice height of the column -- depth[k] in the slice, (depth[k] +
    depth[k + 1]) / 2 towards slice k + 1 (columns 3 .. 6), (depth[k - 1] + depth[k]) / 2 towards slice k - 1 (7 .. 10), the
    virtual slices -1 and nz as deep as the edge slice next to them -- w = crofton_weights(mm_x, mm_y, h, directions) of the
    column's class (a_z, a_y, a_x) and L = sqrt((a_z h)^2 + (a_y mm_y)^2 + (a_x mm_x)^2).  slice_depths=None: 1.0 per slice."""
    if directions not in (3, 13):
        raise ValueError("directions must be 3 or 13")
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)        # the argument checks
    nz = len(zt) - 2
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    d = np.concatenate([d[:1], d, d[-1:]])
    rows = {}

    def row(h):
        """The seven factors of a lattice of height h, computed once per distinct height."""
        h = float(h)
        if h not in rows:
            w = crofton_weights(mm_x, mm_y, h, directions)
            rows[h] = [2.0 * w[cls] * (mm_x * mm_y * h) / math.sqrt((az * h) ** 2 + (ay * mm_y) ** 2 + (ax * mm_x) ** 2)
                       for cls, (az, ay, ax) in enumerate(_SURFACE_CLASS_STEPS)]
        return rows[h]

    F = np.empty((nz, SURFACE_COUNTERS), dtype=np.float64)
    for cols, classes, heights in ((slice(0, 3), slice(0, 3), d[1:-1]), (slice(3, 7), slice(3, 7), (d[1:-1] + d[2:]) / 2.0),
                                   (slice(7, 11), slice(3, 7), (d[:-2] + d[1:-1]) / 2.0)):
        distinct, which = np.unique(heights, return_inverse=True)
        F[:, cols] = np.array([row(h) for h in distinct], dtype=np.float64)[which.reshape(-1), classes]
    return F


@dataclass
class SurfaceArea:
    """surface_area's answer."""
    surface_area_mm2: float
    pair_counts: np.ndarray      # int64 (7,): object / background transitions per class x, y, xy, z, xz, yz, xyz


@dataclass
class ComponentSurface:
    """component_surface's answer: host arrays, one row per selected component in ascending label."""
    labels: np.ndarray            # int64 (m,)
    voxels: np.ndarray            # int64 (m,)
    pair_counts: np.ndarray       # int64 (m, 7): transitions per class x, y, xy, z, xz, yz, xyz
    surface_area_mm2: np.ndarray  # float64 (m,)

    def __len__(self):
        return len(self.labels)


def surface_area(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, directions=13) -> SurfaceArea:
    """The surface area of a resident volume in mm^2 by the discretised Crofton formula (Ohser & Muecklich; the method of ITK's
    Perimeter and MorphoLibJ), without a mesh and without labelling.  For every set voxel and each of its 26 neighbours that is
    clear or outside the stack one transition is counted, per slice and per direction class; the area is the sequential
    float64 sum over the slices in ascending z of count * surface_factors(...), the spacing being distance_transform's
    (slice_depths=None: 1.0 per slice).  directions=3 uses the x, y and z transitions only: 2 / 3 of the exposed-face area.
    A ball is met within about half a percent; an axis-aligned flat face is underestimated (a cube of 8^3 voxels reads 0.8615
    of its face area): the known bias of the estimator.  Two launches, one host read."""
    nz, ny, nx = vol.shape
    F = surface_factors(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, directions)
    L, dev, st = _lib.lib(), vol.device, _stream()
    surf = torch.empty(SURFACE_COUNTERS * nz, dtype=torch.int64, device=dev)
    COUNTERS["components_surface"] += 1
    _lib.check(L.tomo_cc_surface_hist(_p(vol.bits.contiguous()), nz, ny, nx, None, 0, None, None, None, None, 0, None, None, _p(surf),
                                      nz, st), "tomo_cc_surface_hist")
    tab = torch.from_numpy(F).to(dev)
    out = torch.empty(2 + SURFACE_CLASSES, dtype=torch.float64, device=dev)       # the area, the label, the seven counts: one read
    words = out.view(torch.int64)
    _lib.check(L.tomo_cc_surface(None, 0, None, None, None, None, _p(surf), nz, _p(tab), nz, int(directions),
                                 _p(out), _p(words[2:]), _p(words[1:2]), 1, st), "tomo_cc_surface")
    host = out.cpu().numpy()
    return SurfaceArea(float(host[0]), host[2:].view(np.int64).copy())


def _component_surface_from(voxels, labels, counts, area) -> ComponentSurface:
    return ComponentSurface(labels, voxels, np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, SURFACE_CLASSES), area)


def component_surface(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                      largest=False, directions=13) -> ComponentSurface:
    """Surface area per component of a resident volume by the discretised Crofton formula (surface_area) -> ComponentSurface,
    one row per component the keep rule of component_properties selects (at least min_voxels voxels; largest: only the largest
    of those, the lowest label among equals), in ascending label: the rows, in the same order, component_properties returns
    for the same arguments.  A transition is a set voxel of the component next to a voxel that is clear or outside the stack;
    a set neighbour of ANOTHER component (diagonal contact under connectivity 6) is none, so under both connectivities the
    counts of all components add up to surface_area's.  The same four host reads as component_properties; working memory
    scales with the runs, the components and eleven counters per slice of the box of every SELECTED component (88 bytes an
    entry; beyond COMPONENT_HIST_BUDGET bytes for more than one component: TomoError) -- never with the voxels."""
    F = surface_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)
    return ComponentRuns(vol, connectivity).surface(F, directions, min_voxels, largest)


# ----------------------------------------------------------------------------- mean breadth (Crofton)
_BREADTH_NORMALS = tuple(m for m in itertools.product((-1, 0, 1), repeat=3) if m > (0, 0, 0))      # ascending (a_z, a_y, a_x)
_BREADTH_NO_CROSS = _BREADTH_NORMALS.index((1, 0, 0))               # the family whose cells all lie in one slice
_BREADTH_AXES = tuple(_BREADTH_NORMALS.index(m) for m in ((0, 0, 1), (0, 1, 0), (1, 0, 0)))


def breadth_normals() -> np.ndarray:
    """The Miller indices (a_z, a_y, a_x) of the 13 families of lattice planes of mean_breadth, first non-zero entry positive,
    in ascending tuple order -> int64 (13, 3): the columns of section_euler."""
    return np.array(_BREADTH_NORMALS, dtype=np.int64)


def breadth_factors(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, directions=13) -> np.ndarray:
    """What one unit of a section Euler number of slice k adds to the mean breadth -> float64 (nz, 26): B[k][f] = c_m * delta_m
    for family f of breadth_normals() on a lattice of height h = depth[k] (columns 0 .. 12: the cells inside the slice) and
    h = (depth[k] + depth[k + 1]) / 2 (columns 13 .. 25: the cells with corners in slice k + 1).  delta_m = 1 / |n| is the plane
    spacing, n = (a_z / h, a_y / mm_y, a_x / mm_x) the normal, and c_m = crofton_weights(1 / mm_x, 1 / mm_y, 1 / h, directions) of
    the class (|a_z|, |a_y|, |a_x|): the Voronoi shares of the normals, which are the lattice directions of the reciprocal box;
    over the 13 families they sum to 1.  directions=3: 1 / 3 for the three axis normals, 0 otherwise.  The cross columns are 0.0
    in the last slice, and that of (1, 0, 0) -- no cell of it leaves its slice -- everywhere.  slice_depths=None: 1.0 per slice."""
    if directions not in (3, 13):
        raise ValueError("directions must be 3 or 13")
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)        # the argument checks
    nz = len(zt) - 2
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    rows = {}

    def row(h):
        """The 13 factors of a lattice of height h, computed once per distinct height."""
        h = float(h)
        if h not in rows:
            w = crofton_weights(1.0 / mm_x, 1.0 / mm_y, 1.0 / h, directions)
            rows[h] = [w[_SURFACE_CLASS_STEPS.index((abs(az), abs(ay), abs(ax)))]
                       * (1.0 / math.sqrt((az / h) ** 2 + (ay / mm_y) ** 2 + (ax / mm_x) ** 2)) for az, ay, ax in _BREADTH_NORMALS]
        return rows[h]

    B = np.zeros((nz, BREADTH_COLUMNS), dtype=np.float64)
    for cols, rng, heights in ((slice(0, BREADTH_FAMILIES), slice(0, nz), d), (slice(BREADTH_FAMILIES, BREADTH_COLUMNS), slice(0, nz - 1),
                                                                            (d[:-1] + d[1:]) / 2.0)):
        if len(heights):
            distinct, which = np.unique(heights, return_inverse=True)
            B[rng, cols] = np.array([row(h) for h in distinct], dtype=np.float64)[which.reshape(-1)]
    B[:, BREADTH_FAMILIES + _BREADTH_NO_CROSS] = 0.0
    return B


@dataclass
class MeanBreadth:
    """mean_breadth's answer."""
    mean_breadth_mm: float
    section_euler: np.ndarray    # int64 (13,): the Euler numbers of the plane sections per family of breadth_normals()


@dataclass
class ComponentBreadth:
    """component_breadth's answer: host arrays, one row per selected component in ascending label."""
    labels: np.ndarray            # int64 (m,)
    voxels: np.ndarray            # int64 (m,)
    section_euler: np.ndarray     # int64 (m, 13): the Euler numbers of the plane sections per family of breadth_normals()
    mean_breadth_mm: np.ndarray   # float64 (m,)

    def __len__(self):
        return len(self.labels)


def mean_breadth(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, directions=13) -> MeanBreadth:
    """The mean breadth of a resident volume in mm -- the fourth Minkowski functional: 2 pi times it is the integral of mean
    curvature, and for a convex body it is the caliper diameter averaged over all directions -- by the discretised Crofton
    formula (Ohser & Muecklich), without a mesh and without labelling: b = sum over the 13 families of lattice planes of
    c_m * delta_m * chi_m, chi_m the Euler number V - E + F of the sections of the set by the planes of the family, on the
    lattice of the plane (include/tomo_hip.h has the cells).  The spacing is distance_transform's (slice_depths=None: 1.0 per
    slice): the cells inside slice k use its depth, those towards slice k + 1 the mean of the two; the sum is sequential
    float64 over the slices in ascending z and the columns of breadth_factors(...).  directions=3 uses the three axis normals
    only: a box of a x b x c mm reads (a + b + c) / 3 there.  A ball of R = 8 voxels reads 1.017 of 2 R, of R = 16 1.004; a box
    with axis-aligned faces is underestimated (0.873 of (a + b + c) / 2 for a cube): the flat-face bias surface_area has.  An
    inner surface counts negatively: a hollow ball reads outer minus inner diameter.  Two launches, one host read."""
    nz, ny, nx = vol.shape
    B = breadth_factors(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, directions)
    L, dev, st = _lib.lib(), vol.device, _stream()
    hist = torch.empty(BREADTH_WORDS * nz, dtype=torch.int64, device=dev)
    COUNTERS["components_breadth"] += 1
    _lib.check(L.tomo_cc_breadth_hist(_p(vol.bits.contiguous()), nz, ny, nx, None, 0, None, None, None, None, 0, None, None, _p(hist),
                                      nz, st), "tomo_cc_breadth_hist")
    tab = torch.from_numpy(B).to(dev)
    out = torch.empty(2 + BREADTH_FAMILIES, dtype=torch.float64, device=dev)      # the breadth, the label, the 13 numbers: one read
    words = out.view(torch.int64)
    _lib.check(L.tomo_cc_breadth(None, 0, None, None, None, None, _p(hist), nz, _p(tab), nz, int(directions),
                                 _p(out), _p(words[2:]), _p(words[1:2]), 1, st), "tomo_cc_breadth")
    host = out.cpu().numpy()
    return MeanBreadth(float(host[0]), host[2:].view(np.int64).copy())


def _component_breadth_from(voxels, labels, euler, breadth) -> ComponentBreadth:
    return ComponentBreadth(labels, voxels, np.ascontiguousarray(euler, dtype=np.int64).reshape(-1, BREADTH_FAMILIES), breadth)


def component_breadth(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                      largest=False, directions=13) -> ComponentBreadth:
    """Mean breadth per component of a resident volume by the discretised Crofton formula (mean_breadth) -> ComponentBreadth,
    one row per component the keep rule of component_properties selects (at least min_voxels voxels; largest: only the largest
    of those, the lowest label among equals), in ascending label: the rows, in the same order, component_properties returns
    for the same arguments.  Every cell (vertex, edge, face of a section) is anchored at its raster-first corner and credited
    to the component of that corner.  Under connectivity 26 all corners of a cell lie in one component, so a row is exactly the
    value of the mask `labels == c`; a cell across a diagonal contact under connectivity 6 goes to the component of its first
    corner, so under both connectivities the counts of all components add up to mean_breadth's.  The same four host reads as
    component_properties; working memory scales with the runs, the components and 18 counters per slice of the box of every
    SELECTED component (144 bytes an entry; beyond COMPONENT_HIST_BUDGET bytes for more than one component: TomoError) --
    never with the voxels."""
    B = breadth_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)
    return ComponentRuns(vol, connectivity).breadth(B, directions, min_voxels, largest)


def cavity_breadth(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                   max_voxels=None, directions=13) -> ComponentBreadth:
    """component_breadth of the enclosed voids of a resident volume, one row per cavity of cavity_table under the same size
    window (min_voxels <= voxels <= max_voxels), in ascending cavity label: the mean caliper diameter of a convex pore.  One
    labelling of the complement under the complementary connectivity, which is the one the cells of a cavity are credited
    under; an empty or a full volume has no rows.  Arguments are checked before the first launch."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    B = breadth_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)
    return _complement_runs(vol, connectivity).breadth(B, directions, lo, max_voxels=hi, enclosed=True)


# ----------------------------------------------------------------------------- chord lengths along the 13 lattice directions
CHORD_DIRECTIONS = 13
CHORD_FRACTION_BITS = 16     # the steps are summed in units of 2^-16 mm (tomo_profile_stats' fixed point)
CHORD_LDS_BINS = 256         # csrc/chords.hip: chords of fewer voxels have a bin of their own in LDS, longer ones share 256 slots
CHORD_PHASES = ("object", "background")


def chord_directions() -> np.ndarray:
    """The 13 forward steps (dz, dy, dx) of chord_lengths, first non-zero entry positive, in ascending tuple order -> int64
    (13, 3): the table of breadth_normals(), read as steps.  The rows of every table of ChordLengths."""
    return np.array(_BREADTH_NORMALS, dtype=np.int64)


def chord_steps(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0) -> np.ndarray:
    """The length in mm of one step of direction m through a voxel of slice k -> float64 (nz, 13):
    sqrt(((dz * depth[k])^2 + (dy * mm_y)^2) + (dx * mm_x)^2), the path through the voxel's own box (the convention of
    component_caliper(extent="voxels")).  slice_depths=None: 1.0 per slice."""
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)        # the argument checks
    nz = len(zt) - 2
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    s = chord_directions().astype(np.float64)
    return np.sqrt(((s[None, :, 0] * d[:, None]) ** 2 + (s[None, :, 1] * mm_y) ** 2) + (s[None, :, 2] * mm_x) ** 2)


def chord_steps_q(steps) -> np.ndarray:
    """chord_steps in the fixed point of the kernel -> int64, rint(steps * 65536), half to even."""
    return np.rint(np.asarray(steps, dtype=np.float64) * float(1 << CHORD_FRACTION_BITS)).astype(np.int64)


@dataclass
class ChordLengths:
    """chord_lengths' answer: host arrays, one row per direction of chord_directions(); L = max(nz, ny, nx)."""
    directions: np.ndarray       # int64 (13, 3): the steps (dz, dy, dx)
    counts: np.ndarray           # int64 (13, L + 1): chords of length n voxels; column 0 is 0
    border: np.ndarray           # int64 (13, L + 1): those of them whose predecessor or successor lies outside the stack
    sum_q: np.ndarray            # int64 (13, L + 1): the steps of their voxels in units of 2^-16 mm
    steps: np.ndarray            # float64 (nz, 13): chord_steps
    voxels: int                  # voxels of the phase: sum over n of n * counts[m][n] for every m
    chords: np.ndarray           # int64 (13,): chords per direction
    total_length_mm: np.ndarray  # float64 (13,): sum over k ascending of slice_counts[k] * steps[k][m]
    mean_chord_mm: np.ndarray    # float64 (13,): total_length_mm / chords, the mean intercept length; NaN without a chord
    shape: tuple                 # (nz, ny, nx)
    spacing: tuple               # (mean slice depth, mm_y, mm_x)

    def _counts(self, interior):
        return self.counts - self.border if interior else self.counts

    def mean_length_mm(self) -> np.ndarray:
        """The mean length in mm of the chords of every bin -> float64 (13, L + 1): sum_q / counts / 65536, NaN in an empty bin.
        At constant depth it is n times the step; with varying depths a bin of a direction with dz != 0 holds several lengths."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sum_q.astype(np.float64) / self.counts.astype(np.float64) / float(1 << CHORD_FRACTION_BITS)

    def quantiles_mm(self, fractions=(0.1, 0.5, 0.9)) -> np.ndarray:
        """Quantiles of the chord length by number of chords -> float64 (13, len(fractions)): mean_length_mm() of the first bin n
        at which the chords of at most n voxels are at least the fraction of all chords of the direction; NaN without a chord."""
        cum = np.cumsum(self.counts, axis=1)
        mean = self.mean_length_mm()
        out = np.full((CHORD_DIRECTIONS, len(fractions)), np.nan)
        for m in range(CHORD_DIRECTIONS):
            if self.chords[m] > 0:
                for c, f in enumerate(fractions):
                    n = int(np.searchsorted(cum[m], max(1, math.ceil(float(f) * int(self.chords[m]))), side="left"))
                    out[m, c] = mean[m, n]
        return out

    def segments(self) -> np.ndarray:
        """P_m(r), the segments of r voxels of direction m that lie inside the stack -> int64 (13, L + 1) (column 0 is 0):
        max(0, nz - (r - 1) |dz|) * max(0, ny - (r - 1) |dy|) * max(0, nx - (r - 1) |dx|)."""
        r = np.arange(self.counts.shape[1], dtype=np.int64)
        a = np.abs(self.directions)
        P = np.ones((CHORD_DIRECTIONS, len(r)), dtype=np.int64)
        for axis, size in enumerate(self.shape):
            P *= np.maximum(0, size - (r[None, :] - 1) * a[:, axis:axis + 1])
        P[:, 0] = 0
        return P

    def lineal_path(self, interior=False) -> np.ndarray:
        """The lineal-path function -> float64 (13, L + 1): L_m(r) = sum over n >= r of (n - r + 1) * counts[m][n] / P_m(r), the
        share of the r-voxel segments of direction m inside the stack (segments()) that lie wholly in the phase; 0 where P is
        0 and in column 0.  L_m(1) is the volume fraction.  interior=True counts the segments of the chords that are not cut
        by the stack only (counts - border) and leaves the denominators unchanged: a lower bound that does not depend on
        what lies beyond the faces."""
        c = self._counts(interior)
        tail = np.cumsum(c[:, ::-1], axis=1)[:, ::-1]                        # chords of at least r voxels
        num = np.cumsum(tail[:, ::-1], axis=1)[:, ::-1]                      # sum over n >= r of (n - r + 1) * c[n]
        P = self.segments()
        out = np.zeros(c.shape, dtype=np.float64)
        np.divide(num.astype(np.float64), P.astype(np.float64), out=out, where=P > 0)
        out[:, 0] = 0.0
        return out

    def mil_mm(self, interior=False) -> np.ndarray:
        """The mean intercept length per direction in mm -> float64 (13,), NaN without a chord.  interior=False: mean_chord_mm.
        interior=True: the mean length in voxels of the chords that are not cut by the stack (counts - border) times the step
        at the mean slice depth."""
        if not interior:
            return self.mean_chord_mm.copy()
        c = self._counts(True)
        n = np.arange(c.shape[1], dtype=np.int64)
        step = np.sqrt(((self.directions * np.array(self.spacing)) ** 2).sum(axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            return (c * n).sum(axis=1).astype(np.float64) / c.sum(axis=1).astype(np.float64) * step

    def fabric(self, interior=False) -> dict:
        """The MIL fabric tensor -> dict: the symmetric M (3, 3) in (z, y, x) that meets u^T M u = 1 / MIL(u)^2 in the least
        squares over the unit vectors u = s * (mean slice depth, mm_y, mm_x) / |.| of the directions that have a chord (the
        ellipsoid fit of Harrigan & Mann, BoneJ's Anisotropy on a fixed set of directions).  principal_mil_mm = 1 /
        sqrt(eigenvalues) in descending order; axes: the eigenvectors as rows in that order, the largest component positive;
        degree_of_anisotropy = 1 - lambda_min / lambda_max.  interior=True fits mil_mm(interior=True): the chords cut by the
        stack are left out, the step lengths are unchanged.  Fewer than six directions with a chord, or a fit that is not
        positive definite: ValueError."""
        mil = self.mil_mm(interior)
        has = np.isfinite(mil) & (mil > 0)
        if int(has.sum()) < 6:
            raise ValueError("the fabric tensor needs chords in at least six directions (%d have one)" % int(has.sum()))
        u = self.directions[has] * np.array(self.spacing)
        u = u / np.sqrt((u ** 2).sum(axis=1))[:, None]
        A = np.stack([u[:, 0] ** 2, u[:, 1] ** 2, u[:, 2] ** 2, 2 * u[:, 0] * u[:, 1], 2 * u[:, 0] * u[:, 2], 2 * u[:, 1] * u[:, 2]], axis=1)
        t = np.linalg.lstsq(A, 1.0 / mil[has] ** 2, rcond=None)[0]
        M = np.array([[t[0], t[3], t[4]], [t[3], t[1], t[5]], [t[4], t[5], t[2]]])
        lam, vec = np.linalg.eigh(M)                                         # ascending: the longest intercept first
        if not lam[0] > 0:
            raise ValueError("the fitted fabric tensor is not positive definite")
        axes = vec.T.copy()
        for row in axes:
            if row[np.argmax(np.abs(row))] < 0:
                row *= -1.0
        return {"tensor": M, "principal_mil_mm": 1.0 / np.sqrt(lam), "axes": axes,
                "degree_of_anisotropy": float(1.0 - lam[0] / lam[-1]), "directions_used": int(has.sum())}


def chord_lengths_from_tables(tables, slices, steps, shape, spacing) -> ChordLengths:
    """ChordLengths of the integer tables (3, 13, L + 1), the voxels per slice (nz,) and chord_steps: the host half of
    chord_lengths.  total_length_mm comes from the slice counts, not from sum_q: one checks the other."""
    counts, border, sum_q = (np.ascontiguousarray(t, dtype=np.int64) for t in tables)
    slices = np.asarray(slices, dtype=np.int64)
    chords = counts.sum(axis=1)
    total = np.zeros(CHORD_DIRECTIONS, dtype=np.float64)
    for k in range(len(slices)):                                             # sequential float64, ascending k
        total = total + float(slices[k]) * steps[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(chords > 0, total / chords.astype(np.float64), np.nan)
    return ChordLengths(chord_directions(), counts, border, sum_q, steps, int(slices.sum()), chords, total, mean,
                        tuple(int(s) for s in shape), tuple(float(s) for s in spacing))


def chord_lengths(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, phase="object") -> ChordLengths:
    """The chord lengths of a resident volume along the 13 lattice directions (chord_directions()) -> ChordLengths: how far one
    can go through the structure in a straight line, and which way it runs -- for the volume as a whole, without labelling.
    A chord is a maximal straight sequence of set voxels; everything outside the stack is background, and a chord that ends
    at a face of the stack is filed in `border` as well (include/tomo_hip.h has the definitions).  The spacing is
    distance_transform's (slice_depths=None: 1.0 per slice); the lengths in mm are sums of chord_steps in units of 2^-16 mm,
    integer atomics only: the same bytes on every run.  phase="background" measures the pore space: the same kernel on the
    complement inside the stack, where the chords cut by the stack are exactly the border chords.  One call of
    tomo_chord_hist (plus the complement's launch for the background) and the popcount per slice, one host read."""
    if phase not in CHORD_PHASES:
        raise ValueError("phase must be one of %s" % (CHORD_PHASES,))
    nz, ny, nx = vol.shape
    steps = chord_steps(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)
    d_mean = 1.0 if slice_depths is None else float(np.mean(np.asarray(slice_depths, dtype=np.float64)))
    L, dev, st = _lib.lib(), vol.device, _stream()
    bits = vol.bits.contiguous()
    if phase == "background":
        outside = torch.empty_like(bits)
        _lib.check(L.tomo_cc_complement(_p(bits), nz, ny, nx, _p(outside), st), "tomo_cc_complement")
        bits = outside
    lmax = max(nz, ny, nx)
    cells = CHORD_DIRECTIONS * (lmax + 1)
    out = torch.zeros(3 * cells + nz, dtype=torch.int64, device=dev)         # the three tables and the slice counts: one read
    tab = torch.from_numpy(chord_steps_q(steps)).to(dev)
    COUNTERS["chord_lengths"] += 1
    _lib.check(L.tomo_chord_hist(_p(bits), nz, ny, nx, _p(tab), lmax, _p(out), _p(out[cells:]), _p(out[2 * cells:]), st),
               "tomo_chord_hist")
    _lib.check(L.tomo_slice_popcounts(_p(bits), nz, ny, nx, _p(out[3 * cells:]), st), "tomo_slice_popcounts")
    host = out.cpu().numpy()
    return chord_lengths_from_tables(host[:3 * cells].reshape(3, CHORD_DIRECTIONS, lmax + 1), host[3 * cells:], steps, vol.shape,
                               (d_mean, float(mm_per_pixel_y), float(mm_per_pixel_x)))


# ----------------------------------------------------------------------------- the two-point covariance over a box of lags
TWO_POINT_WORK_BUDGET = 1 << 42      # words * lags one call may ask for: admits 1024^3 at (32, 32, 32), refuses it at (64, 64, 63)
TWO_POINT_MAX_RX = 63                # csrc/two_point.hip: a shifted word comes from a word and one neighbour
TWO_POINT_TABLE_LIMIT = 1 << 31      # entries of the table (tomo_two_point: TOMO_E_SIZE from there on)


def two_point_box(max_lag) -> tuple:
    """max_lag of two_point -> (Rz, Ry, Rx): an int stands for all three.  Integers >= 0, Rx <= 63; anything else is a
    ValueError naming max_lag (an int above 63 too: the box is never shrunk behind the caller's back)."""
    box = (max_lag,) * 3 if isinstance(max_lag, (int, np.integer)) and not isinstance(max_lag, (bool, np.bool_)) else max_lag
    try:
        box = tuple(box)
    except TypeError:
        raise ValueError("max_lag must be an int or (Rz, Ry, Rx), not %r" % (max_lag,)) from None
    if len(box) != 3 or any(isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)) for r in box):
        raise ValueError("max_lag must be an int or three ints (Rz, Ry, Rx), not %r" % (max_lag,))
    box = tuple(int(r) for r in box)
    if min(box) < 0:
        raise ValueError("max_lag must not be negative: %r" % (box,))
    if box[2] > TWO_POINT_MAX_RX:
        raise ValueError("max_lag along x is at most %d (a shifted word comes from a word and one neighbour): %r" % (TWO_POINT_MAX_RX, box))
    return box


@dataclass
class TwoPoint:
    """two_point's answer: the integer table of pair counts over the box of lags and what the host needs to read it.  Lag
    h = (hz, hy, hx) sits at [hz, hy + Ry, hx + Rx]; the half space hz >= 0 suffices because N(-h) = N(h).  Every method is NumPy
    on the integers with one pinned order of operations."""
    pairs: np.ndarray            # int64 (Rz + 1, 2 Ry + 1, 2 Rx + 1): N(h), the voxel pairs a lag h apart that both lie in the phase
    max_lag: tuple               # (Rz, Ry, Rx)
    shape: tuple                 # (nz, ny, nx)
    spacing: tuple               # (mean slice depth, mm_y, mm_x)
    voxels: int                  # voxels of the phase: N(0)
    phase: str
    z_lag_mm: np.ndarray         # float64 (Rz + 1,): the mean separation in mm of two slices hz apart; NaN from hz = nz on

    def _lags(self):
        rz, ry, rx = self.max_lag
        return (np.arange(rz + 1, dtype=np.int64)[:, None, None], np.arange(-ry, ry + 1, dtype=np.int64)[None, :, None],
                np.arange(-rx, rx + 1, dtype=np.int64)[None, None, :])

    def inside(self) -> np.ndarray:
        """P(h), the voxel pairs of the stack a lag h apart -> int64 box: max(0, nz - hz) * max(0, ny - |hy|) * max(0, nx - |hx|)."""
        hz, hy, hx = self._lags()
        nz, ny, nx = self.shape
        return np.maximum(0, nz - hz) * np.maximum(0, ny - np.abs(hy)) * np.maximum(0, nx - np.abs(hx))

    def s2(self) -> np.ndarray:
        """The two-point probability S2(h) = N(h) / P(h) -> float64 box, NaN where P = 0.  S2(0) is the volume fraction."""
        P = self.inside()
        out = np.full(P.shape, np.nan, dtype=np.float64)
        np.divide(self.pairs.astype(np.float64), P.astype(np.float64), out=out, where=P > 0)
        return out

    def volume_fraction(self) -> float:
        """S2(0) = N(0) / (nz ny nx)."""
        return float(self.voxels) / float(self.shape[0] * self.shape[1] * self.shape[2])

    def covariance(self) -> np.ndarray:
        """S2(h) - phi * phi, phi = S2(0) -> float64 box."""
        phi = self.volume_fraction()
        return self.s2() - phi * phi

    def correlation(self) -> np.ndarray:
        """covariance() / (phi - phi * phi) -> float64 box: 1 at h = 0, 0 where the two points are independent.  All NaN for an
        empty or a full phase."""
        phi = self.volume_fraction()
        var = phi - phi * phi
        if not var > 0.0:
            return np.full(self.pairs.shape, np.nan, dtype=np.float64)
        return self.covariance() / var

    def lag_mm(self) -> np.ndarray:
        """The length of every lag in mm -> float64 box: sqrt(((zbar(hz))^2 + (hy mm_y)^2) + (hx mm_x)^2), zbar = z_lag_mm: the
        mean of zc[k + hz] - zc[k] over the nz - hz slice pairs, summed in ascending k, zc the slice centres of
        distance_positions.  Exact under uniform depths.  Under varying depths the table is a covariance in INDEX lags and this
        is the mean separation of the pairs a lag stands for, not a distance every pair has.  NaN from hz = nz on."""
        hz, hy, hx = self._lags()
        _, mm_y, mm_x = self.spacing
        return np.sqrt((self.z_lag_mm[:, None, None] ** 2 + (hy * mm_y) ** 2) + (hx * mm_x) ** 2)

    def _along(self, box):
        """The values of a box at r * s for the 13 steps s of chord_directions(), r = 0 .. max(max_lag) -> float64 (13, R + 1),
        NaN where r * s leaves the box."""
        rz, ry, rx = self.max_lag
        R = max(self.max_lag)
        out = np.full((CHORD_DIRECTIONS, R + 1), np.nan, dtype=np.float64)
        for m, (dz, dy, dx) in enumerate(_BREADTH_NORMALS):
            for r in range(R + 1):
                if r * dz <= rz and abs(r * dy) <= ry and abs(r * dx) <= rx:
                    out[m, r] = box[r * dz, r * dy + ry, r * dx + rx]
        return out

    def directional(self) -> np.ndarray:
        """S2 along the 13 steps of chord_directions() -> float64 (13, R + 1), R = max(max_lag): S2 at the lag r * s; NaN where
        r * s leaves the box or P = 0."""
        return self._along(self.s2())

    def correlation_length_mm(self) -> np.ndarray:
        """Where correlation() first falls below 1 / e along each of the 13 directions -> float64 (13,): between the last lag
        r - 1 at or above and the first lag r below, d[r - 1] + (c[r - 1] - 1 / e) / (c[r - 1] - c[r]) * (d[r] - d[r - 1]) with d
        = lag_mm() there.  NaN if no crossing lies inside the box (or a NaN comes first)."""
        c, d = self._along(self.correlation()), self._along(self.lag_mm())
        level = 1.0 / math.e
        out = np.full(CHORD_DIRECTIONS, np.nan, dtype=np.float64)
        for m in range(CHORD_DIRECTIONS):
            for r in range(1, c.shape[1]):
                if not (np.isfinite(c[m, r]) and np.isfinite(c[m, r - 1])):
                    break
                if c[m, r] < level <= c[m, r - 1]:
                    out[m] = d[m, r - 1] + (c[m, r - 1] - level) / (c[m, r - 1] - c[m, r]) * (d[m, r] - d[m, r - 1])
                    break
        return out

    def radial(self, bin_mm) -> tuple:
        """The orientation average -> (centres float64 (n,), values float64 (n,), lags int64 (n,)): shell i holds the lags with
        floor(lag_mm / bin_mm + 0.5) == i and P > 0, its centre is i * bin_mm, its value sum(w N) / sum(w P) with w = 2 for
        hz > 0 (the lag stands for -h as well) and w = 1 in the plane hz = 0 (which holds both), `lags` the sum of w.  A shell
        without a lag reads NaN.  Shell 0 holds h = 0 at least: its value is the volume fraction when bin_mm is below the
        smallest spacing."""
        bin_mm = _positive(bin_mm, "bin_mm")
        P = self.inside()
        d = self.lag_mm()
        ok = (P > 0) & np.isfinite(d)
        shell = np.floor(d[ok] / bin_mm + 0.5).astype(np.int64)
        w = np.where(self._lags()[0] > 0, 2, 1).astype(np.int64) * np.ones(P.shape, dtype=np.int64)
        n = int(shell.max()) + 1 if shell.size else 0
        num, den, lags = (np.zeros(n, dtype=np.int64) for _ in range(3))
        np.add.at(num, shell, (w * self.pairs)[ok])
        np.add.at(den, shell, (w * P)[ok])
        np.add.at(lags, shell, w[ok])
        values = np.full(n, np.nan, dtype=np.float64)
        np.divide(num.astype(np.float64), den.astype(np.float64), out=values, where=den > 0)
        return np.arange(n, dtype=np.float64) * bin_mm, values, lags

    def specific_surface_per_mm(self) -> float:
        """The surface per volume of the stack in 1 / mm: 4 * sum over the 13 steps s_m, in their order, of c_m * (S2(0) -
        S2(s_m)) / |s_m|, |s_m| = sqrt(((dz h)^2 + (dy mm_y)^2) + (dx mm_x)^2) and c_m the weight of the step's class in
        crofton_weights(mm_x, mm_y, h), h the mean slice depth.  The slope of S2 at the origin read as Crofton's intersection
        count: 2 (N(0) - N(s)) is the object / background transitions along +-s that surface_area counts for a body clear of
        the faces.  The estimator of a structure that fills the stack (a foam, a bed, a rock): S2(s) = N(s) / P(s) corrects for
        the pairs the faces cut, so for ONE body in an otherwise empty stack it is not that body's surface over the stack's
        volume -- take 4 sum c_m (N(0) - N(s_m)) / |s_m| from `pairs` there, or surface_area.  Needs every R >= 1 (ValueError);
        NaN where an axis has one voxel."""
        if min(self.max_lag) < 1:
            raise ValueError("specific_surface_per_mm needs max_lag >= 1 along every axis, not %r" % (self.max_lag,))
        h, mm_y, mm_x = self.spacing
        c = crofton_weights(mm_x, mm_y, h, 13)
        s2 = self.directional()
        total = 0.0
        for m, (dz, dy, dx) in enumerate(_BREADTH_NORMALS):
            cls = _SURFACE_CLASS_STEPS.index((abs(dz), abs(dy), abs(dx)))
            total = total + c[cls] * (s2[m, 0] - s2[m, 1]) / math.sqrt(((dz * h) ** 2 + (dy * mm_y) ** 2) + (dx * mm_x) ** 2)
        return float(4.0 * total)


def two_point_z_lags(slice_depths, nz, rz) -> np.ndarray:
    """zbar(hz), hz = 0 .. rz -> float64 (rz + 1,): the mean of zc[k + hz] - zc[k] over k = 0 .. nz - hz - 1, summed in
    ascending k, zc the slice centres of distance_positions (slice_depths=None: 1.0 per slice); NaN from hz = nz on."""
    zc = distance_positions(slice_depths, nz)[0][1:-1]
    out = np.full(int(rz) + 1, np.nan, dtype=np.float64)
    for hz in range(min(int(rz), len(zc) - 1) + 1):
        total = 0.0
        for k in range(len(zc) - hz):
            total = total + (zc[k + hz] - zc[k])
        out[hz] = total / float(len(zc) - hz)
    return out


def two_point_from_table(pairs, max_lag, shape, spacing, phase, slice_depths=None) -> TwoPoint:
    """TwoPoint of an integer table: the host half of two_point (pure NumPy; a caller with a table of its own can use it).
    spacing: (mean slice depth, mm_y, mm_x); slice_depths=None: every slice as deep as the mean."""
    box = two_point_box(max_lag)
    shape = tuple(int(s) for s in shape)
    spacing = tuple(float(s) for s in spacing)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    if pairs.shape != (box[0] + 1, 2 * box[1] + 1, 2 * box[2] + 1):
        raise ValueError("the table of max_lag %r is %r, not %r" % (box, (box[0] + 1, 2 * box[1] + 1, 2 * box[2] + 1), pairs.shape))
    if phase not in CHORD_PHASES:
        raise ValueError("phase must be one of %s" % (CHORD_PHASES,))
    depths = np.full(shape[0], spacing[0]) if slice_depths is None else slice_depths
    return TwoPoint(pairs, box, shape, spacing, int(pairs[0, box[1], box[2]]), phase, two_point_z_lags(depths, shape[0], box[0]))


def two_point(vol: BitVolume, max_lag=16, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, phase="object") -> TwoPoint:
    """The two-point covariance of a resident volume over the box of integer lags hz in [0, Rz], hy in [-Ry, Ry], hx in
    [-Rx, Rx] (max_lag: an int or (Rz, Ry, Rx), Rx <= 63) -> TwoPoint: pairs[hz, hy + Ry, hx + Rx] = the voxel pairs a lag h
    apart that both lie in the phase and inside the stack -- no wrap-around, the non-periodic estimator; a lag that reaches
    the size of its axis reads 0 (include/tomo_hip.h has the definition).  From the integers, on the host: S2 = N / P, the
    covariance, the correlation and its length per direction, the radial average, the specific surface.  The table is a
    function of index lags alone; the spacing (distance_transform's; slice_depths=None: 1.0 per slice) enters on the host.
    phase="background" measures the pore space: the same kernel on the complement inside the stack.  words * lags beyond
    TWO_POINT_WORK_BUDGET, or a table of 2^31 entries or more, is a ValueError before anything is allocated.  Integer adds
    only: the same bytes on every run.  One call of tomo_two_point (plus the complement's launch), one host read."""
    if phase not in CHORD_PHASES:
        raise ValueError("phase must be one of %s" % (CHORD_PHASES,))
    rz, ry, rx = two_point_box(max_lag)
    nz, ny, nx = vol.shape
    distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)                              # the argument checks
    d_mean = 1.0 if slice_depths is None else float(np.mean(np.asarray(slice_depths, dtype=np.float64)))
    cells = (rz + 1) * (2 * ry + 1) * (2 * rx + 1)
    words = nz * ny * ((nx + 63) // 64)
    if cells >= TWO_POINT_TABLE_LIMIT:
        raise ValueError("max_lag %r asks for a table of %d entries; fewer than 2^31 can be served" % ((rz, ry, rx), cells))
    if words * cells > TWO_POINT_WORK_BUDGET:
        raise ValueError("max_lag %r on %r is %d words * %d lags, beyond TWO_POINT_WORK_BUDGET = %d: take a smaller max_lag"
                         % ((rz, ry, rx), tuple(vol.shape), words, cells, TWO_POINT_WORK_BUDGET))
    L, dev, st = _lib.lib(), vol.device, _stream()
    bits = vol.bits.contiguous()
    if phase == "background":
        outside = torch.empty_like(bits)
        _lib.check(L.tomo_cc_complement(_p(bits), nz, ny, nx, _p(outside), st), "tomo_cc_complement")
        bits = outside
    out = torch.empty(cells, dtype=torch.int64, device=dev)                  # zeroed by the call itself
    COUNTERS["two_point"] += 1
    _lib.check(L.tomo_two_point(_p(bits), nz, ny, nx, rz, ry, rx, _p(out), st), "tomo_two_point")
    host = out.cpu().numpy().reshape(rz + 1, 2 * ry + 1, 2 * rx + 1)
    depths = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    return two_point_from_table(host, (rz, ry, rx), vol.shape, (d_mean, float(mm_per_pixel_y), float(mm_per_pixel_x)), phase, depths)


# ----------------------------------------------------------------------------- Euclidean distance in millimetres
EDT_WORKSPACE_BUDGET = 1 << 30      # bytes of scratch a distance call may take; at least one 64-column chunk is always granted


def _positive(x, what):
    x = float(x)
    if not (math.isfinite(x) and x > 0):
        raise ValueError("%s must be positive and finite" % what)
    return x


def distance_positions(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, ny=None, nx=None):
    """The coordinate tables of the distance transform, on the host -> (zt, yt, xt) float64 with n + 2 entries each: entry
    i + 1 is the centre of index i -- point_cloud_z_table's slice centres along z, j * mm_per_pixel_y, i * mm_per_pixel_x --
    and entries 0 / n + 1 are the virtual background sites one step outside the volume (along z one end-slice depth, the
    end-slice repetition of SurfaceExtractor._apply_variable_slice_depths).  slice_depths=None: depth 1.0 per slice.
    yt / xt are None when ny / nx is not given."""
    nz = int(nz)
    d = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    if nz < 1 or len(d) != nz:
        raise ValueError("slice_depths must hold one depth per slice (%d for nz = %d)" % (len(d), nz))
    if not (np.isfinite(d).all() and (d > 0).all()):
        raise ValueError("slice depths must be positive and finite")
    zc = point_cloud_z_table(d, nz)
    zt = np.concatenate([[zc[0] - d[0]], zc, [zc[-1] + d[-1]]])
    mm_y, mm_x = _positive(mm_per_pixel_y, "mm_per_pixel_y"), _positive(mm_per_pixel_x, "mm_per_pixel_x")
    yt = None if ny is None else np.arange(-1, int(ny) + 1, dtype=np.float64) * mm_y
    xt = None if nx is None else np.arange(-1, int(nx) + 1, dtype=np.float64) * mm_x
    return zt, yt, xt


class _DistancePlan:
    """What the three distance calls share: the bits, the tables on the device (one upload) and the chunked workspace."""

    def __init__(self, vol: BitVolume, slice_depths, mm_per_pixel_y, mm_per_pixel_x):
        nz, ny, nx = vol.shape
        tables = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, ny, nx)
        for t in tables:
            if not (np.diff(t) > 0).all():
                raise ValueError("the spacing is too small against the extent: two positions coincide in float64")
        L = _lib.lib()
        self.vol, self.bits = vol, vol.bits.contiguous()
        self.host_tables = tables
        tab = torch.from_numpy(np.concatenate(tables)).to(vol.device)
        self.tab = tab
        self.zt, self.yt, self.xt = tab[:nz + 2], tab[nz + 2:nz + ny + 4], tab[nz + ny + 4:]
        self.ws_bytes = int(L.tomo_edt_workspace_bytes(nz, ny, nx, EDT_WORKSPACE_BUDGET))
        if self.ws_bytes <= 0:
            raise _lib.TomoError("tomo_edt_workspace_bytes failed (%d)" % self.ws_bytes)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=vol.device)

    def head(self):
        nz, ny, nx = self.vol.shape
        return _p(self.bits), nz, ny, nx, _p(self.zt), _p(self.yt), _p(self.xt)

    def tail(self):
        return _p(self.ws), self.ws_bytes, _stream()


def distance_transform(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, inside=True) -> torch.Tensor:
    """Exact Euclidean distance transform of a resident volume in millimetres -> float32 (nz, ny, nx) device tensor.
    Voxel (k, j, i) sits at (zc[k], j * mm_per_pixel_y, i * mm_per_pixel_x), zc = point_cloud_z_table(slice_depths, nz);
    everything outside the volume is background (distance_positions: one layer of virtual sites).  inside=True: at a set
    voxel the distance to the nearest unset site, 0.0 at an unset one.  inside=False: at an unset voxel the distance to the
    nearest set voxel, 0 at a set one, +inf everywhere in an empty volume.  With uniform depths and inside=True this is
    distance_transform_edt(np.pad(v, 1), sampling=(d, mm_y, mm_x))[1:-1, 1:-1, 1:-1].  Scratch: tomo_edt_workspace_bytes,
    at most EDT_WORKSPACE_BUDGET unless one 64-column chunk needs more."""
    plan = _DistancePlan(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    out = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    COUNTERS["distance_transform"] += 1
    _lib.check(_lib.lib().tomo_edt_distance(*plan.head(), int(bool(inside)), _p(out), *plan.tail()), "tomo_edt_distance")
    return out


def offset_volume(vol: BitVolume, radius_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0) -> BitVolume:
    """Erosion / dilation by a ball of radius_mm millimetres -> a NEW BitVolume; `vol` is left untouched.
    radius_mm < 0: the set voxels whose inside distance is > |radius_mm|.  radius_mm > 0: `vol` plus the unset voxels whose
    outside distance is <= radius_mm; the shape stays, so nothing grows past the volume.  radius_mm == 0: a copy.
    The squared distance is compared with radius_mm ** 2 in float64 inside the last pass and balloted into bit words: the
    call allocates the output words, the three small coordinate tables and the chunked scratch of distance_transform
    (bounded by EDT_WORKSPACE_BUDGET; it scales with nz * ny * the chunk's columns) -- never a float per voxel."""
    r = float(radius_mm)
    if not math.isfinite(r):
        raise ValueError("radius_mm must be finite")
    plan = _DistancePlan(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    COUNTERS["distance_offset"] += 1
    if r == 0:
        return BitVolume(plan.bits.clone(), vol.shape)
    out = torch.empty_like(plan.bits)
    _lib.check(_lib.lib().tomo_edt_threshold(*plan.head(), int(r < 0), r * r, int(r < 0), _p(out), *plan.tail()),
               "tomo_edt_threshold")
    return BitVolume(out, vol.shape)


def inscribed_sphere(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0):
    """The largest sphere that fits inside the object: the maximum of distance_transform(inside=True) and the first voxel in
    raster order that attains it -> (radius_mm, (k, j, i)) in Python numbers, None for an empty volume.  No float volume is
    made (a per-thread maximum folded in a fixed order); one host read."""
    nz, ny, nx = vol.shape
    plan = _DistancePlan(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    res = torch.empty(2, dtype=torch.int64, device=vol.device)
    COUNTERS["distance_transform"] += 1
    _lib.check(_lib.lib().tomo_edt_argmax(*plan.head(), 1, _p(res), *plan.tail()), "tomo_edt_argmax")
    bits32, flat = _download(res)
    radius = float(np.array([bits32], dtype=np.int64).astype(np.uint32).view(np.float32)[0])
    if flat < 0 or not radius > 0:
        return None
    return radius, (flat // (ny * nx), flat // nx % ny, flat % nx)


# ----------------------------------------------------------------------------- local thickness and ball openings
LOCAL_THICKNESS_MAX_LEVELS = 512               # distinct squared distances local_thickness' exact mode takes as levels
# bytes the float64 squared distances of a local_thickness call may take (8 B per voxel): 8 GiB admits 512^3 (1 GiB) and
# 1024^3 (exactly 8 GiB), not 2048 x 1024^2
LOCAL_THICKNESS_VOLUME_BUDGET = 1 << 33


@dataclass
class LocalThickness:
    """local_thickness' answer.  Level k (0-based here) is the open ball of radius radii_mm[k]."""
    thickness: torch.Tensor        # float32 (nz, ny, nx) on the device: the diameter 2 r of the voxel's level, 0.0 where none
    radii_mm: np.ndarray           # float64 (K,): the levels used, ascending
    level_voxels: np.ndarray       # int64 (K,): set voxels whose level is k
    level_volume_mm3: np.ndarray   # float64 (K,): their volume under the slice depths
    uncovered_voxels: int          # set voxels below radii_mm[0]
    mean_mm: float                 # of the diameter over the covered set voxels, weighted by volume
    std_mm: float
    max_mm: float


def _check_radii(radii_mm) -> np.ndarray:
    r = np.asarray(radii_mm, dtype=np.float64).reshape(-1)
    if len(r) == 0 or not (np.isfinite(r).all() and (r > 0).all() and (np.diff(r) > 0).all()):
        raise ValueError("radii_mm must be a non-empty, strictly ascending list of positive finite radii")
    return r


def _thickness_statistics(radii, level_volume):
    """(mean, std, max) of the diameter 2 r over the covered voxels, weighted by volume; exactly rounded sums (math.fsum)."""
    d = [2.0 * float(r) for r in radii]
    w = [float(v) for v in level_volume]
    total = math.fsum(w)
    if not total > 0:
        return 0.0, 0.0, 0.0
    mean = math.fsum(wi * di for wi, di in zip(w, d)) / total
    var = math.fsum(wi * ((di - mean) * (di - mean)) for wi, di in zip(w, d)) / total
    return mean, math.sqrt(var), max(di for wi, di in zip(w, d) if wi > 0)


def _thickness_levels(plan: _DistancePlan, d2, r2, live, level_map, eroded):
    """The level loop local_thickness and ComponentRuns.thickness share: for the first `live` squared radii, ascending, the
    eroded set {set && d2 >= r2} balloted into `eroded` and its outside transform, whose tail writes the level into the zeroed
    int32 level_map where it covers a set voxel.  The caller owns both buffers (eroded: None without a live level)."""
    L = _lib.lib()
    bits, nzyx, tables = plan.head()[0], plan.head()[1:4], plan.head()[4:]
    for k in range(live):
        _lib.check(L.tomo_edt_at_least(_p(d2), bits, *nzyx, float(r2[k]), _p(eroded), _stream()), "tomo_edt_at_least")
        _lib.check(L.tomo_edt_cover(_p(eroded), bits, *nzyx, *tables, float(r2[k]), k + 1, _p(level_map), *plan.tail()), "tomo_edt_cover")


# ----------------------------------------------------------------------------- inscribed sphere and thickness per component
@dataclass
class ComponentThickness:
    """component_thickness' answer: host arrays, one row per selected component in ascending label.  The fields from radii_mm
    on are None without radii."""
    labels: np.ndarray             # int64 (m,)
    voxels: np.ndarray             # int64 (m,)
    radius_mm: np.ndarray          # float64 (m,): the largest float32 inside distance of the component, widened
    center_index: np.ndarray       # int64 (m, 3): (k, j, i) of the first voxel in raster order that attains it
    center_mm: np.ndarray          # float64 (m, 3): that voxel in the coordinates of distance_positions
    radii_mm: np.ndarray = None            # float64 (K,): the levels, ascending
    level_voxels: np.ndarray = None        # int64 (m, K): voxels of the component whose level is k
    level_volume_mm3: np.ndarray = None    # float64 (m, K): their volume under the slice depths
    uncovered_voxels: np.ndarray = None    # int64 (m,): voxels of the component below radii_mm[0]
    mean_mm: np.ndarray = None             # float64 (m,): _thickness_statistics per row
    std_mm: np.ndarray = None
    max_mm: np.ndarray = None

    def __len__(self):
        return len(self.labels)


def _thickness_measurement(K) -> _Measurement:
    """The level histogram of K levels as a measurement of ComponentRuns._rows: K + 1 words per slice of a selected box."""
    return _Measurement("component_thickness", ((torch.int64, (K + 1,)), (torch.float64, (K,))), 0, K + 1,
                        "voxels per slice and thickness level", "tomo_cc_level_hist", "components_levels", "tomo_cc_level_sums")


def _component_thickness_args(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, radii_mm):
    """The argument checks of component_thickness, all on the host -> (radii or None, slice weights): the radii, the depths and
    pixel sizes, and with radii the memory guard of local_thickness, raised before anything is allocated."""
    radii = None if radii_mm is None else _check_radii(radii_mm)
    nz, ny, nx = shape
    weights = _slice_weights(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)[:nz]
    if radii is not None and 8 * nz * ny * nx > LOCAL_THICKNESS_VOLUME_BUDGET:
        raise ValueError("component_thickness: the squared distances of a %d x %d x %d volume take %d bytes, more than "
                         "LOCAL_THICKNESS_VOLUME_BUDGET (%d)" % (nz, ny, nx, 8 * nz * ny * nx, LOCAL_THICKNESS_VOLUME_BUDGET))
    return radii, weights


def _thickness_statistics_rows(radii, volume) -> np.ndarray:
    """_thickness_statistics of every row of volume float64 (m, K) -> float64 (m, 3).  Millions of specks share a handful of
    level tables, so the rows are grouped first and the statistics computed once per distinct row: a 64-bit mix of the bits of
    a row is the key (one flat sort), and every row is then compared with the one that stands for its key -- a collision
    falls back to sorting the rows themselves."""
    m, K = volume.shape
    if m == 0:
        return np.zeros((0, 3), dtype=np.float64)
    words = volume.view(np.uint64)
    key = np.zeros(m, dtype=np.uint64)
    for k in range(K):
        key = (key ^ words[:, k]) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(k + 1)       # wraps: that is the mix
    _, first, row = np.unique(key, return_index=True, return_inverse=True)
    distinct = volume[first]
    if not np.array_equal(distinct[row].view(np.uint64), words):
        distinct, row = np.unique(volume, axis=0, return_inverse=True)
    stats = np.array([_thickness_statistics(radii, v) for v in distinct], dtype=np.float64).reshape(-1, 3)
    return stats[np.asarray(row).reshape(-1)]


def _component_thickness_from(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, rows, radii=None, levels=None) -> ComponentThickness:
    """Host side of the downloaded rows: rows int64 (m, 4) as tomo_cc_value_rows writes them; levels: _rows' download of the
    level histogram (voxels, labels, level counts (m, K + 1), level volumes (m, K)), None for no selected component."""
    nz, ny, nx = shape
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
    m = len(rows)
    flat = rows[:, 3]
    index = np.stack([flat // (ny * nx), flat // nx % ny, flat % nx], axis=1).astype(np.int64)
    zt, yt, xt = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, ny, nx)
    centre = np.stack([zt[index[:, 0] + 1], yt[index[:, 1] + 1], xt[index[:, 2] + 1]], axis=1).astype(np.float64)
    out = ComponentThickness(rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].astype(np.uint32).view(np.float32).astype(np.float64),
                             index, centre)
    if radii is None:
        return out
    K = len(radii)
    if levels is None:
        counts, volume = np.zeros((0, K + 1), dtype=np.int64), np.zeros((0, K), dtype=np.float64)
    else:
        _, labels, counts, volume = levels
        if not np.array_equal(labels, out.labels):
            raise _lib.TomoError("component_thickness: the rows of the level histogram are not the rows of the selection")
    stats = _thickness_statistics_rows(radii, np.ascontiguousarray(volume, dtype=np.float64))
    out.radii_mm, out.level_voxels, out.level_volume_mm3 = radii, counts[:, 1:].copy(), np.ascontiguousarray(volume)
    out.uncovered_voxels = counts[:, 0].copy()
    out.mean_mm, out.std_mm, out.max_mm = stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy()
    return out


def component_thickness(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                        largest=False, radii_mm=None) -> ComponentThickness:
    """The inscribed sphere and, with radii_mm, the local thickness per component of a resident volume -> ComponentThickness,
    one row per component the keep rule of component_properties selects (at least min_voxels voxels; largest: only the largest
    of those, the lowest label among equals), in ascending label: the rows component_properties returns for the same rule.
    radius_mm is the maximum of distance_transform(inside=True) over the component and center_index the first voxel in raster
    order that attains it: inscribed_sphere of the mask `labels == c`, bit for bit.  radii_mm (a strictly ascending list of
    positive finite radii): level_voxels, level_volume_mm3, uncovered_voxels, mean_mm, std_mm and max_mm are what
    local_thickness(mask of the component, radii_mm=radii_mm) returns, per row.
    Neither number needs the mask: the nearest background site of a voxel is never a voxel of ANOTHER component (stepping from it
    towards the voxel ends at an unset voxel that is no farther), and an open digital ball round a centre where it fits is
    connected through set voxels, so the transform and the level map of the whole volume, read under the component, are the
    component's own.  Cost without radii: one float32 inside transform (4 B per voxel) and two passes over it; with radii: ONE
    float64 transform for both parts, local_thickness' level loop once for the whole volume, and a histogram of K + 1 counters
    per slice of every selected component's box (beyond COMPONENT_HIST_BUDGET bytes for more than one component: TomoError) --
    never a transform per component.  With radii the squared distances take 8 B per voxel: beyond
    LOCAL_THICKNESS_VOLUME_BUDGET a ValueError before anything is allocated.  Integer atomics only: the same bytes on every run.
    An empty volume, or nothing selected, gives zero rows.  Arguments are checked before the first launch."""
    _check_connectivity(connectivity)
    _keep_rule(min_voxels, largest)
    _component_thickness_args(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, radii_mm)
    return ComponentRuns(vol, connectivity).thickness(slice_depths, mm_per_pixel_y, mm_per_pixel_x, radii_mm, min_voxels, largest)


# ----------------------------------------------------------------------------- caliper (Feret) diameters and the oriented box
CALIPER_DIRECTIONS = 64      # directions of the default set: the three axes and a Fibonacci lattice on the upper hemisphere
CALIPER_EXTENTS = ("voxels", "centres")
CALIPER_PROBES = 200000      # probe vectors of caliper_cover


def caliper_directions(count=CALIPER_DIRECTIONS) -> np.ndarray:
    """The default direction set -> float64 (count, 3) unit vectors as (z, y, x).  Rows 0-2 are the axes z, y, x; the other
    n = count - 3 rows are a Fibonacci lattice on the upper hemisphere (u and -u measure the same width): z_i = (i + 0.5) / n,
    phi_i = i pi (3 - sqrt 5), row (z, r sin phi, r cos phi) with r = sqrt(1 - z^2).  count < 3: ValueError."""
    count = int(count)
    if count < 3:
        raise ValueError("caliper_directions: count must be at least 3 (the axes)")
    out = np.zeros((count, 3), dtype=np.float64)
    out[0, 0] = out[1, 1] = out[2, 2] = 1.0
    n = count - 3
    if n:
        i = np.arange(n, dtype=np.float64)
        z = (i + 0.5) / n
        r = np.sqrt(1.0 - z * z)
        phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
        rows = np.stack([z, r * np.sin(phi), r * np.cos(phi)], axis=1)
        out[3:] = rows / np.sqrt((rows * rows).sum(axis=1))[:, None]
    return out


def caliper_cover(directions) -> float:
    """How far the largest width over a direction set can fall short of the true max Feret diameter: the smallest max_m |q . u_m|
    over CALIPER_PROBES unit probe vectors q (normalised normal deviates of numpy.random.default_rng(0)).  A segment of length D
    along q has width D |q . u| along u, so max_mm >= cover * D.  Measured: 0.9669 for caliper_directions(64), 0.9823 for 128,
    0.9922 for 256."""
    u = _check_directions(directions)
    q = np.random.default_rng(0).standard_normal((CALIPER_PROBES, 3))
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    worst = 1.0
    for a in range(0, len(q), 20000):                                   # 20 000 x M products at a time
        worst = min(worst, float(np.abs(q[a:a + 20000] @ u.T).max(axis=1).min()))
    return worst


def _check_directions(directions) -> np.ndarray:
    """directions=None: the default set; else float64 (M, 3) C-contiguous, M >= 1, finite, unit within 1e-12 (ValueError)."""
    if directions is None:
        return caliper_directions()
    try:
        u = np.ascontiguousarray(directions, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("directions must be a float (M, 3) array") from None
    if u.ndim != 2 or u.shape[1] != 3 or u.shape[0] < 1:
        raise ValueError("directions must have the shape (M, 3) with M >= 1, not %s" % (u.shape,))
    if not np.isfinite(u).all():
        raise ValueError("directions must be finite")
    if (np.abs(np.sqrt((u * u).sum(axis=1)) - 1.0) > 1e-12).any():
        raise ValueError("directions must be unit vectors (within 1e-12)")
    return u


@dataclass
class _CaliperTables:
    """The host tables of one caliper call (include/tomo_hip.h, tomo_cc_caliper)."""
    zc: np.ndarray               # float64 (nz,), (ny,), (nx,): where a voxel sits, the inner entries of distance_positions
    yt: np.ndarray
    xt: np.ndarray
    depth: np.ndarray            # float64 (nz,): the real depth of every slice
    pz: np.ndarray               # float64 (M, nz), (M, ny), (M, nx): the projections of those on every direction
    py: np.ndarray
    px: np.ndarray
    h: np.ndarray                # float64 (M, nz): half the width of a voxel's box along every direction; None: extent="centres"


def _caliper_args(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, directions, extent):
    """The argument checks of component_caliper, all on the host -> (directions float64 (M, 3), _CaliperTables)."""
    if extent not in CALIPER_EXTENTS:
        raise ValueError("extent must be 'voxels' or 'centres'")
    u = _check_directions(directions)
    nz, ny, nx = shape
    zt, yt, xt = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, ny, nx)
    zc, yt, xt = zt[1:-1].copy(), yt[1:-1].copy(), xt[1:-1].copy()
    depth = np.ones(nz) if slice_depths is None else np.asarray(slice_depths, dtype=np.float64).reshape(-1).copy()
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    a = np.abs(u)
    h = None if extent == "centres" else 0.5 * ((a[:, 0:1] * depth[None, :] + a[:, 1:2] * mm_y) + a[:, 2:3] * mm_x)
    return u, _CaliperTables(zc, yt, xt, depth, zc[None, :] * u[:, 0:1], yt[None, :] * u[:, 1:2], xt[None, :] * u[:, 2:3], h)


@dataclass
class ComponentCaliper:
    """component_caliper's answer: host arrays, one row per selected component in ascending label; vectors in (z, y, x) order.
    The fields from axes on are None without oriented."""
    labels: np.ndarray                     # int64 (m,)
    voxels: np.ndarray                     # int64 (m,)
    directions: np.ndarray                 # float64 (M, 3): the shared directions
    hi_mm: np.ndarray                      # float64 (m, M): the largest projection (extent="voxels": of the voxel boxes)
    lo_mm: np.ndarray                      # float64 (m, M): the smallest
    width_mm: np.ndarray                   # float64 (m, M): hi_mm - lo_mm, the caliper diameter along every direction
    max_mm: np.ndarray                     # float64 (m,): the largest width ...
    max_index: np.ndarray                  # int64 (m,): ... its direction, the lowest index among equals ...
    max_direction: np.ndarray              # float64 (m, 3): ... and that row of directions
    min_mm: np.ndarray                     # float64 (m,): the smallest width, likewise
    min_index: np.ndarray
    min_direction: np.ndarray
    axes: np.ndarray = None                # float64 (m, 3, 3): component_moments' principal_axes, rows
    oriented_extent_mm: np.ndarray = None  # float64 (m, 3): the widths along those
    oriented_center_mm: np.ndarray = None  # float64 (m, 3): the midpoints (hi + lo) / 2 along the axes, mapped back to (z, y, x)
    oriented_volume_mm3: np.ndarray = None  # float64 (m,): the product of the three extents

    def __len__(self):
        return len(self.labels)


def _component_caliper_from(dirs, shared=None, moments=None, own=None, oriented=False) -> ComponentCaliper:
    """Host side of the downloaded rows: shared / own = (rows int64 (m, 4), hi, lo, width float64 (m, M), ext float64 (m, 2)) as
    tomo_cc_caliper_rows writes them for the shared directions / the component's own axes; shared=None: no selected component."""
    M = len(dirs)
    if shared is None:
        shared = (np.zeros((0, 4), dtype=np.int64), *(np.zeros((0, M), dtype=np.float64) for _ in range(3)), np.zeros((0, 2), dtype=np.float64))
        if oriented:
            own = (np.zeros((0, 4), dtype=np.int64), *(np.zeros((0, 3), dtype=np.float64) for _ in range(3)), np.zeros((0, 2), dtype=np.float64))
    rows, hi, lo, width, ext = shared
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
    imax, imin = rows[:, 2].copy(), rows[:, 3].copy()
    out = ComponentCaliper(rows[:, 0].copy(), rows[:, 1].copy(), dirs, np.ascontiguousarray(hi), np.ascontiguousarray(lo),
                           np.ascontiguousarray(width), ext[:, 0].copy(), imax, dirs[imax], ext[:, 1].copy(), imin, dirs[imin])
    if oriented:
        _, ohi, olo, owidth, _ = own
        axes = np.zeros((0, 3, 3), dtype=np.float64) if moments is None else np.ascontiguousarray(moments.principal_axes)
        mid = 0.5 * (ohi + olo)
        centre = (mid[:, 0:1] * axes[:, 0, :] + mid[:, 1:2] * axes[:, 1, :]) + mid[:, 2:3] * axes[:, 2, :]
        out.axes, out.oriented_extent_mm, out.oriented_center_mm = axes, np.ascontiguousarray(owidth), np.ascontiguousarray(centre)
        out.oriented_volume_mm3 = (owidth[:, 0] * owidth[:, 1]) * owidth[:, 2]
    return out


def component_caliper(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                      largest=False, directions=None, extent="voxels", oriented=False) -> ComponentCaliper:
    """Caliper (Feret) diameters per component of a resident volume -> ComponentCaliper, one row per component the keep rule of
    component_properties selects (at least min_voxels voxels; largest: only the largest of those, the lowest label among
    equals), in ascending label: the rows component_properties returns for the same rule.
    The caliper diameter along a unit vector u = (u_z, u_y, u_x) is the distance between the two planes with normal u that
    hold the component between them: width = hi - lo.  Voxel (k, j, i) sits at (zc[k], j mm_y, i mm_x), the coordinates of
    distance_transform, and projects to p = ((zc[k] u_z + j mm_y u_y) + i mm_x u_x) + 0.0, every product and sum rounded on
    its own.  extent="centres": hi = max p, lo = min p over the voxels.  extent="voxels" (the default): the union of the voxel
    boxes, hi = max(p + H), lo = min(p - H) with H = 0.5 ((|u_z| d_k + |u_y| mm_y) + |u_x| mm_x), d_k the depth of slice k: one
    voxel reads its own box width along u, not 0.  directions: float (M, 3) unit vectors (within 1e-12) shared by all
    components; None: caliper_directions(), CALIPER_DIRECTIONS = 64 of them.  max_mm / min_mm are the largest and the
    smallest width over the set, with the index and the row of the direction (the lowest index among equals).  max_mm is the
    max Feret diameter up to the set's cover factor (caliper_cover: max_mm >= 0.9669 D for the default set, 0.9823 for 128
    directions, 0.9922 for 256) and never above it; min_mm is an UPPER bound of the min Feret diameter: the width a sieve must
    have for the grain to pass is at most that.
    oriented=True: component_moments runs first under the same rule, and every component is also measured along its own
    principal axes: axes (component_moments' principal_axes, bytes equal), oriented_extent_mm (the widths along them: the box
    aligned with the moment axes -- not the minimum-volume box), oriented_center_mm (the midpoints along the axes mapped back
    to (z, y, x) mm) and oriented_volume_mm3 (the product of the extents).
    Cost: a projection is monotone along an x-run, so only the two ends of every run are evaluated: one pass over the rows per
    8 directions, nothing per voxel.  Memory: 16 M bytes per SELECTED component for the extremes (beyond COMPONENT_HIST_BUDGET
    for more than one component: TomoError naming min_voxels) -- nothing per component of the volume.  Maxima and minima of
    integer keys only: the same bytes on every run, and bit for bit what NumPy gives over all voxels.  An empty volume, or
    nothing selected, gives zero rows.  Arguments are checked before the first launch."""
    _check_connectivity(connectivity)
    _keep_rule(min_voxels, largest)
    _caliper_args(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, directions, extent)
    return ComponentRuns(vol, connectivity).caliper(slice_depths, mm_per_pixel_y, mm_per_pixel_x, directions, extent, oriented,
                                                    min_voxels, largest)


def cavity_caliper(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, min_voxels=0,
                   max_voxels=None, directions=None, extent="voxels", oriented=False) -> ComponentCaliper:
    """component_caliper of the enclosed voids of a resident volume, one row per cavity of cavity_table under the same size
    window (min_voxels <= voxels <= max_voxels), in ascending cavity label: how long and how wide a pore is -- a crack reads its
    length in max_mm and its opening in min_mm, where the equivalent diameter is no size at all.  One labelling of the
    complement under the complementary connectivity; an empty or a full volume has no rows.  Arguments are checked before the
    first launch."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    _caliper_args(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x, directions, extent)
    bg = _complement_runs(vol, connectivity)
    return bg.caliper(slice_depths, mm_per_pixel_y, mm_per_pixel_x, directions, extent, oriented, lo, max_voxels=hi, enclosed=True)


# ----------------------------------------------------------------------------- geodesic distance
GEODESIC_SWEEP_BATCH = 8             # sweeps enqueued between two reads of the change counter (a sweep of a clean volume returns at once)
GEODESIC_SWEEP_LIMIT = 1 << 16       # a guard against an endless host loop, no tuning knob; read when called
GEODESIC_VOLUME_BUDGET = 1 << 33     # bytes of the float32 map (a zone call: of its three per-voxel maps); read when called


def geodesic_weights(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0):
    """The step weights of the geodesic metric, on the host -> (wxy float32 (3,): the steps x, y, xy; wz float32
    (max(nz - 1, 1), 4): the steps z, zx, zy, zyx across the boundary between slice k and k + 1).  A weight is the Euclidean
    length of the step in mm, float64 sqrt(((dx mm_x)^2 + (dy mm_y)^2) + dzc^2) with dzc = zc[k + 1] - zc[k] of
    distance_positions, rounded once to float32."""
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    dzc = np.diff(zt[1:-1])
    steps = np.array([(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)])               # (dx, dy) of x, y, xy
    plane = (steps[:, 0] * mm_x) * (steps[:, 0] * mm_x) + (steps[:, 1] * mm_y) * (steps[:, 1] * mm_y)
    wxy = np.sqrt(plane + 0.0 * 0.0).astype(np.float32)
    wz = np.zeros((max(int(nz) - 1, 1), 4), dtype=np.float32)
    if len(dzc):
        inplane = np.concatenate([[0.0], plane[[0, 1, 2]]])             # z, zx, zy, zyx
        wz[:] = np.sqrt(inplane[None, :] + (dzc * dzc)[:, None]).astype(np.float32)
    return wxy, wz


@dataclass
class _GeodesicTables:
    """The host side of one geodesic call: the weights and where a voxel sits."""
    wxy: np.ndarray
    wz: np.ndarray
    zc: np.ndarray
    mm_y: float
    mm_x: float
    shape: tuple


def _geodesic_tables(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x) -> _GeodesicTables:
    """The argument checks every geodesic call shares, all on the host."""
    nz = shape[0]
    wxy, wz = geodesic_weights(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)
    if not ((wxy > 0).all() and np.isfinite(wxy).all() and (nz < 2 or ((wz > 0).all() and np.isfinite(wz).all()))):
        raise ValueError("the spacing does not give positive finite float32 step lengths")
    return _GeodesicTables(wxy, wz, zt[1:-1].copy(), float(mm_per_pixel_y), float(mm_per_pixel_x), tuple(int(a) for a in shape))


def _geodesic_search_sweeps(sweeps) -> int:
    if isinstance(sweeps, (bool, np.bool_)) or not isinstance(sweeps, (int, np.integer)) or sweeps < 2:
        raise ValueError("sweeps must be a whole number of at least 2")
    return int(sweeps)


class _GeodesicPlan:
    """What the sweeps of one geodesic call share: the bits, the weights on the device, the two dirty arrays and the counters.
    tables=None: a plan without weights, for the sweeps that read none (propagate_reconstruction)."""

    def __init__(self, vol: BitVolume, tables, connectivity):
        nz, ny, nx = vol.shape
        nbytes = 4 * nz * ny * nx
        if nbytes > GEODESIC_VOLUME_BUDGET:                              # read when called, before anything is allocated
            raise _lib.TomoError("geodesic distance: the float32 map of %d x %d x %d voxels takes %d bytes, more than "
                                 "GEODESIC_VOLUME_BUDGET (%d)" % (nz, ny, nx, nbytes, GEODESIC_VOLUME_BUDGET))
        L = _lib.lib()
        self.tiles = int(L.tomo_geo_tiles(nz, ny, nx))
        if self.tiles <= 0:
            raise _lib.TomoError("tomo_geo_tiles failed (%d)" % self.tiles)
        dev = vol.device
        self.vol, self.bits, self.connectivity = vol, vol.bits.contiguous(), int(connectivity)
        if tables is not None:
            w = torch.from_numpy(np.concatenate([tables.wxy, tables.wz.reshape(-1)])).to(dev)
            self.w, self.wxy, self.wz = w, w[:3], w[3:]
        self.dirty = torch.zeros((2, self.tiles), dtype=torch.int32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.cur = 0                                                     # the dirty array the next sweep reads
        self.changed = 0                                                 # counters[0] as last read

    def seed_tail(self):
        """What the two seeding entry points take behind dist (tomo_geo_seed_bits: without the counters)."""
        return _p(self.dirty[self.cur]), _p(self.counters)

    def _sweeps(self, launch, what, counter) -> int:
        """launch(cur, next) enqueues one sweep; batches of GEODESIC_SWEEP_BATCH until one changes nothing -> the sweeps launched."""
        limit, batch = int(GEODESIC_SWEEP_LIMIT), max(1, int(GEODESIC_SWEEP_BATCH))
        done = 0
        while True:
            if done >= limit:
                raise _lib.TomoError("%s: no fixed point after %d sweeps (GEODESIC_SWEEP_LIMIT)" % (what, done))
            k = min(batch, limit - done)
            for _ in range(k):
                launch(_p(self.dirty[self.cur]), _p(self.dirty[1 - self.cur]))
                self.cur = 1 - self.cur
            done += k
            COUNTERS[counter] += k
            changed = _download(self.counters)[0]
            if changed == self.changed:
                return done
            self.changed = changed

    def propagate(self, dist: torch.Tensor) -> int:
        """Sweeps until a batch changes nothing -> the sweeps launched.  No seed: none.  Termination is guaranteed -- values only
        fall and come from a finite set; GEODESIC_SWEEP_LIMIT only guards the host loop."""
        L, st = _lib.lib(), _stream()
        nz, ny, nx = self.vol.shape
        if not bool(self.dirty[self.cur].any().item()):
            return 0

        def sweep(cur, nxt):
            _lib.check(L.tomo_geo_sweep(_p(self.bits), nz, ny, nx, self.connectivity, _p(self.wxy), _p(self.wz), _p(dist), cur, nxt,
                                        _p(self.counters), st), "tomo_geo_sweep")
        return self._sweeps(sweep, "geodesic distance", "geodesic_sweeps")

    def propagate_zones(self, dist: torch.Tensor, zone: torch.Tensor) -> int:
        """The label phase over the FINAL dist of propagate(), which left every flag clear -> the sweeps launched.  It starts with
        every flag set (one fill): a tile without work changes nothing, marks nobody and is out after the first sweep.  Labels
        only fall through a finite set, so it ends; the loop and its guard are propagate()'s."""
        L, st = _lib.lib(), _stream()
        nz, ny, nx = self.vol.shape
        self.dirty[self.cur].fill_(1)

        def sweep(cur, nxt):
            _lib.check(L.tomo_zone_sweep(_p(self.bits), nz, ny, nx, self.connectivity, _p(self.wxy), _p(self.wz), _p(dist), _p(zone),
                                         cur, nxt, _p(self.counters), st), "tomo_zone_sweep")
        return self._sweeps(sweep, "geodesic zones", "zone_sweeps")

    def propagate_reconstruction(self, mask: torch.Tensor, g: torch.Tensor) -> int:
        """The sweeps of a grey reconstruction over tomo_recon_seed's g -> the sweeps launched.  It starts with every flag set, as
        propagate_zones does.  Values only rise through the finite set of the inputs, so it ends; the loop and its guard are
        propagate()'s."""
        L, st = _lib.lib(), _stream()
        nz, ny, nx = self.vol.shape
        self.dirty[self.cur].fill_(1)

        def sweep(cur, nxt):
            _lib.check(L.tomo_recon_sweep(_p(self.bits), nz, ny, nx, self.connectivity, _p(mask), _p(g), cur, nxt, _p(self.counters), st),
                       "tomo_recon_sweep")
        return self._sweeps(sweep, "reconstruction", "recon_sweeps")


def _geodesic_seeds(shape, seeds):
    """seeds -> ("bits", BitVolume) or ("index", int64 host array of flat indices); ValueError for anything else."""
    nz, ny, nx = shape
    if isinstance(seeds, BitVolume):
        if tuple(seeds.shape) != tuple(shape):
            raise ValueError("seeds must have the shape of the volume")
        return "bits", seeds
    a = seeds.detach().cpu().numpy() if isinstance(seeds, torch.Tensor) else np.asarray(seeds)
    if a.size == 0:
        return "index", np.zeros(0, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
        raise ValueError("seeds must be a BitVolume or an integer array (n, 3) of (z, y, x)")
    a = a.astype(np.int64)
    if (a < 0).any() or (a >= np.array([nz, ny, nx])).any():
        raise ValueError("a seed lies outside the volume")
    return "index", (a[:, 0] * ny + a[:, 1]) * nx + a[:, 2]


def _geodesic_map(vol: BitVolume, seeds, tables: _GeodesicTables, connectivity):
    """-> (float32 map, the plan that made it)."""
    kind, s = seeds
    L, dev, st = _lib.lib(), vol.device, _stream()
    nz, ny, nx = vol.shape
    plan = _GeodesicPlan(vol, tables, connectivity)
    COUNTERS["geodesic_calls"] += 1
    if kind == "bits":
        dist = torch.empty(vol.shape, dtype=torch.float32, device=dev)
        _lib.check(L.tomo_geo_seed_bits(_p(plan.bits), _p(s.bits.contiguous()), nz, ny, nx, _p(dist), plan.seed_tail()[0], st),
                   "tomo_geo_seed_bits")
    else:
        dist = torch.full(vol.shape, float("inf"), dtype=torch.float32, device=dev)
        if len(s):
            index = torch.from_numpy(s).to(dev)
            _lib.check(L.tomo_geo_seed_index(_p(plan.bits), nz, ny, nx, _p(index), None, len(s), _p(dist), *plan.seed_tail(), st),
                       "tomo_geo_seed_index")                            # a seed on an unset voxel is ignored: the flag is not read
    plan.propagate(dist)
    return dist, plan


def geodesic_distance(vol: BitVolume, seeds, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=26) -> torch.Tensor:
    """Geodesic distance from the seeds through the set voxels of a resident volume, in millimetres -> float32 (nz, ny, nx)
    device tensor: 0.0 at a seed that is set, +inf at a set voxel no seed reaches and at every unset voxel.  seeds: a BitVolume
    of the same shape, or an integer array (n, 3) of (z, y, x); a seed on an unset voxel is ignored.
    The metric: voxel (k, j, i) sits at (zc[k], j mm_y, i mm_x), the coordinates of distance_transform; a step goes between
    two set voxels that are neighbours under the connectivity (6 or 26; the 26-adjacency of the two ends alone, no
    corner-cutting test: label_components' adjacency, so a path never leaves a component) and weighs its Euclidean length in
    mm (geodesic_weights); the distance is the minimum over the paths of the left-to-right float32 sum of the weights.  That
    is the path length on the 6 / 26 lattice: exact along the lattice directions and an overestimate between them, like any
    chamfer metric, and a float32 sum carries float32's relative precision along a very long path.
    The device relaxes 8 x 8 x 64 tiles in LDS, sweep after sweep, until a batch of GEODESIC_SWEEP_BATCH sweeps changes
    nothing; d' = fl32(d + w) is monotone in d, so every order of relaxations ends at the same bytes -- those Dijkstra's
    algorithm with the same float32 additions returns.  More than GEODESIC_SWEEP_LIMIT sweeps: TomoError; a map of more than
    GEODESIC_VOLUME_BUDGET bytes: TomoError before anything is allocated.  An empty volume, or no seed on a set voxel: no
    sweep is launched.  Arguments are checked before the first launch."""
    connectivity = _check_connectivity(connectivity)
    tables = _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return _geodesic_map(vol, _geodesic_seeds(vol.shape, seeds), tables, connectivity)[0]


def geodesic_reach(vol: BitVolume, seeds, max_mm=None, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0,
                   connectivity=26) -> BitVolume:
    """The set voxels within max_mm millimetres of a seed along geodesic_distance's paths (dist <= max_mm) -> a NEW BitVolume:
    the geodesic ball.  max_mm=None: every voxel a seed reaches -- the binary reconstruction of the seeds in the volume, the
    components a seed touches."""
    connectivity = _check_connectivity(connectivity)
    r = float("inf") if max_mm is None else float(max_mm)
    if not r >= 0:
        raise ValueError("max_mm must be non-negative or None")
    tables = _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    dist, plan = _geodesic_map(vol, _geodesic_seeds(vol.shape, seeds), tables, connectivity)
    out = torch.empty_like(plan.bits)
    _lib.check(_lib.lib().tomo_geo_reach(_p(plan.bits), _p(dist), *vol.shape, r, _p(out), _stream()), "tomo_geo_reach")
    return BitVolume(out, vol.shape)


@dataclass
class ComponentGeodesic:
    """component_geodesic's answer: host arrays, one row per selected component in ascending label; vectors in (z, y, x) order."""
    labels: np.ndarray           # int64 (m,)
    voxels: np.ndarray           # int64 (m,)
    length_mm: np.ndarray        # float64 (m,): the distance of the last search (a float32 value), centre to centre
    ends_index: np.ndarray       # int64 (m, 2, 3): the two ends of that search, (z, y, x)
    ends_mm: np.ndarray          # float64 (m, 2, 3): where they sit
    chord_mm: np.ndarray         # float64 (m,): the straight distance between the two end centres
    tortuosity: np.ndarray       # float64 (m,): length_mm / chord_mm, 1.0 where the chord is 0

    def __len__(self):
        return len(self.labels)


def _component_geodesic_from(tables: _GeodesicTables, rows, rows_prev) -> ComponentGeodesic:
    """Host side of the downloaded rows (label, voxels, float32 bits of the distance, flat index) of the last search and of its
    start."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
    rows_prev = np.ascontiguousarray(rows_prev, dtype=np.int64).reshape(-1, 4)
    m = len(rows)
    length = rows[:, 2].astype(np.uint32).view(np.float32).astype(np.float64)
    ends = np.zeros((m, 2, 3), dtype=np.int64)
    mm = np.zeros((m, 2, 3), dtype=np.float64)
    if m:
        nz, ny, nx = tables.shape
        for e, flat in enumerate((rows_prev[:, 3], rows[:, 3])):
            ends[:, e, 0], rest = np.divmod(flat, ny * nx)
            ends[:, e, 1], ends[:, e, 2] = np.divmod(rest, nx)
        mm[:, :, 0] = tables.zc[ends[:, :, 0]]
        mm[:, :, 1] = ends[:, :, 1] * tables.mm_y
        mm[:, :, 2] = ends[:, :, 2] * tables.mm_x
    d = mm[:, 1, :] - mm[:, 0, :]
    chord = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    tort = np.ones(m, dtype=np.float64)
    np.divide(length, chord, out=tort, where=chord > 0)
    return ComponentGeodesic(rows[:, 0].copy(), rows[:, 1].copy(), length, ends, mm, chord, tort)


def component_geodesic(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, sweeps=3,
                       min_voxels=0, largest=False) -> ComponentGeodesic:
    """Geodesic length per component of a resident volume -> ComponentGeodesic, one row per component the keep rule of
    component_properties selects, in ascending label: the rows component_properties returns for the same rule.
    The method is the repeated farthest-point search (as in MorphoLibJ's geodesic diameter), for all selected components at
    once: a0 = the first voxel of the component in raster order; `sweeps` times (at least 2: ValueError) the geodesic distance
    is propagated from a(s - 1) and a_s is the farthest voxel of the component, the lowest flat index among equals.
    length_mm is the distance of the last search, ends_index / ends_mm its two ends (a(sweeps - 1), a_sweeps), chord_mm the
    straight distance between the end centres and tortuosity their ratio (1.0 where the chord is 0).  The metric is
    geodesic_distance's with the steps of `connectivity`; length_mm is a LOWER bound of the geodesic diameter on that metric,
    and it is centre to centre: one voxel reads 0.0.  A coiled fibre or a bent crack reads its length here, where the caliper
    diameter reads the width of the coil.  An empty volume, or nothing selected, gives zero rows.  Arguments are checked
    before the first launch."""
    _check_connectivity(connectivity)
    _keep_rule(min_voxels, largest)
    _geodesic_search_sweeps(sweeps)
    _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return ComponentRuns(vol, connectivity).geodesic(slice_depths, mm_per_pixel_y, mm_per_pixel_x, sweeps, min_voxels, largest)


def cavity_geodesic(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6, sweeps=3,
                    min_voxels=0, max_voxels=None) -> ComponentGeodesic:
    """component_geodesic of the enclosed voids of a resident volume, one row per cavity of cavity_table under the same size
    window, in ascending cavity label: how long a pore is along itself.  One labelling of the complement under the
    complementary connectivity, whose steps the paths take; an empty or a full volume has no rows.  Arguments are checked
    before the first launch."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    _geodesic_search_sweeps(sweeps)
    _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    bg = _complement_runs(vol, connectivity)
    return bg.geodesic(slice_depths, mm_per_pixel_y, mm_per_pixel_x, sweeps, lo, max_voxels=hi, enclosed=True)


# ----------------------------------------------------------------------------- zones of markers, the cut, the separation
def _zone_markers(vol: BitVolume, markers):
    """markers -> ("bits", BitVolume) or ("map", int32 device tensor); TypeError / ValueError for anything else, on the host."""
    if isinstance(markers, BitVolume):
        if tuple(markers.shape) != tuple(vol.shape):
            raise ValueError("markers must have the shape of the volume")
        if markers.device != vol.device:
            raise ValueError("markers must be on the volume's device")
        return "bits", markers
    return "map", _zone_map(vol, markers, "markers")


def _zone_map(vol: BitVolume, m, what) -> torch.Tensor:
    if not isinstance(m, torch.Tensor):
        raise TypeError("%s must be %san int32 tensor (nz, ny, nx)" % (what, "a BitVolume or " if what == "markers" else ""))
    if m.dtype != torch.int32:
        raise TypeError("%s must be int32" % what)
    if tuple(m.shape) != tuple(vol.shape):
        raise ValueError("%s must have the shape of the volume" % what)
    if m.device != vol.device:
        raise ValueError("%s must be on the volume's device" % what)
    return m


def _zone_budget(shape):
    """Before anything is allocated: a zone call holds three per-voxel maps at once."""
    nz, ny, nx = shape
    nbytes = 12 * nz * ny * nx
    if nbytes > GEODESIC_VOLUME_BUDGET:
        raise _lib.TomoError("geodesic zones: the float32 distance map, the int32 zone map and the int32 marker map of %d x %d x %d "
                             "voxels take %d bytes, more than GEODESIC_VOLUME_BUDGET (%d)" % (nz, ny, nx, nbytes, GEODESIC_VOLUME_BUDGET))


def _geodesic_zones(vol: BitVolume, markers, tables: _GeodesicTables, connectivity):
    """-> (zones, dist, (distance sweeps, label sweeps), the marker components of a BitVolume or None)."""
    kind, m = markers
    _zone_budget(vol.shape)
    L, dev = _lib.lib(), vol.device
    nz, ny, nx = vol.shape
    count = None
    if kind == "bits":
        m, count = ComponentRuns(m, connectivity).labels()
    plan = _GeodesicPlan(vol, tables, connectivity)
    COUNTERS["zone_calls"] += 1
    dist = torch.empty(vol.shape, dtype=torch.float32, device=dev)
    zone = torch.empty(vol.shape, dtype=torch.int32, device=dev)
    _lib.check(L.tomo_zone_seed_labels(_p(plan.bits), _p(m.contiguous()), nz, ny, nx, _p(dist), _p(zone), plan.seed_tail()[0], _stream()),
               "tomo_zone_seed_labels")
    far = plan.propagate(dist)                                           # phase one: the distances, to their fixed point
    near = plan.propagate_zones(dist, zone) if far else 0               # phase two: the labels over the final distances
    return zone, dist, (far, near), count


def geodesic_zones(vol: BitVolume, markers, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=26):
    """Which marker reaches a voxel first through the object -> (zones int32 (nz, ny, nx) device tensor, dist float32 device
    tensor): the geodesic influence zones of the markers inside the set voxels of a resident volume.
    markers: an int32 device tensor of the volume's shape -- a positive entry on a set voxel is a marker voxel with that label,
    entries <= 0 and entries on unset voxels are ignored, labels need not be consecutive -- or a BitVolume, which is labelled
    under `connectivity` with ComponentRuns(markers, connectivity).labels(): 1 .. n in raster order.
    dist is geodesic_distance(vol, the marker voxels) under the same spacing and connectivity, byte for byte.  An edge q -> p
    between neighbouring set voxels is tight when fl32(dist(q) + w(q, p)) == dist(p) with dist(p) finite -- the float32 addition
    the distance sweep makes; zone(p) is the smallest marker label among the markers from which p can be reached along tight
    edges, 0 at unset voxels and at set voxels no marker reaches; a marker voxel keeps its label.  That is the least fixed point
    of zone(p) = min(zone(p), zone(q) over tight q -> p) over a fixed graph: one answer, whatever the schedule.
    Two phases on the device: the distance sweeps of geodesic_distance to their fixed point, then label sweeps over the final
    distances (tomo_zone_sweep), in the same host loop: GEODESIC_SWEEP_BATCH sweeps between two counter reads, more than
    GEODESIC_SWEEP_LIMIT: TomoError.  The call holds three per-voxel maps at once (dist, zones, the marker map); more than
    GEODESIC_VOLUME_BUDGET bytes: TomoError before anything is allocated.  An empty volume, or no marker on a set voxel: zones
    all 0, no sweep is launched.  Arguments are checked before the first launch."""
    connectivity = _check_connectivity(connectivity)
    tables = _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    zone, dist, _, _ = _geodesic_zones(vol, _zone_markers(vol, markers), tables, connectivity)
    return zone, dist


def _split_zones(vol: BitVolume, zones: torch.Tensor, connectivity):
    """-> (the cut BitVolume, the 1-element int64 device counter of the cleared voxels)."""
    bits = vol.bits.contiguous()
    out = torch.empty_like(bits)
    cleared = torch.zeros(1, dtype=torch.int64, device=vol.device)
    COUNTERS["zone_cuts"] += 1
    _lib.check(_lib.lib().tomo_zone_cut(_p(bits), _p(zones.contiguous()), *vol.shape, connectivity, _p(out), _p(cleared), _stream()),
               "tomo_zone_cut")
    return BitVolume(out, vol.shape), cleared


def split_zones(vol: BitVolume, zones: torch.Tensor, connectivity=26) -> BitVolume:
    """The cut between zones -> a NEW BitVolume; `vol` is left untouched.  A set voxel p is cleared when some neighbour q under
    the connectivity is set with 0 < zones(q) < zones(p): the lower label keeps the contact.  Afterwards no two voxels of
    different zones are adjacent, so every component of the result lies in one zone; a component without a marker (zones 0)
    is untouched.  zones: geodesic_zones' map, or any int32 device tensor of the volume's shape (entries <= 0 are no zone)."""
    connectivity = _check_connectivity(connectivity)
    return _split_zones(vol, _zone_map(vol, zones, "zones"), connectivity)[0]


@dataclass
class Separation:
    """separate_components' answer."""
    volume: BitVolume            # the cut volume: every per-component measurement applies to it unchanged
    markers: int                 # marker components the zones grew from
    cut_voxels: int              # set voxels the cut cleared
    zones: torch.Tensor          # int32 (nz, ny, nx) device tensor: geodesic_zones of the markers
    sweeps: tuple                # (distance sweeps, label sweeps) launched


def _separation_args(shape, radius_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels):
    """The argument checks of separate_components, all on the host -> (radius, tables, connectivity, min_marker_voxels)."""
    if isinstance(radius_mm, (bool, np.bool_)) or not isinstance(radius_mm, (int, float, np.integer, np.floating)):
        raise ValueError("radius_mm must be positive and finite")
    r = _positive(radius_mm, "radius_mm")
    connectivity = _check_connectivity(connectivity)
    tables = _geodesic_tables(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return r, tables, connectivity, _whole_size(min_marker_voxels, "min_marker_voxels")


def separate_components(vol: BitVolume, radius_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                        min_marker_voxels=1) -> Separation:
    """Marker-based separation of touching objects (grains joined by a neck, pore bodies joined by a throat) -> Separation.
    1. markers = offset_volume(vol, -radius_mm, ...): the exact ball erosion, the voxels whose inside distance exceeds
       radius_mm (positive and finite, else ValueError) -- the cores of the objects.
    2. Markers of fewer than min_marker_voxels voxels under `connectivity` are dropped (keep_components).
    3. geodesic_zones grows the markers back through the object; split_zones cuts where two growths meet.
    Separation.volume is a plain BitVolume: volume, box, moments, Euler number, surface, thickness, caliper and geodesic length
    per component apply to the separated objects unchanged (ComponentRuns(sep.volume, connectivity)).  An object thinner than
    the radius everywhere has no marker and stays whole.  A fixed radius over-segments elongated or lobed objects: a grain
    whose erosion falls into two cores is cut in two, and no single radius suits grains of different sizes: separate_by_height
    takes its markers from the h-maxima of the distance map instead.  For another marker rule build the markers yourself and
    hand the map to geodesic_zones and split_zones.  separate_components(cavity_volume(vol), ...) separates pore bodies at
    their throats.  Arguments are checked before the first launch.  separate_with_contacts returns the contact table of the zones as well."""
    args = _separation_args(vol.shape, radius_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels)
    return _separate_by_radius(vol, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x)[0]


def _separate_by_radius(vol: BitVolume, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x):
    r, tables, connectivity, least = args
    return _separate(vol, lambda: offset_volume(vol, -r, slice_depths, mm_per_pixel_y, mm_per_pixel_x), tables, connectivity, least)


def _separate(vol: BitVolume, marker_rule, tables: _GeodesicTables, connectivity, least):
    """The separation itself -> (Separation, the zones' distance map).  marker_rule() -> the marker BitVolume: the one thing in
    which separate_components and separate_by_height differ."""
    _zone_budget(vol.shape)
    COUNTERS["separate_components"] += 1
    markers = marker_rule()
    if least > 1:
        markers = keep_components(markers, least, False, connectivity)
    zone, dist, sweeps, count = _geodesic_zones(vol, ("bits", markers), tables, connectivity)
    out, cleared = _split_zones(vol, zone, connectivity)
    return Separation(out, int(count), int(_download(cleared)[0]), zone, sweeps), dist


# ----------------------------------------------------------------------------- the contact table between zones
CONTACT_TABLE_BUDGET = 1 << 30       # bytes of the slot arrays of zone_contacts' hash table; read when called
CONTACT_SLOT_BYTES = 44              # per slot: key, pairs, first index (8 each), z_lo, z_hi, value, path, row of the slot (4 each)
CONTACT_ENTRY_BYTES = 56             # per slice entry of a row: seven uint64 counters, one per direction class
CONTACT_COLUMNS = 17                 # int64 words per row of tomo_contact_finish
CONTACT_SLOT_LIMIT = 1 << 30         # slots the kernels index


@dataclass
class ZoneContacts:
    """zone_contacts' answer: host arrays, one row per pair of zones in contact, sorted by (zone_a, zone_b)."""
    zone_a: np.ndarray            # int64 (P,): the lower label of the pair
    zone_b: np.ndarray            # int64 (P,): the higher label
    pairs: np.ndarray             # int64 (P,): 26-adjacent voxel pairs across the interface
    pair_counts: np.ndarray       # int64 (P, 7): the same per class x, y, xy, z, xz, yz, xyz
    area_mm2: np.ndarray          # float64 (P,): the Crofton estimate of the interface area
    z_range: np.ndarray           # int64 (P, 2): the lowest and the highest slice of a contact pair (of its raster-earlier voxel)
    first_index: np.ndarray       # int64 (P, 3): (z, y, x) of the first raster-earlier voxel of a contact pair
    value_max: np.ndarray = None  # float32 (P,): the largest of `values` on the interface; None without values
    value_index: np.ndarray = None  # int64 (P, 3): (z, y, x) of the first voxel that attains it
    path_mm: np.ndarray = None    # float32 (P,): the shortest way between the two zones' markers across the interface; None without dist

    def __len__(self):
        return len(self.zone_a)

    def coordination(self, labels=None):
        """-> (labels int64, neighbours int64, area_mm2 float64): per zone the number of distinct zones it touches and its
        summed contact area, the rows added in table order.  labels=None: the zones that occur in the table, ascending.  With
        `labels` (distinct) the answer follows them, a zone without a contact reads 0, and zones not listed are left out."""
        zs = np.concatenate([self.zone_a, self.zone_b]).astype(np.int64)
        areas = np.concatenate([self.area_mm2, self.area_mm2]).astype(np.float64)
        if labels is None:
            labels = np.unique(zs)
        labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        order = np.argsort(labels, kind="stable")
        ranked = labels[order]
        if len(ranked) > 1 and (ranked[1:] == ranked[:-1]).any():
            raise ValueError("labels must be distinct")
        neighbours = np.zeros(len(labels), dtype=np.int64)
        area = np.zeros(len(labels), dtype=np.float64)
        if len(labels) and len(zs):
            pos = np.minimum(np.searchsorted(ranked, zs), len(ranked) - 1)
            known = ranked[pos] == zs
            at = order[pos[known]]
            np.add.at(neighbours, at, 1)
            np.add.at(area, at, areas[known])
        return labels, neighbours, area


def _contact_values(vol: BitVolume, m, what):
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise TypeError("%s must be a float32 tensor (nz, ny, nx)" % what)
    if m.dtype != torch.float32:
        raise TypeError("%s must be float32" % what)
    if tuple(m.shape) != tuple(vol.shape):
        raise ValueError("%s must have the shape of the volume" % what)
    if m.device != vol.device:
        raise ValueError("%s must be on the volume's device" % what)
    return m


def _contact_args(vol: BitVolume, zones, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, directions, values, dist):
    """The argument checks of zone_contacts, all on the host -> (zones, connectivity, F, directions, tables, values, dist)."""
    zones = _zone_map(vol, zones, "zones")
    connectivity = _check_connectivity(connectivity)
    F = surface_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)
    tables = _geodesic_tables(vol.shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return zones, connectivity, F, int(directions), tables, _contact_values(vol, values, "values"), _contact_values(vol, dist, "dist")


def _contact_capacity(pairs: int) -> int:
    """The slots of the hash table for N contact pairs: a power of two, at least 2 N (the zone pairs cannot exceed N), capped by
    CONTACT_TABLE_BUDGET and by what the kernels index."""
    limit = min(int(CONTACT_TABLE_BUDGET) // CONTACT_SLOT_BYTES, CONTACT_SLOT_LIMIT)
    if limit < 1:
        raise _lib.TomoError("zone_contacts: CONTACT_TABLE_BUDGET (%d bytes) does not hold one slot of %d bytes"
                             % (CONTACT_TABLE_BUDGET, CONTACT_SLOT_BYTES))
    cap = 64
    while cap < 2 * pairs and cap < CONTACT_SLOT_LIMIT:
        cap <<= 1
    while cap > limit:
        cap >>= 1
    return cap


def _empty_contacts(values, dist) -> ZoneContacts:
    i, f = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    return ZoneContacts(i, i.copy(), i.copy(), np.zeros((0, SURFACE_CLASSES), dtype=np.int64), np.zeros(0, dtype=np.float64),
                        np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int64), None if values is None else f,
                        None if values is None else np.zeros((0, 3), dtype=np.int64), None if dist is None else f.copy())


def _zone_contacts(vol: BitVolume, args) -> ZoneContacts:
    zones, connectivity, F, directions, tables, values, dist = args
    L, dev, st = _lib.lib(), vol.device, _stream()
    nz, ny, nx = vol.shape
    bits, zones = vol.bits.contiguous(), zones.contiguous()
    values = None if values is None else values.contiguous()
    dist = None if dist is None else dist.contiguous()
    head = (_p(bits), _p(zones), nz, ny, nx)
    COUNTERS["zone_contacts"] += 1
    count = torch.empty(1, dtype=torch.int64, device=dev)
    COUNTERS["contact_launches"] += 1
    _lib.check(L.tomo_contact_count(*head, _p(count), st), "tomo_contact_count")
    pairs = _download(count)[0]
    if pairs == 0:
        return _empty_contacts(values, dist)
    cap = _contact_capacity(pairs)
    keys, total, first = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(3))
    z_lo, z_hi = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    top = None if values is None else torch.empty(cap, dtype=torch.int32, device=dev)
    path = wxy = wz = None
    if dist is not None:
        path = torch.empty(cap, dtype=torch.int32, device=dev)
        wxy, wz = torch.from_numpy(tables.wxy).to(dev), torch.from_numpy(np.ascontiguousarray(tables.wz)).to(dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)          # pairs that found no slot, pairs whose key was not found
    COUNTERS["contact_launches"] += 1
    _lib.check(L.tomo_contact_insert(*head, _p(values), _p(dist), _p(wxy), _p(wz), cap, _p(keys), _p(total), _p(z_lo), _p(z_hi),
                                     _p(first), _p(top), _p(path), _p(counters), st), "tomo_contact_insert")
    # P rows, never voxels: the occupied slots, their keys sorted, the row of every slot, the slice segments of the rows
    taken = keys != 0
    span = (z_hi - z_lo + 1).to(torch.int64) * taken                   # an empty slot counts for nothing
    rows, lost, entries = _download(torch.stack([taken.sum(), counters[0], span.sum()]))          # the one host read
    if lost:
        raise _lib.TomoError("zone_contacts: the hash table of %d slots (CONTACT_TABLE_BUDGET = %d bytes, %d bytes a slot) has no room "
                             "for the zone pairs of %d contact pairs" % (cap, CONTACT_TABLE_BUDGET, CONTACT_SLOT_BYTES, pairs))
    if entries * CONTACT_ENTRY_BYTES > COMPONENT_HIST_BUDGET:
        raise _lib.TomoError("zone_contacts: the per-slice counters of %d zone pairs take %d bytes, more than COMPONENT_HIST_BUDGET (%d)"
                             % (rows, entries * CONTACT_ENTRY_BYTES, COMPONENT_HIST_BUDGET))
    slots = taken.nonzero_static(size=rows).reshape(-1)
    order = keys[slots].sort()[1]                                 # the keys are unique: stability does not matter
    slot_of_row = slots[order].to(torch.int32)
    row_of_slot = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    row_of_slot[slot_of_row.long()] = torch.arange(rows, dtype=torch.int32, device=dev)
    length = span[slot_of_row.long()]
    offset = (length.cumsum(0) - length).contiguous()
    hist = torch.empty(entries * SURFACE_CLASSES, dtype=torch.int64, device=dev)
    where = None if values is None else torch.empty(rows, dtype=torch.int64, device=dev)
    COUNTERS["contact_launches"] += 1
    _lib.check(L.tomo_contact_hist(*head, _p(values), cap, _p(keys), _p(row_of_slot), _p(z_lo), _p(top), _p(offset), rows, _p(hist),
                                   entries, _p(where), _p(counters), st), "tomo_contact_hist")
    tab = torch.from_numpy(F).to(dev)
    out = torch.empty(rows * CONTACT_COLUMNS + 2, dtype=torch.int64, device=dev)
    COUNTERS["contact_launches"] += 1
    _lib.check(L.tomo_contact_finish(rows, _p(slot_of_row), cap, _p(keys), _p(total), _p(z_lo), _p(z_hi), _p(first), _p(top), _p(path),
                                     _p(where), _p(offset), _p(hist), entries, _p(tab), nz, directions, _p(out), _p(counters), st),
               "tomo_contact_finish")
    out[rows * CONTACT_COLUMNS:] = counters
    host = out.cpu().numpy()
    t = host[:rows * CONTACT_COLUMNS].reshape(rows, CONTACT_COLUMNS)
    counts = t[:, 3:10]
    if host[-1] or host[-2] or not np.array_equal(counts.sum(axis=1), t[:, 2]):
        raise _lib.TomoError("zone_contacts: the three passes disagree about the contact pairs (internal error: %d pairs without a "
                             "row)" % int(host[-1]))
    if connectivity == 6:                                              # a contact needs a shared face: x, y or z
        t = t[(counts[:, 0] + counts[:, 1] + counts[:, 3]) > 0]

    def index(flat):
        return np.stack(np.unravel_index(flat, (nz, ny, nx)), axis=1).astype(np.int64).reshape(-1, 3)

    def f32(col):
        return np.ascontiguousarray(t[:, col]).astype(np.uint32).view(np.float32)

    return ZoneContacts(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), np.ascontiguousarray(t[:, 3:10]),
                        np.ascontiguousarray(t[:, 10]).view(np.float64), np.ascontiguousarray(t[:, 11:13]), index(t[:, 13]),
                        None if values is None else f32(14), None if values is None else index(t[:, 15]),
                        None if dist is None else f32(16))


def zone_contacts(vol: BitVolume, zones: torch.Tensor, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=26,
                  directions=13, values=None, dist=None) -> ZoneContacts:
    """The contact table between zones -> ZoneContacts, one row per pair of zones that touch, sorted by (zone_a, zone_b): the
    edges that belong to the nodes a separation yields.  zones: geodesic_zones' map or any int32 device tensor of the volume's
    shape.  A voxel takes part when it is set and its entry is positive.  A contact pair is an unordered pair of 26-adjacent
    voxels that take part and lie in different zones, counted once at its raster-earlier voxel p, in the slice of p and in one
    of surface_area's seven direction classes.  Per zone pair (a, b) = (min, max) of the two labels:
    pairs / pair_counts  the contact pairs, and per class;  z_range the lowest and highest slice;  first_index the first p
    area_mm2     the Crofton estimate of the interface: the sequential float64 sum over the slices in ascending z and the
                 classes in ascending order of count * surface_factors(...)[k][class] -- one adjacent pair of unlike voxels is
                 one crossing of the interface by a lattice line, so the factor is surface_area's (columns 3 .. 6: towards slice
                 k + 1); directions=3 uses x, y and z only.  A flat interface is underestimated as surface_area's flat faces are.
    value_max    with values (a float32 device map, NaN-free): the largest value over the voxels of the zone pair's contact
                 pairs, value_index the first voxel that attains it.  values=distance_transform(vol) gives the throat: the
                 radius of the largest ball centred on the interface that fits in the object.
    path_mm      with dist (geodesic_zones' second result): the minimum over the contact pairs of fl32(fl32(dist(p) + w) +
                 dist(q)), w the float32 step of geodesic_weights -- the shortest way from a marker of one zone to a marker of
                 the other that crosses the interface there; +inf where no pair is finite.
    connectivity does not change what is counted; it says which rows are contacts: 26 every zone pair with a contact pair, 6
    those that share a face (pair_counts of x, y or z positive) -- the rows are filtered after the download and hold the same bytes.
    On the device: tomo_contact_count gives the contact pairs N (none: the empty table, one launch); tomo_contact_insert fills
    an open-addressed hash table of at least 2 N slots, a power of two, within CONTACT_TABLE_BUDGET bytes (44 a slot) -- a table
    that would need more is allocated at the cap, and if it then overflows the call raises TomoError, it never returns a short
    table; the rows are sorted and laid out in torch (P rows, never voxels; one host read); tomo_contact_hist counts per slice
    and class (56 bytes a slice entry; beyond COMPONENT_HIST_BUDGET: TomoError before the allocation); tomo_contact_finish sums.
    Integer atomics only: the same bytes on every run.  Arguments are checked before the first launch; the inputs are left
    untouched.  The pore network of the closed pores is the same call on the zones of cavity_volume(vol)."""
    return _zone_contacts(vol, _contact_args(vol, zones, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, directions,
                                             values, dist))


def separate_with_contacts(vol: BitVolume, radius_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                           min_marker_voxels=1, directions=13):
    """separate_components and the contact table of its zones -> (Separation, ZoneContacts): the separation as
    separate_components makes it, then zone_contacts of the zones the call already holds under the same spacing and
    connectivity, with values=distance_transform(vol, ...) -- value_max is the throat radius -- and dist = the zones' distance
    map, so path_mm is the way from core to core.  separate_with_contacts(cavity_volume(vol), ...) is the pore network of the
    closed pores: pore bodies, throats and the ways between them."""
    args = _separation_args(vol.shape, radius_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels)
    surface_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)          # the argument check
    sep, dist = _separate_by_radius(vol, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return sep, _separation_contacts(vol, sep, dist, slice_depths, mm_per_pixel_y, mm_per_pixel_x, args[2], directions)


def _separation_contacts(vol: BitVolume, sep: Separation, dist, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, directions):
    """The contact table of a separation's zones: the throat from the inside distance, the way from the zones' distance map."""
    inside = distance_transform(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return _zone_contacts(vol, _contact_args(vol, sep.zones, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, directions,
                                             inside, dist))


# ----------------------------------------------------------------------------- grey reconstruction, h-maxima, separation by height
RECON_F_NAN = 8                      # counters[1] of tomo_recon_seed: NaN on a set voxel
RECON_F_WORK = 16                    # ... some set voxel starts below its ceiling: without it the seeded map is final


def _recon_map(vol: BitVolume, m, what) -> torch.Tensor:
    if m is None:
        raise TypeError("%s must be a float32 tensor (nz, ny, nx)" % what)
    return _contact_values(vol, m, what)


def _recon_height(h, what="h") -> float:
    """h as the device subtracts it: rounded once to float32, positive and finite there."""
    if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be positive and finite" % what)
    with np.errstate(over="ignore"):
        h32 = np.float32(h)
    if not (np.isfinite(h32) and h32 > 0):
        raise ValueError("%s must be positive and finite as a float32" % what)
    return float(h32)


def _recon_budget(shape, maps, what):
    """Before anything is allocated: the call holds `maps` float32 maps at once, the caller's included."""
    nz, ny, nx = shape
    nbytes = 4 * maps * nz * ny * nx
    if nbytes > GEODESIC_VOLUME_BUDGET:
        raise _lib.TomoError("%s: %d float32 maps of %d x %d x %d voxels take %d bytes, more than GEODESIC_VOLUME_BUDGET (%d)"
                             % (what, maps, nz, ny, nx, nbytes, GEODESIC_VOLUME_BUDGET))


def _reconstruct(vol: BitVolume, mask: torch.Tensor, marker, mode, h, connectivity, what) -> torch.Tensor:
    """Seed and sweep -> g.  mode: tomo_recon_seed's (0 the marker map, 1 mask - h, 2 the float just below the mask)."""
    L, st = _lib.lib(), _stream()
    nz, ny, nx = vol.shape
    plan = _GeodesicPlan(vol, None, connectivity)
    COUNTERS["recon_calls"] += 1
    mask = mask.contiguous()
    marker = None if marker is None else marker.contiguous()
    g = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    _lib.check(L.tomo_recon_seed(_p(plan.bits), _p(mask), _p(marker), mode, h, nz, ny, nx, _p(g), _p(plan.counters), st), "tomo_recon_seed")
    flags = int(_download(plan.counters)[1])
    if flags & RECON_F_NAN:
        raise ValueError("%s: NaN on a set voxel" % what)
    if flags & RECON_F_WORK:                                             # an empty volume, or a marker at the ceiling everywhere: no sweep
        plan.propagate_reconstruction(mask, g)
    return g


def reconstruct(vol: BitVolume, mask: torch.Tensor, marker: torch.Tensor, connectivity=26) -> torch.Tensor:
    """Greyscale morphological reconstruction by dilation of `marker` under `mask` inside the set voxels of a resident volume ->
    float32 (nz, ny, nx) device tensor g: the least fixed point above m' = min(marker, mask) of
        g(p) = max(m'(p), min(mask(p), max over the set neighbours q of g(q))),
    neighbours under `connectivity` (6 or 26 between two SET voxels, label_components' adjacency).  Every dome of the mask that
    holds no marker value of its own is cut down to the level at which it is reached from outside.  mask, marker: float32 device
    tensors of the volume's shape; unset voxels take no part -- their entries are not read, NaN included -- and g holds 0.0
    there.  Values are ordered as float32 orders them, -0.0 counts as +0.0 and comes back as +0.0; NaN on a set voxel: ValueError.
    On the device: tomo_recon_seed writes m', then tomo_recon_sweep raises 8 x 8 x 64 tiles in LDS, sweep after sweep, in
    geodesic_distance's host loop (GEODESIC_SWEEP_BATCH sweeps between two counter reads, more than GEODESIC_SWEEP_LIMIT:
    TomoError).  The operator takes minima and maxima only, so it is monotone and every order of tiles ends at the same bytes.
    A plateau needs one sweep per tile it crosses.  The call holds three maps (mask, marker, g); more than
    GEODESIC_VOLUME_BUDGET bytes: TomoError before anything is allocated.  An empty volume, or a marker that is nowhere below
    the mask, launches no sweep.  Arguments are checked before the first launch; the inputs are left untouched."""
    connectivity = _check_connectivity(connectivity)
    mask, marker = _recon_map(vol, mask, "mask"), _recon_map(vol, marker, "marker")
    _recon_budget(vol.shape, 3, "reconstruct")
    return _reconstruct(vol, mask, marker, 0, 0.0, connectivity, "reconstruct")


def h_maxima(vol: BitVolume, values: torch.Tensor, h, connectivity=26) -> torch.Tensor:
    """The h-maxima transform HMAX_h(values) = reconstruct(vol, values, fl32(values - h)) -> float32 device tensor: every dome of
    the map is cut down by h, or to its saddle when it stands less than h above it.  h: positive and finite as a float32 (else
    ValueError); the subtraction is one float32 operation per voxel, made by the seeding pass, so no marker map is allocated:
    the call holds two maps."""
    connectivity = _check_connectivity(connectivity)
    values, h = _recon_map(vol, values, "values"), _recon_height(h)
    _recon_budget(vol.shape, 2, "h_maxima")
    return _reconstruct(vol, values, None, 1, h, connectivity, "h_maxima")


def _regional_maxima(vol: BitVolume, values: torch.Tensor, connectivity, what) -> BitVolume:
    values = values.contiguous()
    g = _reconstruct(vol, values, None, 2, 0.0, connectivity, what)
    bits = vol.bits.contiguous()
    out = torch.empty_like(bits)
    _lib.check(_lib.lib().tomo_recon_below(_p(bits), _p(values), _p(g), *vol.shape, _p(out), _stream()), "tomo_recon_below")
    return BitVolume(out, vol.shape)


def regional_maxima(vol: BitVolume, values: torch.Tensor, connectivity=26) -> BitVolume:
    """The regional maxima of a float32 map inside the set voxels -> a NEW BitVolume: the plateaus -- connected sets of equal
    values under `connectivity` -- with no higher set neighbour.  Computed as the set voxels with reconstruct(values, the float
    just below values) < values: a plateau with a higher neighbour is filled back to its own value, a maximum stays one float
    below.  A plateau at -inf has nothing below it and is not reported.  The call holds two maps (8 bytes a voxel against
    GEODESIC_VOLUME_BUDGET)."""
    connectivity = _check_connectivity(connectivity)
    values = _recon_map(vol, values, "values")
    _recon_budget(vol.shape, 2, "regional_maxima")
    return _regional_maxima(vol, values, connectivity, "regional_maxima")


def extended_maxima(vol: BitVolume, values: torch.Tensor, h, connectivity=26) -> BitVolume:
    """EMAX_h(values) = regional_maxima(h_maxima(values, h)) -> a NEW BitVolume: one connected marker on every dome of the map
    that stands at least h above its saddle (MorphoLibJ's extended maxima).  On a distance map the markers of grains of any
    size, while surface roughness below h makes none.  The call holds the caller's map and two more (12 bytes a voxel against
    GEODESIC_VOLUME_BUDGET, checked before anything is allocated); the h-maxima map is freed before the call returns."""
    connectivity = _check_connectivity(connectivity)
    values, h = _recon_map(vol, values, "values"), _recon_height(h)
    _recon_budget(vol.shape, 3, "extended_maxima")
    domes = _reconstruct(vol, values, None, 1, h, connectivity, "extended_maxima")
    out = _regional_maxima(vol, domes, connectivity, "extended_maxima")
    del domes
    return out


def _height_args(shape, h_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm):
    """The argument checks of separate_by_height, all on the host -> (h, tables, connectivity, min_marker_voxels, min_radius)."""
    h = _recon_height(h_mm, "h_mm")
    connectivity = _check_connectivity(connectivity)
    tables = _geodesic_tables(shape, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    least = _whole_size(min_marker_voxels, "min_marker_voxels")
    if isinstance(min_radius_mm, (bool, np.bool_)) or not isinstance(min_radius_mm, (int, float, np.integer, np.floating)) or \
            not (math.isfinite(min_radius_mm) and min_radius_mm >= 0):
        raise ValueError("min_radius_mm must be non-negative and finite")
    return h, tables, connectivity, least, float(min_radius_mm)


def _separate_by_height(vol: BitVolume, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x):
    h, tables, connectivity, least, least_radius = args
    spacing = (slice_depths, mm_per_pixel_y, mm_per_pixel_x)

    def markers():
        domes = extended_maxima(vol, distance_transform(vol, *spacing), h, connectivity)
        if least_radius > 0:                                             # domes of thin debris go
            domes = BitVolume(domes.bits & offset_volume(vol, -least_radius, *spacing).bits, vol.shape)
        return domes
    return _separate(vol, markers, tables, connectivity, least)


def separate_by_height(vol: BitVolume, h_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                       min_marker_voxels=1, min_radius_mm=0.0) -> Separation:
    """separate_components with h-maxima markers -> Separation: the markers are extended_maxima(vol, distance_transform(vol,
    ...), h_mm, connectivity) -- one marker on every dome of the inside distance that stands at least h_mm above its saddle,
    the rule of MorphoLibJ's distance-transform watershed.  A large and a small pair of touching grains are split by the same
    h_mm, where no single erosion radius finds both, and roughness below h_mm makes no marker.  min_radius_mm > 0: the markers
    are ANDed with offset_volume(vol, -min_radius_mm, ...), so the domes of debris thinner than that go.  Markers of fewer than
    min_marker_voxels voxels are dropped; zones and cut are separate_components'.  h_mm must be positive and finite as a
    float32, min_radius_mm non-negative and finite (ValueError).  While the markers are made the call holds three float32 maps
    (the distance, its h-maxima, the reconstruction), freed before the zones take their three.  Arguments are checked before
    the first launch.  separate_by_height_with_contacts returns the contact table as well."""
    args = _height_args(vol.shape, h_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm)
    return _separate_by_height(vol, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x)[0]


def separate_by_height_with_contacts(vol: BitVolume, h_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, connectivity=6,
                                     min_marker_voxels=1, min_radius_mm=0.0, directions=13):
    """separate_by_height and the contact table of its zones -> (Separation, ZoneContacts), as separate_with_contacts returns
    them for the fixed radius: value_max is the throat radius, path_mm the way from marker to marker."""
    args = _height_args(vol.shape, h_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm)
    surface_factors(slice_depths, vol.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)          # the argument check
    sep, dist = _separate_by_height(vol, args, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    return sep, _separation_contacts(vol, sep, dist, slice_depths, mm_per_pixel_y, mm_per_pixel_x, args[2], directions)


# ----------------------------------------------------------------------------- homotopic thinning: the curve skeleton
THIN_SUBPASSES = 48                  # sub-passes of one iteration: six directions, eight subfields each (tomo_thin_pass)
THIN_COUNTER_WORDS = 1024            # tomo_thin_pass spreads its count of cleared voxels over 64 counters, 128 bytes apart
THIN_ITERATION_BATCH = 1             # iterations, each of 48 launches, enqueued between two reads of the counters; read when called
THIN_ITERATION_LIMIT = 1 << 16       # a guard against an endless host loop, no tuning knob; read when called


def _skeleton_args(vol, curve, connectivity, anchors):
    """The argument checks of the thinning calls, all on the host -> (curve, anchors)."""
    if not isinstance(vol, BitVolume):
        raise TypeError("vol must be a BitVolume")
    connectivity = _check_connectivity(connectivity)
    curve = bool(curve)
    if curve and connectivity == 6:
        raise ValueError("curve=True needs connectivity 26: the end rule counts 26-neighbours and would eat a 6-connected staircase "
                         "from its end (curve=False thins under 6)")
    if anchors is not None:
        if not isinstance(anchors, BitVolume):
            raise TypeError("anchors must be a BitVolume or None")
        if tuple(anchors.shape) != tuple(vol.shape) or tuple(anchors.bits.shape) != tuple(vol.bits.shape):
            raise ValueError("anchors must have the shape of the volume")
        if anchors.device != vol.device:
            raise ValueError("anchors must be on the volume's device")
    return curve, anchors


def _skeleton(vol: BitVolume, curve, connectivity, anchors):
    """Thin a copy of the volume -> (BitVolume, iterations).  Iterations of 48 sub-passes, THIN_ITERATION_BATCH of them between
    two reads; every iteration has a counter row of its own, so the first one that cleared nothing is known whatever the batch."""
    L, dev, st = _lib.lib(), vol.device, _stream()
    nz, ny, nx = vol.shape
    src = vol.bits.contiguous()
    bits = torch.empty_like(src)
    bits.copy_(src)
    out = BitVolume(bits, (nz, ny, nx))
    COUNTERS["thin_calls"] += 1
    if _download(popcount_async(out))[0] == 0:                           # nothing to thin: no sub-pass is launched
        return out, 0
    tiles = int(L.tomo_geo_tiles(nz, ny, nx))
    if tiles <= 0:
        raise _lib.TomoError("tomo_geo_tiles failed (%d)" % tiles)
    keep = None if anchors is None else anchors.bits.contiguous()
    limit, batch = int(THIN_ITERATION_LIMIT), max(1, int(THIN_ITERATION_BATCH))
    stamp = torch.zeros(tiles, dtype=torch.int32, device=dev)
    counters = torch.zeros((batch, THIN_COUNTER_WORDS), dtype=torch.int64, device=dev)
    done = 0
    while True:
        if done >= limit:
            raise _lib.TomoError("skeleton: no fixed point after %d iterations (THIN_ITERATION_LIMIT)" % done)
        k = min(batch, limit - done)
        if done:
            counters.zero_()
        for j in range(k):
            row = _p(counters[j])
            for d in range(6):
                for s in range(8):
                    tick = THIN_SUBPASSES * (done + j) + 8 * d + s + 1
                    _lib.check(L.tomo_thin_pass(_p(bits), _p(keep), nz, ny, nx, connectivity, int(curve), d, s, _p(stamp), tick, row, st),
                               "tomo_thin_pass")
        COUNTERS["thin_passes"] += THIN_SUBPASSES * k
        host = _download(counters.sum(dim=1))
        for j in range(k):
            if host[j] == 0:                                             # the first iteration that cleared nothing: the fixed point
                COUNTERS["thin_iterations"] += done + j + 1
                return out, done + j + 1
        done += k


def skeleton(vol: BitVolume, curve=True, connectivity=26, anchors=None) -> BitVolume:
    """The skeleton of a resident volume by homotopic thinning -> a NEW BitVolume; the input is left untouched (MorphoLibJ /
    BoneJ Skeletonize3D, scikit-image skeletonize_3d answer the same question with another order of deletions).  One definition
    (include/tomo_hip.h): an iteration is 48 sub-passes -- the directions -z, +z, -y, +y, -x, +x, inside each the eight
    subfields 4 (z & 1) + 2 (y & 1) + (x & 1) in ascending order -- and a sub-pass clears, all at once, every set voxel of its
    subfield whose neighbour in its direction is clear or outside the stack, that is a simple point under `connectivity` (26,
    or 6; the background has the other one, outside the stack is background) and, with curve=True, is no end (exactly one set
    26-neighbour).  The result is the volume after the first iteration that cleared nothing.  Two voxels of one subfield are
    never 26-neighbours, so every deletion is the deletion of a simple point: components, cavities and handles are those of
    the input.  curve=False gives the ultimate homotopic kernel (a ball becomes one voxel, a ring a closed curve, a shell stays
    a closed surface); curve=True the curve skeleton; curve=True with connectivity 6 is a ValueError.  anchors: a BitVolume of
    voxels that are never cleared (extended_maxima of the distance map pins the skeleton to the domes), or None.
    The thinning is in voxel steps: spacing and slice depths play no part in it.
    On the device: tomo_thin_pass in place on a copy -- a candidate only reads bits no sub-pass of its kind writes, so there is
    no second buffer, and the bytes are the same on every run -- with one uint32 per 8 x 8 x 64 tile that lets a tile rest once
    it and its neighbours lost nothing for 48 sub-passes.  Memory: the copy and 4 bytes a tile, nothing per voxel.  The host
    enqueues THIN_ITERATION_BATCH iterations between two counter reads (more than THIN_ITERATION_LIMIT iterations: TomoError);
    the bytes and the iteration count do not depend on the batch.  COUNTERS: thin_calls, thin_iterations (the last, idle one
    included), thin_passes.  An empty volume launches no sub-pass (0 iterations).  Arguments are checked
    before the first launch."""
    curve, anchors = _skeleton_args(vol, curve, connectivity, anchors)
    return _skeleton(vol, curve, int(connectivity), anchors)[0]


@dataclass
class SkeletonNodes:
    """skeleton_nodes' answer: two bit volumes on the device and four counts."""
    ends: BitVolume              # the set voxels with exactly one set 26-neighbour
    junctions: BitVolume         # ... with three or more
    voxels: int
    end_points: int
    junction_voxels: int
    isolated: int                # set voxels without a set 26-neighbour


def _skeleton_nodes(skel: BitVolume) -> SkeletonNodes:
    L, dev = _lib.lib(), skel.device
    bits = skel.bits.contiguous()
    ends, junctions = torch.empty_like(bits), torch.empty_like(bits)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    COUNTERS["thin_nodes"] += 1
    _lib.check(L.tomo_thin_nodes(_p(bits), *skel.shape, _p(ends), _p(junctions), _p(counters), _stream()), "tomo_thin_nodes")
    return SkeletonNodes(BitVolume(ends, skel.shape), BitVolume(junctions, skel.shape), *_download(counters))


def skeleton_nodes(skel: BitVolume) -> SkeletonNodes:
    """The free ends and the junctions of a skeleton (or of any volume) by 26-neighbour counts -> SkeletonNodes: a set voxel with
    exactly one set neighbour is an end, one with three or more a junction voxel, one with none is isolated.  A junction of a
    one-voxel curve is a small cluster of junction voxels, not one: junction_voxels counts voxels.  One pass, one host read."""
    if not isinstance(skel, BitVolume):
        raise TypeError("skel must be a BitVolume")
    return _skeleton_nodes(skel)


@dataclass
class ComponentSkeleton:
    """component_skeleton's answer: host arrays, one row per selected component in ascending label."""
    labels: np.ndarray           # int64 (m,)
    voxels: np.ndarray           # int64 (m,)
    skeleton_voxels: np.ndarray  # int64 (m,): the voxels of the component's piece of the skeleton
    end_points: np.ndarray       # int64 (m,): its free ends
    junction_voxels: np.ndarray  # int64 (m,): its junction voxels

    def __len__(self):
        return len(self.labels)


def _component_skeleton_from(ride, rows) -> ComponentSkeleton:
    ride = np.ascontiguousarray(ride, dtype=np.int64).reshape(-1, 2)
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 3)
    return ComponentSkeleton(ride[:, 0].copy(), ride[:, 1].copy(), rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy())


def component_skeleton(vol: BitVolume, connectivity=26, min_voxels=0, largest=False, curve=True, anchors=None) -> ComponentSkeleton:
    """Skeleton voxels, free ends and junction voxels per component of a resident volume -> ComponentSkeleton, one row per
    component the keep rule of component_properties selects, in ascending label: the rows component_properties returns for the
    same rule.  The volume is labelled under `connectivity` and thinned under the same connectivity (skeleton's arguments and
    errors: curve=True needs 26).  Thinning preserves components, so every component owns exactly one piece of the skeleton,
    and the counts are taken under the ORIGINAL runs of the labelling.  A fibre reads two ends and no junction, a ring none of
    either, a branching crack its branch points.  An empty volume, or nothing selected, gives zero rows.  Arguments are
    checked before the first launch."""
    _skeleton_args(vol, curve, connectivity, anchors)
    _keep_rule(min_voxels, largest)
    return ComponentRuns(vol, connectivity).skeleton(min_voxels, largest, curve, anchors)


def cavity_skeleton(vol: BitVolume, connectivity=6, min_voxels=0, max_voxels=None, curve=True, anchors=None) -> ComponentSkeleton:
    """component_skeleton of the enclosed voids of a resident volume, one row per cavity of cavity_table under the same size
    window, in ascending cavity label.  The complement is labelled and thinned under the complementary connectivity: the
    default connectivity=6 of the solid gives 26-connected pores, which curve=True needs."""
    connectivity = _check_connectivity(connectivity)
    lo, hi = _check_size_window(min_voxels, max_voxels)
    _skeleton_args(vol, curve, 32 - connectivity, anchors)
    return _complement_runs(vol, connectivity).skeleton(lo, False, curve, anchors, max_voxels=hi, enclosed=True)


# ----------------------------------------------------------------------------- the branch table of a skeleton
def branch_steps(slice_depths, nz, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0) -> np.ndarray:
    """The length in mm of one step per slice and column of tomo_branch_hist, on the host -> float64 (nz, 11): columns 0 .. 2 the
    steps x, y, xy in the slice, 3 .. 6 the steps z, xz, yz, xyz towards slice k + 1, 7 .. 10 the same towards k - 1.  An entry is
    sqrt(((dx mm_x)^2 + (dy mm_y)^2) + dzc^2) in float64 with dzc = zc[k + 1] - zc[k] upward, zc[k] - zc[k - 1] downward (zc: the
    slice centres of distance_positions) and 0.0 where that slice does not exist -- no voxel steps there.  Rounded to float32,
    the entries are geodesic_weights'.  slice_depths=None: depth 1.0 per slice."""
    zt, _, _ = distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)        # the argument checks
    zc = zt[1:-1]
    nz = len(zc)
    mm_y, mm_x = float(mm_per_pixel_y), float(mm_per_pixel_x)
    up, down = np.zeros(nz), np.zeros(nz)
    up[:-1] = zc[1:] - zc[:-1]
    down[1:] = zc[1:] - zc[:-1]
    out = np.empty((nz, SURFACE_COUNTERS), dtype=np.float64)
    for cls, (az, ay, ax) in enumerate(_SURFACE_CLASS_STEPS):
        plane = (ax * mm_x) * (ax * mm_x) + (ay * mm_y) * (ay * mm_y)
        if az == 0:
            out[:, cls] = np.sqrt(plane + 0.0 * 0.0)
        else:
            out[:, cls] = np.sqrt(plane + up * up)
            out[:, cls + 4] = np.sqrt(plane + down * down)
    return out


@dataclass
class SkeletonBranchRows:
    """The branches of skeleton_branches: host arrays, one row per selected branch in ascending label."""
    label: np.ndarray            # int64 (m,): the label of the branch in ComponentRuns(regular, 26)
    voxels: np.ndarray           # int64 (m,)
    length_mm: np.ndarray        # float64 (m,): the two attaching steps included
    step_counts: np.ndarray      # int64 (m, 7): the edges per class x, y, xy, z, xz, yz, xyz
    attach_index: np.ndarray     # int64 (m, 2): the flat indices of the attached node voxels, lo <= hi; -1, -1 for a cycle
    nodes: np.ndarray            # int64 (m, 2): the labels of those voxels' nodes; 0, 0 for a cycle
    chord_mm: np.ndarray         # float64 (m,): the distance between the two attached voxels; nan for a cycle
    tortuosity: np.ndarray       # float64 (m,): length / chord; inf where the chord is 0, nan for a cycle
    kind: np.ndarray             # int64 (m,): 0 closed cycle, 1 both nodes free ends, 2 exactly one (a spur), 3 neither

    def __len__(self):
        return len(self.label)


@dataclass
class SkeletonNodeRows:
    """The nodes of skeleton_branches: host arrays, one row per node in ascending label."""
    label: np.ndarray            # int64 (n,): the label of the node in ComponentRuns(node_voxels, 26)
    voxels: np.ndarray           # int64 (n,)
    end_voxels: np.ndarray       # int64 (n,): its voxels with at most one set neighbour
    junction_voxels: np.ndarray  # int64 (n,): ... with three or more
    branches: np.ndarray         # int64 (n,): the attachments of the selected branches, with multiplicity
    index_box: np.ndarray        # int64 (n, 6): zmin, zmax, ymin, ymax, xmin, xmax, inclusive
    centroid_index: np.ndarray   # float64 (n, 3)
    centroid_mm: np.ndarray      # float64 (n, 3): component_properties' centroid
    free_end: np.ndarray         # bool (n,): one voxel, and that voxel has exactly one set neighbour

    def __len__(self):
        return len(self.label)


@dataclass
class SkeletonBranches:
    """skeleton_branches' answer."""
    branches: SkeletonBranchRows
    nodes: SkeletonNodeRows
    regular: BitVolume           # on the device: the set voxels with exactly two set 26-neighbours
    node_voxels: BitVolume       # ... and all the others
    voxels: int
    regular_voxels: int
    node_voxel_count: int
    isolated: int


@dataclass
class PrunedSkeleton:
    """prune_skeleton's answer."""
    volume: BitVolume            # a NEW volume
    removed_branches: int
    removed_voxels: int          # the voxels of those branches and the free ends they hung from
    rounds: int                  # the rounds that removed something


def _branch_args(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x, min_voxels=0):
    """The argument checks of the branch calls, all on the host -> (steps, zc, mm_y, mm_x, min_voxels)."""
    if not isinstance(skel, BitVolume):
        raise TypeError("skel must be a BitVolume")
    steps = branch_steps(slice_depths, skel.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    zt, _, _ = distance_positions(slice_depths, skel.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    return steps, zt[1:-1].copy(), float(mm_per_pixel_y), float(mm_per_pixel_x), _whole_size(min_voxels, "min_voxels")


def _branch_rows_from(shape, zc, mm_y, mm_x, voxels, labels, length, counts, attach, count, node_of, free_end) -> SkeletonBranchRows:
    """Host arithmetic on the downloaded rows.  chord_mm = sqrt(((dx)^2 + (dy)^2) + dz^2) between the two attached voxels at
    (zc[k], j * mm_y, i * mm_x)."""
    nz, ny, nx = shape
    m = len(labels)
    cycle = count == 0
    at = np.where(attach < 0, 0, attach)
    k, rest = at // (ny * nx), at % (ny * nx)
    pz, py, px = zc[k] if m else np.zeros((0, 2)), (rest // nx) * mm_y, (rest % nx) * mm_x
    dz, dy, dx = pz[:, 1] - pz[:, 0], py[:, 1] - py[:, 0], px[:, 1] - px[:, 0]
    chord = np.where(cycle, np.nan, np.sqrt((dx * dx + dy * dy) + dz * dz))
    with np.errstate(divide="ignore", invalid="ignore"):
        tortuosity = np.where(cycle, np.nan, np.where(chord == 0, np.inf, length / chord))
    free = np.concatenate([[False], free_end])[node_of].reshape(m, 2)
    kind = np.where(cycle, 0, 3 - free.sum(axis=1)).astype(np.int64)
    return SkeletonBranchRows(labels, voxels, length, counts, attach, node_of, chord, tortuosity, kind)


def _empty_branch_rows() -> SkeletonBranchRows:
    i, f = (lambda *s: np.zeros(s, dtype=np.int64)), (lambda *s: np.zeros(s, dtype=np.float64))
    return SkeletonBranchRows(i(0), i(0), f(0), i(0, SURFACE_CLASSES), i(0, 2), i(0, 2), f(0), f(0), i(0))


def _empty_node_rows() -> SkeletonNodeRows:
    i, f = (lambda *s: np.zeros(s, dtype=np.int64)), (lambda *s: np.zeros(s, dtype=np.float64))
    return SkeletonNodeRows(i(0), i(0), i(0), i(0), i(0), i(0, 6), f(0, 3), f(0, 3), np.zeros(0, dtype=bool))


def _skeleton_branches(skel: BitVolume, args, slice_depths):
    """-> (SkeletonBranches, the ComponentRuns of R or None, the ComponentRuns of N or None)."""
    steps, zc, mm_y, mm_x, min_voxels = args
    L, dev = _lib.lib(), skel.device
    bits = skel.bits.contiguous()
    whole = BitVolume(bits, skel.shape)
    regular, node_voxels = BitVolume(torch.empty_like(bits), skel.shape), BitVolume(torch.empty_like(bits), skel.shape)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    COUNTERS["skeleton_branches"] += 1
    COUNTERS["branch_split"] += 1
    _lib.check(L.tomo_branch_split(_p(bits), *skel.shape, _p(regular.bits), _p(node_voxels.bits), _p(counters), _stream()),
               "tomo_branch_split")
    voxels, regular_voxels, node_count, isolated = (int(v) for v in _download(counters))
    branches, nodes, runs_r, runs_n, rows = _empty_branch_rows(), _empty_node_rows(), None, None, None
    if regular_voxels:                                                  # the branches: a labelling of R, the steps, the attachments
        runs_r = ComponentRuns(regular, 26)
        rows = runs_r.branch_rows(steps, whole, min_voxels)
    if node_count:                                                      # the nodes: a labelling of N, its table, its ends and junctions
        runs_n = ComponentRuns(node_voxels, 26)
        p = runs_n.properties(_slice_weights(slice_depths, skel.shape[0], mm_y, mm_x), mm_y, mm_x)
        picked = runs_n.select()
        marks = _skeleton_nodes(whole)
        kinds = torch.zeros((picked.m, 2), dtype=torch.int64, device=dev)
        for column, other in enumerate((marks.ends, marks.junctions)):
            _lib.check(L.tomo_thin_count(_p(runs_n.bits), *skel.shape, *runs_n._tables(), _p(runs_n.tot), _p(other.bits), _p(picked.sel),
                                         _p(picked.slot), _p(kinds), column, 2, picked.table.shape[0], picked.m, _stream()),
                       "tomo_thin_count")
        (kinds,) = runs_n._download_checked("skeleton_branches", kinds)
        ends, junctions = kinds[:, 0].copy(), kinds[:, 1].copy()
        nodes = SkeletonNodeRows(p.labels, p.voxels, p.voxels - junctions, junctions, np.zeros(len(p), dtype=np.int64), p.index_box,
                                 p.centroid_index, p.centroid_mm, (p.voxels == 1) & (ends == 1))
    if rows is not None:                                                # which nodes the attached voxels lie in
        vox, labels, length, counts, attach, count = rows
        node_of = np.zeros((len(labels), 2), dtype=np.int64)
        if len(labels) and runs_n is not None:
            node_of = runs_n.label_at(torch.from_numpy(attach).to(dev)).cpu().numpy()
            runs_n._checked()
        branches = _branch_rows_from(skel.shape, zc, mm_y, mm_x, vox, labels, length, counts, attach, count, node_of, nodes.free_end)
        nodes.branches = np.bincount(node_of[count > 0].reshape(-1), minlength=len(nodes) + 1)[1:].astype(np.int64)
    return SkeletonBranches(branches, nodes, regular, node_voxels, voxels, regular_voxels, node_count, isolated), runs_r, runs_n


def skeleton_branches(skel: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, min_voxels=0) -> SkeletonBranches:
    """The branch table of a skeleton (or of any volume: nothing assumes thinness) -> SkeletonBranches: how many branches it has,
    how long each is in mm under the real slice depths, which nodes it joins and how tortuous it is (AnalyzeSkeleton of BoneJ /
    MorphoLibJ and skan answer the same question).  One definition (include/tomo_hip.h): under the 26-adjacency a set voxel
    with exactly two set neighbours is REGULAR, every other one a NODE voxel; a branch is a component of the regular voxels -- a
    path or a closed cycle --, a node a component of the node voxels (an end next to a junction belongs to the junction's node,
    two voxels are one node without a branch), a free end a one-voxel node with one neighbour.  A path is attached to node
    voxels by exactly two edges.  length_mm adds up every edge with an end in the branch, the two attaching steps included:
    the sequential float64 sum, slice by slice and column by column, of count * branch_steps(...).  kind: 0 a closed cycle, 1
    both nodes are free ends (a plain fibre), 2 exactly one is (a terminal branch, a spur), 3 neither.  min_voxels: only the
    branches of at least that many voxels get a row; nodes.branches then counts the attachments of those.
    On the device: tomo_branch_split, one ComponentRuns for the regular and one for the node voxels, tomo_branch_hist behind the
    driver of the per-component measurements (88 bytes per slice of the box of every selected branch; beyond
    COMPONENT_HIST_BUDGET bytes for more than one branch: its TomoError) with tomo_cc_surface adding up, tomo_branch_attach,
    and tomo_branch_lookup for the nodes of the attached voxels; the nodes' ends and junctions come from tomo_thin_nodes under
    the node tables (tomo_thin_count).  Memory scales with the runs, the branches and their slices, never with the voxels.
    An empty volume launches nothing past the split; one without regular voxels labels its nodes and returns zero branch rows.
    Arguments are checked before the first launch."""
    args = _branch_args(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x, min_voxels)
    return _skeleton_branches(skel, args, slice_depths)[0]


PRUNE_ROUND_LIMIT = 1 << 16          # a guard against an endless host loop, no tuning knob; read when called


def _check_rounds(rounds):
    if rounds is None:
        return None
    if isinstance(rounds, (bool, np.bool_)) or not isinstance(rounds, (int, np.integer)) or rounds < 0:
        raise ValueError("rounds must be a non-negative whole number or None")
    return int(rounds)


def _prune(skel: BitVolume, args, slice_depths, rounds, rule, what) -> PrunedSkeleton:
    """The rounds of pruning.  rule(t) -> bool (m,) over the rows of t.branches, the table of the volume as it stands: the
    branches that go (only kind 2 may be named); each goes with the free-end voxel it hangs from."""
    dev = skel.device
    vol = BitVolume(skel.bits.contiguous().clone(), skel.shape)
    removed_branches = removed_voxels = done = 0
    while rounds is None or done < rounds:
        if done >= int(PRUNE_ROUND_LIMIT):
            raise _lib.TomoError("%s: no fixed point after %d rounds (PRUNE_ROUND_LIMIT)" % (what, done))
        t, runs_r, runs_n = _skeleton_branches(vol, args, slice_depths)
        b = t.branches
        gone = rule(t)
        if not gone.any():
            break
        COUNTERS["prune_rounds"] += 1
        flags_r = np.zeros(runs_r.n, dtype=np.uint8)
        flags_r[b.label[gone] - 1] = 1
        ends = b.nodes[gone]
        ends = ends[np.concatenate([[False], t.nodes.free_end])[ends]]   # of the two nodes of a spur the free end
        flags_n = np.zeros(runs_n.n, dtype=np.uint8)
        flags_n[ends - 1] = 1
        vol = runs_n.clear(torch.from_numpy(flags_n).to(dev), runs_r.clear(torch.from_numpy(flags_r).to(dev), vol))
        removed_branches += int(gone.sum())
        removed_voxels += int(b.voxels[gone].sum()) + len(ends)
        done += 1
    return PrunedSkeleton(vol, removed_branches, removed_voxels, done)


def prune_skeleton(skel: BitVolume, min_length_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, rounds=1) -> PrunedSkeleton:
    """Remove the short terminal branches of a skeleton -> PrunedSkeleton with a NEW volume; the input is left untouched.  One
    round removes every branch of kind 2 of skeleton_branches -- exactly one of its nodes is a free end -- with length_mm <
    min_length_mm, together with the free-end voxel it hangs from; the node at its other end stays.  A pendant path is a chain
    of simple-point deletions, so components, cavities and handles are the input's.  rounds=None repeats the round on the
    table of the pruned volume until one removes nothing (a round only merges branches into longer ones, so this ends;
    PRUNE_ROUND_LIMIT guards the loop with a TomoError).  Plain fibres (kind 1) and cycles are never touched.  On the device a round is
    skeleton_branches and two tomo_branch_clear: the tables of the regular voxels with the flags of the branches, then the
    tables of the node voxels with the flags of their free ends.  Arguments are checked before the first launch."""
    args = _branch_args(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    min_length_mm = float(min_length_mm)
    if math.isnan(min_length_mm):
        raise ValueError("min_length_mm must be a number")
    rounds = _check_rounds(rounds)
    return _prune(skel, args, slice_depths, rounds, lambda t: (t.branches.kind == 2) & (t.branches.length_mm < min_length_mm),
                  "prune_skeleton")


# ----------------------------------------------------------------------------- a value along the branches: radii, throats
def _profile_values(vol: BitVolume, values) -> torch.Tensor:
    """The checks of a value map, all on the host: a float32 tensor of the volume's shape on its device."""
    if values is None:
        raise TypeError("values must be a float32 tensor (nz, ny, nx)")
    return _contact_values(vol, values, "values")


def _bits_as_float32(column) -> np.ndarray:
    return np.ascontiguousarray(column, dtype=np.int64).astype(np.uint32).view(np.float32)


@dataclass
class BranchValueRows:
    """The branches of skeleton_branch_profile: host arrays, row for row those of SkeletonBranchRows."""
    label: np.ndarray            # int64 (m,)
    voxels: np.ndarray           # int64 (m,)
    min: np.ndarray              # float32 (m,): the smallest value over the regular voxels of the branch -- its throat
    min_index: np.ndarray        # int64 (m,): the lowest flat index that attains it
    max: np.ndarray              # float32 (m,)
    max_index: np.ndarray        # int64 (m,)
    sum_q: np.ndarray            # int64 (m,): the sum of rint(float64(v) * 65536)
    mean: np.ndarray             # float64 (m,): (sum_q / 65536) / voxels
    attach_value: np.ndarray     # float32 (m, 2): the values at attach_index; nan for a cycle

    def __len__(self):
        return len(self.label)


@dataclass
class NodeValueRows:
    """The nodes of skeleton_branch_profile: host arrays, row for row those of SkeletonNodeRows."""
    label: np.ndarray            # int64 (n,)
    max: np.ndarray              # float32 (n,): the largest value over the voxels of the node
    max_index: np.ndarray        # int64 (n,): the lowest flat index that attains it

    def __len__(self):
        return len(self.label)


@dataclass
class SkeletonProfile:
    """skeleton_branch_profile's answer."""
    table: SkeletonBranches      # what skeleton_branches returns for the same arguments, from the same call
    branches: BranchValueRows
    nodes: NodeValueRows


def _profile_rows_from(rows, attach_value=None) -> BranchValueRows:
    """Host arithmetic on the rows of ComponentRuns.value_profile.  mean = (float64(sum_q) / 65536.0) / voxels."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, PROFILE_COLUMNS)
    m = len(rows)
    if attach_value is None:
        attach_value = np.full((m, 2), np.nan, dtype=np.float32)
    mean = (rows[:, 4].astype(np.float64) / 65536.0) / rows[:, 1].astype(np.float64)
    return BranchValueRows(rows[:, 0].copy(), rows[:, 1].copy(), _bits_as_float32(rows[:, 2]), rows[:, 5].copy(),
                           _bits_as_float32(rows[:, 3]), rows[:, 6].copy(), rows[:, 4].copy(), mean,
                           np.ascontiguousarray(attach_value, dtype=np.float32).reshape(m, 2))


def _node_value_rows_from(rows) -> NodeValueRows:
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
    return NodeValueRows(rows[:, 0].copy(), _bits_as_float32(rows[:, 2]), rows[:, 3].copy())


def _values_at(values: torch.Tensor, index: np.ndarray) -> np.ndarray:
    """The entries of the map at host flat indices -> float32 host array of their shape, nan where the index is negative."""
    index = np.ascontiguousarray(index, dtype=np.int64)
    out = np.full(index.shape, np.nan, dtype=np.float32)
    there = index >= 0
    if there.any():
        at = torch.from_numpy(index[there]).to(values.device)
        out[there] = values.contiguous().reshape(-1).index_select(0, at).cpu().numpy()
    return out


def skeleton_branch_profile(skel: BitVolume, values: torch.Tensor, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0,
                            min_voxels=0) -> SkeletonProfile:
    """A per-voxel value along the branches of a skeleton -> SkeletonProfile: with values = distance_transform of the OBJECT, the
    radius of the object along its centre-line -- how wide each channel is and where it is narrowest (Tb.Th along the skeleton
    in BoneJ, the throat radius of a pore-network model).  values: a float32 device tensor of the volume's shape.  One
    definition (include/tomo_hip.h): per branch of skeleton_branches, over its REGULAR voxels only, min and max compare the
    float32 bit patterns, min_index / max_index are the lowest flat index (z * ny + y) * nx + x that attains each, sum_q is the
    int64 sum of rint(float64(v) * 65536) -- fixed point at 2^-16, the same bytes on every run and under every order -- and
    mean = (sum_q / 65536) / voxels.  attach_value holds the values at attach_index (nan for a cycle).  Per node: the largest
    value over its voxels and the lowest index that attains it.  An entry on a set voxel must be admitted: 0.0 <= v < 2^20,
    not -0.0 (ValueError otherwise); the entries of unset voxels are never read and may be anything.
    table is skeleton_branches' answer from the same call, and the rows line up with table.branches / table.nodes by
    construction: the value passes run under the run tables and the one selection of that call, there is no second labelling.
    On the device: tomo_profile_stats, tomo_profile_where, tomo_profile_rows under the tables of the regular voxels,
    tomo_cc_value_max / _first / _rows under those of the node voxels, one gather of 2 m entries.  Memory: 28 bytes per branch,
    12 per node, nothing per voxel.  An empty skeleton launches nothing past the split; one without regular voxels gives zero
    branch rows.  Arguments are checked before the first launch."""
    args = _branch_args(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x, min_voxels)
    values = _profile_values(skel, values)
    COUNTERS["branch_profile"] += 1
    t, runs_r, runs_n = _skeleton_branches(skel, args, slice_depths)
    branches, nodes = _profile_rows_from(np.zeros((0, PROFILE_COLUMNS))), _node_value_rows_from(np.zeros((0, 4)))
    if runs_n is not None:
        nodes = _node_value_rows_from(runs_n.value_max(values))
    if runs_r is not None:
        rows = runs_r.value_profile(values, args[4])
        branches = _profile_rows_from(rows, _values_at(values, t.branches.attach_index))
    return SkeletonProfile(t, branches, nodes)


def _check_factor(factor) -> float:
    if isinstance(factor, (bool, np.bool_)) or not isinstance(factor, (int, float, np.integer, np.floating)) or not factor >= 0:
        raise ValueError("factor must be a non-negative number")
    return float(factor)


def prune_skeleton_relative(skel: BitVolume, values: torch.Tensor, factor=1.0, min_length_mm=0.0, slice_depths=None, mm_per_pixel_y=1.0,
                            mm_per_pixel_x=1.0, rounds=None) -> PrunedSkeleton:
    """prune_skeleton with a threshold that follows the object: one round removes every branch of kind 2 with
    length_mm < max(min_length_mm, factor * r), r = the float64 of the entry of `values` at the attached voxel of the node that
    is NOT the free end -- with values = distance_transform of the object, the radius of the object where the spur leaves it.
    Curve thinning makes a thick part sprout spurs about as long as the part is thick, so one absolute length is wrong for any
    object with two scales; factor 1.0 removes a spur that does not reach out of the ball it hangs from.  The clears, the
    free-end voxel that goes along, the topology and the meaning of rounds (default: to the fixed point) are prune_skeleton's;
    factor=0 IS prune_skeleton(min_length_mm).  An r that is nan compares false: the branch stays.  factor negative or nan:
    ValueError; values: a float32 device tensor of the volume's shape (TypeError / ValueError).  Per round one gather of the
    spurs' entries on top of prune_skeleton's work.  Arguments are checked before the first launch."""
    args = _branch_args(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    values = _profile_values(skel, values)
    factor = _check_factor(factor)
    min_length_mm = float(min_length_mm)
    if math.isnan(min_length_mm):
        raise ValueError("min_length_mm must be a number")
    rounds = _check_rounds(rounds)
    COUNTERS["prune_relative"] += 1

    def rule(t):
        b = t.branches
        spur = b.kind == 2
        stays = np.concatenate([[False], t.nodes.free_end])[b.nodes[spur]]            # (k, 2): exactly one True a row
        held = np.where(stays[:, 0], b.attach_index[spur, 1], b.attach_index[spur, 0])
        gone = np.zeros(len(b), dtype=bool)
        with np.errstate(invalid="ignore"):
            gone[spur] = b.length_mm[spur] < np.maximum(min_length_mm, factor * _values_at(values, held).astype(np.float64))
        return gone

    return _prune(skel, args, slice_depths, rounds, rule, "prune_skeleton_relative")


def local_thickness(vol: BitVolume, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0, radii_mm=None,
                    max_levels=LOCAL_THICKNESS_MAX_LEVELS) -> LocalThickness:
    """Local thickness (Hildebrand & Ruegsegger) of a resident volume in millimetres -> LocalThickness.
    Coordinates and background are distance_transform's: voxel (k, j, i) sits at (zt[k + 1], yt[j + 1], xt[i + 1]) of
    distance_positions, everything outside the stack is background.  D2(q) is the float64 squared inside distance of set voxel
    q, |pq|^2 = ((dx^2 + dy^2) + dz^2) in float64, every d a difference of two table entries.  For the ascending squared radii
    r_1^2 < ... < r_K^2
        level(p) = max{ k : there is a set voxel q with D2(q) >= r_k^2 and |pq|^2 < r_k^2 }
    at a set voxel p, 0 without such a k: {D2 >= r_k^2} are the centres where the open ball of radius r_k fits, and {level
    reaches k} is the opening by that ball (opening_volume).  Digital openings are not monotone in r -- a level can cover fewer
    voxels than the next larger one -- hence the maximum.  thickness = float32(2 r_level) at a set voxel of level >= 1, 0.0 at
    a set voxel below r_1, +0.0 at every unset voxel.
    radii_mm=None (exact): the levels are all distinct values of D2 over the set voxels and the result is exactly
    2 max{D(q) : |pq| < D(q)}: every set voxel reads at least 2 D(p), the maximum is twice the inscribed radius, nothing is
    uncovered.  More than max_levels distinct values: ValueError before any level runs -- pass radii_mm then.  That happens for
    any sizeable solid, and with spacings that are not exactly representable: values equal on paper differ in the last bit and
    count as distinct.  Exact mode is for unit or binary-fraction spacings and for thin structures.
    radii_mm = a strictly ascending list of positive finite radii: r_k^2 = r_k * r_k in float64; levels above the largest D2
    are never launched and count 0.
    level_volume_mm3: per level the voxels per slice times (mm_x * mm_y) * depth, added in ascending z in float64
    (component_properties' order).  mean_mm / std_mm / max_mm: of the diameter 2 r_k over the covered set voxels, weighted by
    that volume; 0.0 for an empty volume.
    Cost: one inside transform, then per level one ballot pass and one outside transform of a bit volume (the cheap bit-scan x
    pass), then one finishing pass.  Memory: D2 at 8 B per voxel (beyond LOCAL_THICKNESS_VOLUME_BUDGET bytes: ValueError before
    anything is allocated), the result at 4 B per voxel, one extra bit volume and distance_transform's chunked workspace; exact
    mode also pays torch.unique's sort of the positive D2.  Three host reads in exact mode (the level count, the levels, the
    counts), two with radii (the largest D2, the counts)."""
    exact = radii_mm is None
    radii = None if exact else _check_radii(radii_mm)
    max_levels = int(max_levels)
    if max_levels < 1:
        raise ValueError("max_levels must be at least 1")
    nz, ny, nx = vol.shape
    distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)      # the depth and pixel checks, before any device use
    if 8 * nz * ny * nx > LOCAL_THICKNESS_VOLUME_BUDGET:
        raise ValueError("local_thickness: the squared distances of a %d x %d x %d volume take %d bytes, more than "
                         "LOCAL_THICKNESS_VOLUME_BUDGET (%d)" % (nz, ny, nx, 8 * nz * ny * nx, LOCAL_THICKNESS_VOLUME_BUDGET))
    weights = _slice_weights(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)[:nz]
    plan = _DistancePlan(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    L, dev = _lib.lib(), vol.device
    COUNTERS["local_thickness"] += 1
    d2 = torch.empty(vol.shape, dtype=torch.float64, device=dev)
    _lib.check(L.tomo_edt_squared(*plan.head(), 1, _p(d2), *plan.tail()), "tomo_edt_squared")
    if exact:
        levels = d2[d2 > 0].unique()                             # torch.unique: ascending; D2 > 0 exactly at the set voxels
        if levels.numel() > max_levels:
            raise ValueError("local_thickness: %d distinct squared distances, more than max_levels (%d): give the levels in "
                             "radii_mm" % (levels.numel(), max_levels))
        r2 = levels.cpu().numpy()
        radii = np.sqrt(r2)
        live = len(r2)
    else:
        r2 = radii * radii
        live = int(np.searchsorted(r2, float(d2.max().item()), side="right"))     # r_k^2 <= the largest D2: a centre exists
    K = len(r2)
    level_map = torch.zeros(vol.shape, dtype=torch.int32, device=dev)
    eroded = torch.empty_like(plan.bits) if live else None
    bits, nzyx = plan.head()[0], plan.head()[1:4]
    _thickness_levels(plan, d2, r2, live, level_map, eroded)
    del d2
    values = torch.from_numpy((2.0 * radii).astype(np.float32)).to(dev) if K else None
    counts = torch.empty((nz, K + 1), dtype=torch.int64, device=dev)
    _lib.check(L.tomo_edt_thickness_finish(_p(level_map), bits, *nzyx, _p(values), K, _p(counts), _stream()),
               "tomo_edt_thickness_finish")
    per_slice = counts.cpu().numpy()
    volume = np.zeros(K, dtype=np.float64)
    for z in range(nz):                                          # ascending z, one float64 addition per slice and level
        volume += per_slice[z, 1:] * weights[z]
    voxels = per_slice.sum(axis=0)
    mean, std, top = _thickness_statistics(radii, volume)
    return LocalThickness(level_map.view(torch.float32), radii, voxels[1:].copy(), volume, int(voxels[0]), mean, std, top)


def opening_volume(vol: BitVolume, radius_mm, slice_depths=None, mm_per_pixel_y=1.0, mm_per_pixel_x=1.0) -> BitVolume:
    """The opening of a resident volume by the OPEN ball of radius_mm millimetres -> a NEW BitVolume; `vol` is left untouched:
    the set voxels p with a set voxel q such that D2(q) >= radius_mm ** 2 and |pq|^2 < radius_mm ** 2 (local_thickness'
    definitions), i.e. local_thickness(vol, ..., radii_mm=[radius_mm]).thickness > 0.  radius_mm == 0: a copy.
    One inside transform whose tail ballots the eroded set, one outside transform of those bits whose tail ballots d2 < r^2
    and ANDs the original words: two bit volumes and distance_transform's chunked workspace, never a float per voxel."""
    r = float(radius_mm)
    if not (math.isfinite(r) and r >= 0):
        raise ValueError("radius_mm must be finite and not negative")
    plan = _DistancePlan(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    COUNTERS["opening_volume"] += 1
    if r == 0:
        return BitVolume(plan.bits.clone(), vol.shape)
    L = _lib.lib()
    bits, rest = plan.head()[0], plan.head()[1:]
    eroded, out = torch.empty_like(plan.bits), torch.empty_like(plan.bits)
    _lib.check(L.tomo_edt_threshold_masked(bits, *rest, 1, r * r, 0, bits, _p(eroded), *plan.tail()), "tomo_edt_threshold_masked")
    _lib.check(L.tomo_edt_threshold_masked(_p(eroded), *rest, 0, r * r, 1, bits, _p(out), *plan.tail()), "tomo_edt_threshold_masked")
    return BitVolume(out, vol.shape)


def pack_closed(mask: torch.Tensor) -> BitVolume:
    """np.stack + _close_volume_ends (voxel_processor.py:46, :56-77) from a device uint8 / bool (nz, ny, nx) mask stack in ONE
    pass over the mask where the layout allows it (nz >= 3, nx % 16 == 0): pack + fill the end slices, then the fused
    pack + stencil kernel; otherwise pack, then close_ends in place."""
    mask = _mask_u8(mask)
    nz, ny, nx = mask.shape
    if nz < 3 or nx % 16 != 0 or mask.data_ptr() % 16 != 0 or not PACK_CLOSE_FUSED:
        return close_ends(pack(mask), inplace=True)
    L = _lib.lib()
    wx = L.tomo_words_per_row(nx)
    bits = torch.empty((nz, ny, wx), dtype=torch.int64, device=mask.device)
    scratch = torch.empty(ny * wx + 8, dtype=torch.int64, device=mask.device)
    _lib.check(L.tomo_pack_close_ends(_p(mask), _p(bits), nz, ny, nx, _p(scratch), _stream()), "tomo_pack_close_ends")
    return BitVolume(bits, (nz, ny, nx))


def close_ends(vol: BitVolume, inplace: bool = False, fill: bool = True) -> BitVolume:
    """_close_volume_ends (voxel_processor.py:56-77): fill holes of the two end slices, then the z recurrence.
    inplace=True overwrites `vol` (for a volume the caller owns, e.g. fresh from pack) instead of copying it first.
    fill=False: the z recurrence alone, the end slices taken as they are (a Z-slab rank puts its neighbours' slices there)."""
    nz, ny, nx = vol.shape
    L = _lib.lib()
    out = vol if inplace else BitVolume(vol.bits.clone(), vol.shape)
    if fill:
        scratch = torch.empty(ny * out.bits.shape[2] + 8, dtype=torch.int64, device=vol.device)
        _lib.check(L.tomo_fill_holes_ends(_p(out.bits), nz, ny, nx, _p(scratch), _stream()), "tomo_fill_holes_ends")
    if nz > 2:
        ws = torch.empty(L.tomo_close_ends_workspace_words(nz, ny, nx), dtype=torch.int64, device=vol.device)
        _lib.check(L.tomo_close_ends_scan(_p(out.bits), nz, ny, nx, _p(ws), _stream()), "tomo_close_ends_scan")
    return out


def smooth(vol: BitVolume, iterations: int = 3, create_manifold: bool = True) -> BitVolume:
    """smooth_voxel_data (voxel_processor.py:79-97): opening, then `iterations` closings (3-D cross).  The pass list is
    planned in tomo_smooth (csrc/bits.hip): repeated closings are one closing, so every request is ONE launch."""
    nz, ny, nx = vol.shape
    out = torch.empty_like(vol.bits)
    _lib.check(_lib.lib().tomo_smooth(_p(vol.bits), _p(out), nz, ny, nx, int(iterations), int(bool(create_manifold)), _stream()),
               "tomo_smooth")
    return BitVolume(out, vol.shape)


# ----------------------------------------------------------------------------- field
def make_field(vol: BitVolume, manifold: bool = True, add_padding: bool = True, sparse: bool = False) -> Field:
    """surface_extractor.py:43-53 + float32 cast: the scalar field marching cubes reads.

    sparse=True (Gaussian field from the bit volume only) leaves constant tiles that no marching-cubes cell at level 0.5
    can touch unwritten: `data` is then valid only within one voxel of the surface's cells (Field.sparse is set)."""
    nz, ny, nx = vol.shape
    L = _lib.lib()
    pad = 1 if (manifold and add_padding) else 0
    Nz, Ny, Nx = nz + 2 * pad, ny + 2 * pad, nx + 2 * pad
    pitch = L.tomo_field_pitch(nx, pad)
    data = torch.empty((Nz, Ny, pitch), dtype=torch.float32, device=vol.device)
    xorg = L.tomo_field_xorg(pad)
    # the field kernel leaves the sign records (marching-cubes pass 1 input) behind as a by-product
    fused = bool(manifold)
    signs = None
    sbuf = None
    gcls = None
    if fused:
        S, NyP = L.tomo_mc_segments_per_row(Nx, xorg), L.tomo_sign_rows(Ny)
        sbuf = torch.empty(L.tomo_sign_buffer_words(Nz, Ny, Nx, xorg), dtype=torch.int64, device=vol.device)
        signs = sbuf[: Nz * S * NyP * 4].view(Nz, S, NyP, 4)
        gcls = torch.empty((Nz, NyP // 16, S), dtype=torch.uint8, device=vol.device)
    is_sparse = bool(manifold and FIELD_FROM_BITS and sparse)
    if is_sparse:
        span = torch.empty(L.tomo_field_span_bytes(nz, ny, nx, pad), dtype=torch.uint8, device=vol.device)
        _lib.check(L.tomo_field_fill_bits_sparse(_p(vol.bits), _p(data), nz, ny, nx, pad, _p(sbuf), _p(gcls), _p(span), _stream()),
                   "tomo_field_fill_bits_sparse")
    elif manifold and FIELD_FROM_BITS:
        # the Gaussian field straight from the bit volume: border rules applied while the kernel stages its input
        _lib.check(L.tomo_field_fill_bits(_p(vol.bits), _p(data), nz, ny, nx, pad, _p(sbuf), _p(gcls), _stream()),
                   "tomo_field_fill_bits")
    else:
        ez, ey, ewx = L.tomo_ext_slices(nz, pad), L.tomo_ext_rows(ny, pad), L.tomo_ext_words_per_row(nx, pad)
        ext = torch.empty((ez, ey, ewx), dtype=torch.int64, device=vol.device)
        _lib.check(L.tomo_extend_bits(_p(vol.bits), _p(ext), nz, ny, nx, pad, _stream()), "tomo_extend_bits")
        _lib.check(L.tomo_field_fill(_p(ext), _p(data), nz, ny, nx, pad, 1 if manifold else 0, _p(sbuf), _p(gcls), _stream()),
                   "tomo_field_fill")
    return Field(data, Nz, Ny, Nx, pitch, xorg, signs, 0.5, gcls, sparse=is_sparse)


def field_signs(f: Field, level: float, z_begin: int = 0, z_end: int = None):
    """Sign records of a float field for slices [z_begin, z_end) (all by default), written into f.signs."""
    L = _lib.lib()
    z_end = f.Nz if z_end is None else z_end
    if f.signs is None:
        S, NyP = L.tomo_mc_segments_per_row(f.Nx, f.xorg), L.tomo_sign_rows(f.Ny)
        f.signs = torch.empty((f.Nz, S, NyP, 4), dtype=torch.int64, device=f.data.device)
        f.gcls = torch.empty((f.Nz, NyP // 16, S), dtype=torch.uint8, device=f.data.device)
    _lib.check(L.tomo_field_signs(_p(f.data), f.Nz, f.Ny, f.Nx, f.pitch, f.xorg, float(level), z_begin, z_end,
                                  _p(f.signs), _p(f.gcls), _stream()), "tomo_field_signs")
    f.signs_level = float(level)
    return f.signs


def field_from_dense(dense: torch.Tensor) -> Field:
    """Wrap an arbitrary float32 (Nz,Ny,Nx) device volume (tests: marching cubes on noise volumes)."""
    Nz, Ny, Nx = dense.shape
    pitch = (Nx + 3) // 4 * 4          # the marching-cubes loads read whole float4s inside a row's pitch
    data = torch.zeros((Nz, Ny, pitch), dtype=torch.float32, device=dense.device)
    data[:, :, :Nx] = dense
    return Field(data, Nz, Ny, Nx, pitch, 0)


# ----------------------------------------------------------------------------- marching cubes
def _check_limits(na, nv=0, nf=0, ids=1):
    """TomoError when a pass leaves the 32-bit index range: na list entries (LIST_LIMIT; `ids` int32 table entries per list
    position -- 4 in the mc3 chain), nv vertices / nf triangles (MESH_LIMIT)."""
    if na >= LIST_LIMIT or na * ids >= 2 ** 31:
        raise _lib.TomoError("surface too large for 32-bit indices")
    if nv >= MESH_LIMIT or nf >= MESH_LIMIT:
        raise _lib.TomoError("mesh too large for 32-bit indices")


def drop_degenerate(faces: torch.Tensor) -> torch.Tensor:
    """Triangles with three distinct vertex indices, order kept (surface_extractor.py:122-125)."""
    return faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]


def marching_cubes(f: Field, level: float = 0.5, z_offset: int = 0):
    """skimage.measure.marching_cubes(volume, level) (surface_extractor.py:55) -> RawMesh or None.

    None stands for the two exceptions of the wrapper that the reference swallows
    (level outside the data range / no vertices found).
    """
    L = _lib.lib()
    if min(f.Nz, f.Ny, f.Nx) < 2:
        return None
    dev = f.data.device
    st = _stream()
    lvl = float(level)
    geo = (f.Nz, f.Ny, f.Nx, f.pitch, f.xorg, lvl)
    spr = L.tomo_mc_segments_per_row(f.Nx, f.xorg)
    nseg = f.Nz * f.Ny * spr
    # pass 1: active voxels per segment, scan, list of active segments
    if f.signs is None or f.signs_level != lvl:
        if f.sparse:
            raise _lib.TomoError("a sparse field holds floats only near the 0.5 surface: other levels need make_field(sparse=False)")
        field_signs(f, lvl)
    seg_act = torch.empty(nseg * 4, dtype=torch.int64, device=dev)   # 32-byte record per NON-EMPTY segment
    seg_cnt = torch.empty(nseg, dtype=torch.int32, device=dev)       # active voxels of every segment
    _lib.check(L.tomo_mc_classify(_p(f.signs), _p(f.gcls), f.Nz, f.Ny, f.Nx, f.xorg, _p(seg_act), _p(seg_cnt), st), "tomo_mc_classify")
    seg_aoff = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)   # [0:4] segment scan, [4:8] voxel scan + emit errors
    wsb = L.tomo_mc_scan_workspace_bytes(nseg)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.tomo_mc_scan_segments(_p(seg_cnt), nseg, _p(seg_aoff), _p(totals), _p(ws), wsb, st), "tomo_mc_scan_segments")
    # pass 2-3: compact voxel list, one MC33 evaluation per active voxel, scan of the counts.
    # With a size hint (the list length of the last field of this geometry) the three launches go out BEFORE the segment
    # scan's total has come back -- into buffers of hint + 25 % entries, guarded on the device -- and one download
    # brings all counters; a list that turns out longer than the buffer is simply redone the plain way.
    tot2 = totals[4:]
    hint_key = (f.Nz, f.Ny, f.Nx)
    hint = _NA_HINT.get(hint_key) if NA_HINTS else None
    na = None
    if hint:
        cap = int(hint * 1.25) + 4096
        if cap < LIST_LIMIT:
            vox_key = torch.empty(cap, dtype=torch.int64, device=dev)
            vox_counts = torch.empty(cap, dtype=torch.int32, device=dev)
            vox_flags = torch.empty(cap, dtype=torch.uint8, device=dev)
            vox_voff = torch.empty(cap + 1, dtype=torch.int32, device=dev)
            vox_foff = torch.empty(cap + 1, dtype=torch.int32, device=dev)
            wsb2 = L.tomo_mc_scan_workspace_bytes(cap)
            ws2 = torch.empty(wsb2, dtype=torch.uint8, device=dev)
            _lib.check(L.tomo_mc_list_capped(f.Nz, f.Ny, f.Nx, f.xorg, _p(seg_aoff), _p(seg_act), _p(vox_key), cap, st),
                       "tomo_mc_list_capped")
            _lib.check(L.tomo_mc_eval_capped(_p(f.data), *geo, _p(vox_key), cap, _p(totals), _p(vox_counts), _p(vox_flags), st),
                       "tomo_mc_eval_capped")
            _lib.check(L.tomo_mc_scan(_p(vox_counts), cap, _p(vox_voff), _p(vox_foff), _p(tot2), _p(ws2), wsb2, st),
                       "tomo_mc_scan")
            host = totals.cpu()
            na, nv, nf = int(host[0]), int(host[4]), int(host[5])
            if na > cap:
                COUNTERS["na_hint_miss"] += 1
                na = None                                   # too short: the plain path below redoes list, eval and scan
            else:
                COUNTERS["na_hint_hit"] += 1
    if na is None:
        na = int(totals[0].item())
        if na == 0:
            return None
        _check_limits(na)
        vox_key = torch.empty(na, dtype=torch.int64, device=dev)
        _lib.check(L.tomo_mc_list(f.Nz, f.Ny, f.Nx, f.xorg, _p(seg_aoff), _p(seg_act), _p(vox_key), st), "tomo_mc_list")
        vox_counts = torch.empty(na, dtype=torch.int32, device=dev)
        vox_flags = torch.empty(na, dtype=torch.uint8, device=dev)
        _lib.check(L.tomo_mc_eval(_p(f.data), *geo, _p(vox_key), na, _p(vox_counts), _p(vox_flags), st), "tomo_mc_eval")
        vox_voff = torch.empty(na + 1, dtype=torch.int32, device=dev)
        vox_foff = torch.empty(na + 1, dtype=torch.int32, device=dev)
        wsb2 = L.tomo_mc_scan_workspace_bytes(na)
        ws2 = torch.empty(wsb2, dtype=torch.uint8, device=dev)
        _lib.check(L.tomo_mc_scan(_p(vox_counts), na, _p(vox_voff), _p(vox_foff), _p(tot2), _p(ws2), wsb2, st),
                   "tomo_mc_scan")
        nv, nf = [int(x) for x in tot2[:2].cpu()]
    del seg_cnt
    if na == 0:
        return None
    _NA_HINT[hint_key] = na
    if nv == 0:
        return None
    _check_limits(na, nv, nf)
    # pass 4: vertices and triangles
    vkey = torch.empty(nv, dtype=torch.int64, device=dev)
    vpos = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces32 = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    _lib.check(L.tomo_mc_emit(_p(f.data), *geo, _p(vox_key), na, _p(seg_act), _p(seg_aoff), _p(vox_voff), _p(vox_foff), _p(vox_flags),
                              int(z_offset), _p(vkey), _p(vpos), _p(faces32), _p(tot2), st), "tomo_mc_emit")
    mesh = RawMesh(vkey, vpos, faces32[:nf])
    mesh._mc = (f, geo, vox_key, na, seg_act, seg_aoff, vox_voff, vox_flags)   # for first_touch_order (manifold=False)
    mesh._stats = totals  # [7] != 0 would mean a triangle corner without vertex (no download here: the tests read it)
    return mesh


_depth_tables = {}      # (device, thread, add_padding, bytes of the depth table) -> (cum, adj) device tensors


def _depth_tables_on_device(d, add_padding, dev):
    """surface_extractor.py:88-95: adjusted depths and their cumulative sums, uploaded once per distinct table (the
    orchestrator and the benchmark pass the same table call after call)."""
    # per thread: the rank threads of a rehearsed slab job run on their own streams, and a tensor made on one stream must not
    # be handed to kernels of another without the allocator knowing
    key = (str(dev), threading.get_ident(), bool(add_padding), d.tobytes())
    hit = _depth_tables.get(key)
    if hit is None:
        adj = np.concatenate([[d[0]], d, [d[-1]]]) if add_padding else d
        cum = np.cumsum(np.concatenate([[0], adj]))
        hit = (torch.from_numpy(np.ascontiguousarray(cum)).to(dev), torch.from_numpy(np.ascontiguousarray(adj)).to(dev))
        if len(_depth_tables) >= 32:
            _depth_tables.pop(next(iter(_depth_tables)))
        _depth_tables[key] = hit
    return hit


def _depth_args(slice_depths, add_padding, dev):
    """The depth table as the vertex kernels take it: (cum tensor, its length, adj tensor, its length); no table: (None, 0, None, 0)."""
    d = np.ascontiguousarray(slice_depths, dtype=np.float64)
    if not len(d):
        return None, 0, None, 0
    cum_t, adj_t = _depth_tables_on_device(d, add_padding, dev)
    return cum_t, cum_t.shape[0], adj_t, adj_t.shape[0]


def finalize_vertices(vpos: torch.Tensor, slice_depths, mm_per_pixel_y, mm_per_pixel_x, manifold=True, add_padding=True):
    """surface_extractor.py:57-65 and :82-113, in place on the (V,3) float32 device tensor."""
    cum_t, ncum, adj_t, nadj = _depth_args(slice_depths, add_padding, vpos.device)
    _lib.check(_lib.lib().tomo_vertex_finalize(_p(vpos), vpos.shape[0], 1 if manifold else 0, _p(cum_t), ncum, _p(adj_t),
                                               nadj, float(np.float32(mm_per_pixel_y)), float(np.float32(mm_per_pixel_x)),
                                               _stream()), "tomo_vertex_finalize")
    return vpos


def unique_rows(vpos: torch.Tensor):
    """np.unique(rows, axis=0, return_inverse=True) of finalised vertex rows -> (uniq (U,3), rank (V,) int32)."""
    L = _lib.lib()
    dev = vpos.device
    nv = vpos.shape[0]
    vpos = vpos.contiguous()
    uniq = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    rank = torch.empty(nv, dtype=torch.int32, device=dev)
    if nv == 0:
        return uniq, rank
    wsb = L.tomo_mesh_unique_workspace_bytes(nv)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.check(L.tomo_mesh_unique(_p(vpos), nv, _p(uniq), _p(rank), _p(totals), _p(ws), wsb, _stream()), "tomo_mesh_unique")
    return uniq[: int(totals[0].item())], rank


def lookup_rows(uniq: torch.Tensor, query: torch.Tensor, sync: bool = True):
    """Index of every query row in the sorted unique row list -> (idx (Q,) int32, number of rows not found -- an int, or
    with sync=False the 1-element device tensor, so that the caller can fold the download into a later one)."""
    dev = uniq.device
    nq = query.shape[0]
    out = torch.empty(nq, dtype=torch.int32, device=dev)
    miss = torch.zeros(1, dtype=torch.int64, device=dev)
    if nq == 0:
        return out, (0 if sync else miss)
    _lib.check(_lib.lib().tomo_mesh_lookup(_p(uniq.contiguous()), uniq.shape[0], _p(query.contiguous()), nq, _p(out), _p(miss),
                                           _stream()), "tomo_mesh_lookup")
    return out, (int(miss.item()) if sync else miss)


def first_touch_order(mesh: RawMesh):
    """Renumber a RawMesh the way skimage numbers vertices (order of first touch in the serial cell scan).
    Returns (vpos (V,3) float32, faces (F,3) int32): what measure.marching_cubes returns to the reference."""
    L = _lib.lib()
    f, geo, vox_key, na, seg_act, seg_aoff, vox_voff, vox_flags = mesh._mc
    dev = mesh.vpos.device
    st = _stream()
    nv = mesh.vpos.shape[0]
    created = torch.empty(na, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    args = (_p(f.data), *geo, _p(vox_key), na, _p(seg_act), _p(seg_aoff), _p(vox_voff), _p(vox_flags))
    _lib.check(L.tomo_mc_first_touch(*args, 0, _p(created), None, None, _p(totals), st), "tomo_mc_first_touch")
    base = torch.empty(na + 1, dtype=torch.int32, device=dev)
    wsb = L.tomo_mc_scan_workspace_bytes(na)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.tomo_mc_scan(_p(created), na, _p(base), None, _p(totals), _p(ws), wsb, st), "tomo_mc_scan")
    ft_rank = torch.full((nv,), -1, dtype=torch.int32, device=dev)
    _lib.check(L.tomo_mc_first_touch(*args, 1, None, _p(base), _p(ft_rank), _p(totals), st), "tomo_mc_first_touch")
    ncreated, _, _, nbad = [int(x) for x in totals.cpu()]
    if nbad or ncreated != nv or int((ft_rank < 0).sum().item()):
        raise _lib.TomoError("internal error: first-touch numbering is not a permutation of the vertices")
    idx = ft_rank.to(torch.int64)
    vpos = torch.empty_like(mesh.vpos)
    vpos[idx] = mesh.vpos
    faces = ft_rank[mesh.faces32.to(torch.int64)] if mesh.faces32.shape[0] else mesh.faces32
    return vpos, faces


def extract_surface(vol: BitVolume, slice_depths, mm_per_pixel_y, mm_per_pixel_x, manifold=True, add_padding=True):
    """extract_manifold_surface (surface_extractor.py:34-75) on device tensors.

    Returns (vertices (V,3) float32, faces (F,3) int64 -- int32 and skimage's numbering when manifold=False)
    device tensors, or None where the reference returns None.
    """
    f = make_field(vol, manifold, add_padding, sparse=FIELD_SPARSE)
    if manifold:
        m = mc3_vertices(f, slice_depths, mm_per_pixel_y, mm_per_pixel_x, add_padding)
        return None if m is None else (m.uniq, m.faces_final)
    # surface_extractor.py:55-72 without the manifold branches: skimage's own numbering, int32 faces
    mesh = marching_cubes(f, 0.5)
    if mesh is None:
        return None
    vpos, faces = first_touch_order(mesh)
    finalize_vertices(vpos, slice_depths, mm_per_pixel_y, mm_per_pixel_x, False, add_padding)
    return vpos, faces


class PendingSurface:
    """extract_surface whose counters may not have been read yet: result() -> (vertices, faces) or None."""

    def __init__(self, value=None, surface=None):
        self._value, self._surface = value, surface

    def result(self):
        m, self._surface = self._surface, None
        if m is not None:
            if m.deferred:
                m = m.finish()
            self._value = None if m is None else (m.uniq, m.faces_final)
        return self._value


def extract_surface_submit(vol: BitVolume, slice_depths, mm_per_pixel_y, mm_per_pixel_x, manifold=True, add_padding=True):
    """extract_surface in two halves, for a caller that processes one stack after the other: everything is enqueued here
    (from the size hints of the last surface of this geometry) and the ONE download of the pass is started; .result() waits
    for it.  Enqueueing the next stack before reading this one keeps the GPU busy through the host's read (bench.py)."""
    if manifold:
        f = make_field(vol, manifold, add_padding, sparse=FIELD_SPARSE)
        return PendingSurface(surface=mc3_vertices(f, slice_depths, mm_per_pixel_y, mm_per_pixel_x, add_padding, defer=True))
    return PendingSurface(value=extract_surface(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x, manifold, add_padding))


# ----------------------------------------------------------------------------- mc3: marching cubes + finalise + unique, one chain
MC3 = True              # manifold=True surfaces go through the mc3 chain (csrc/mc.hip, "mc3"); the name is read by bench.py
_MC3_HINT = {}          # field geometry -> (active voxels, vertices, triangles) of the last surface of that geometry
# The unique stage: ONE hand-written kernel (tomo_mc3_sort_rank_fused; a workgroup per sort segment, everything in LDS) unless
# the last surface of the geometry had a segment too long for it (a flat cap of > 4 096 vertices between two planes, a noise
# slice): then rocPRIM's segmented sort + merge + rank kernels (tomo_mc3_sort_rank_top), as in rounds 2-3.
FUSED_SORT = os.environ.get("TOMO_FUSED_SORT", "1") not in ("", "0")     # A/B switch
_MC3_LARGE = {}         # field geometry -> True: use the rocPRIM path
_PINNED = {}


def _download(t):
    """A small int64 device vector (the 8 counters of a chain) in ONE transfer into page-locked memory -> list of ints (no
    pageable bounce buffer, no extra blit).  One buffer per device, thread and length: rank threads of a slab job share the process."""
    key = (str(t.device), threading.get_ident(), t.numel())
    host = _PINNED.get(key)
    if host is None:
        host = _PINNED[key] = torch.empty(t.numel(), dtype=torch.int64, pin_memory=True)
    host.copy_(t if t.dim() == 1 else t.reshape(-1), non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.tolist()


def wait_event(event, timeout_s, what="the stream"):
    """event.synchronize() with a deadline: polls (busy for the first 2 ms -- the usual wait is microseconds -- then in 0.1 ms
    naps) and raises TomoError after timeout_s seconds."""
    import time
    if event.query():
        return
    t0 = time.monotonic()
    while not event.query():
        dt = time.monotonic() - t0
        if dt > timeout_s:
            raise _lib.TomoError("%s did not arrive within %.0f s: the GPU is stuck or a neighbour rank has left the job" % (what, timeout_s))
        if dt > 2e-3:
            time.sleep(1e-4)


class PendingDownload:
    """A small int64 device vector on its way into page-locked memory: started on the current stream, read by wait().
    Every pending download owns its buffer for as long as it lives (several passes may be in flight), buffers are recycled
    per (device, thread, length)."""
    _free = {}

    def __init__(self, t):
        t = t.reshape(-1)
        self._key = (str(t.device), threading.get_ident(), int(t.numel()))
        pool = PendingDownload._free.setdefault(self._key, [])
        self._host = pool.pop() if pool else torch.empty(t.numel(), dtype=torch.int64, pin_memory=True)
        self._host.copy_(t, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(t.device))

    def wait(self, timeout_s=None):
        """timeout_s: give up (TomoError) when the copy has not arrived by then -- for a stream that carries RCCL calls, which
        have no timeout of their own: a neighbour rank that left the job must become an error here, not a hang."""
        if timeout_s is None:
            self._event.synchronize()
        else:
            wait_event(self._event, timeout_s, "the counters of a pass")
        out = self._host.tolist()
        PendingDownload._free[self._key].append(self._host)
        self._host = None
        return out


class Mc3Surface:
    """One pass of the mc3 chain over a manifold=True field at level 0.5, and the surface it leaves behind.  Built from the field,
    the depth table and pixel sizes, `z_offset` (a Z-slab rank's first padded slice), `z_top` (also count the rows with
    z' == z_top into tot[7]: the plane shared with the rank above) and optionally `tot`, the int64[8] its kernels count in (a
    caller may place it inside a larger buffer it downloads itself).  States, as mc3_vertices drives them:
      classified  classify(): sign records -> seg_act / seg_cnt
      enqueued    enqueue(cap, cap_v, cap_f) = build_list + eval_scan + vertices_sort into buffers of those capacities, faces()
                  adds the triangles; no count is read.  Capacities from a size hint are guesses: only the counters say
                  whether everything fitted
      deferred    `deferred` is set: enqueued from hints, counters unread.  With triangles start_counters() has begun their
                  download and finish() completes the pass; without, the caller reads `tot` itself and calls adopt()
      resolved    resolve() / adopt() have published uniq, table, faces_final, na / nv / nf and stored the size hint
    tot: [0] active voxels (na)  [1] vertices (nv)  [2] triangles (nf)  [3] overflow flags (bit 3: a sort segment too long for
    the fused kernel)  [4] rows that do not ascend strictly  [5] degenerate triangles  [6] corners without vertex  [7] rows on z_top.
    Buffers: field; seg_act, seg_cnt, seg_blk, seg_aoff (per segment); vox_key, vox_loc, vox_til, vox_flags, vox_used, vox_f3,
    vox_c3, blk3 (`cap` list positions); slice_tab (sort segments); vrec (rows + id, unsorted) and rows (sorted, duplicate-free),
    both of capacity cap_v; table int32 (vertex id -> row index; id = 4 * list position of the owner voxel + slot: 4 * cap
    entries); cap_f, the triangle capacity.  Results: `uniq` (U,3) float32 final rows in np.unique's order (rows[:nv] unless
    the general unique re-sorted them), `table`, and `faces_final` (F,3) int64 when the triangles were asked for."""

    def __init__(self, f, slice_depths, mm_per_pixel_y, mm_per_pixel_x, add_padding=True, z_offset=0, z_top=None, tot=None):
        self.field, self.z_offset = f, int(z_offset)
        self.z_top = float("nan") if z_top is None else float(z_top)
        self.hint_key = (f.Nz, f.Ny, f.Nx, self.z_offset)
        self._depth = _depth_args(slice_depths, add_padding, f.data.device)
        self._mm = (float(np.float32(mm_per_pixel_y)), float(np.float32(mm_per_pixel_x)))
        self.tot = torch.empty(8, dtype=torch.int64, device=f.data.device) if tot is None else tot
        self.uniq = self.table = self.faces_final = None
        self.nv = self.nf = self.na = 0
        self.deferred = False
        self._pending = None        # (PendingDownload of tot, triangles) between start_counters() and finish()

    def classify(self):
        L, f, dev = _lib.lib(), self.field, self.field.data.device
        if f.signs is None or f.signs_level != 0.5:
            if f.sparse:
                raise _lib.TomoError("a sparse field holds floats only near the 0.5 surface")
            field_signs(f, 0.5)
        nseg = f.Nz * f.Ny * L.tomo_mc_segments_per_row(f.Nx, f.xorg)
        self.seg_act = torch.empty(nseg * 4, dtype=torch.int64, device=dev)
        self.seg_cnt = torch.empty(nseg, dtype=torch.int32, device=dev)
        _lib.check(L.tomo_mc_classify(_p(f.signs), _p(f.gcls), f.Nz, f.Ny, f.Nx, f.xorg, _p(self.seg_act), _p(self.seg_cnt), _stream()),
                   "tomo_mc_classify")
        self.seg_blk = torch.empty((nseg + 255) // 256, dtype=torch.int32, device=dev)
        self.seg_aoff = torch.empty(nseg + 1, dtype=torch.int32, device=dev)

    def build_list(self, cap):
        f, self.cap = self.field, cap
        self.vox_key = torch.empty(cap, dtype=torch.int64, device=f.data.device)
        _lib.check(_lib.lib().tomo_mc3_list(f.Nz, f.Ny, f.Nx, f.xorg, _p(self.seg_cnt), _p(self.seg_act), _p(self.seg_blk), _p(self.seg_aoff),
                                            _p(self.vox_key), cap, _p(self.tot), _stream()), "tomo_mc3_list")

    def eval_scan(self, cap_v, cap_f):
        L, f, cap, st, dev = _lib.lib(), self.field, self.cap, _stream(), self.field.data.device
        self.vox_loc = torch.empty(cap, dtype=torch.int32, device=dev)
        self.vox_til = torch.empty(cap, dtype=torch.int32, device=dev)
        self.vox_flags = torch.empty(cap, dtype=torch.uint8, device=dev)
        self.vox_used = torch.empty(cap, dtype=torch.int16, device=dev)
        self.vox_f3 = torch.empty(3 * cap, dtype=torch.float32, device=dev)
        self.vox_c3 = torch.empty(3 * cap, dtype=torch.float32, device=dev)
        self.blk3 = torch.empty(3 * ((cap + 255) // 256), dtype=torch.int32, device=dev)
        self.slice_tab = torch.empty(L.tomo_mc3_slice_table_words(f.Nz, f.Ny), dtype=torch.int32, device=dev)
        _lib.check(L.tomo_mc3_eval(_p(f.data), f.Nz, f.Ny, f.Nx, f.pitch, f.xorg, 0.5, _p(self.vox_key), cap, _p(self.tot), self.z_offset,
                                   _p(self.vox_loc), _p(self.vox_til), _p(self.vox_flags), _p(self.vox_used), _p(self.vox_f3),
                                   _p(self.vox_c3), _p(self.blk3), st), "tomo_mc3_eval")
        _lib.check(L.tomo_mc3_scan(f.Nz, f.Ny, f.Nx, f.xorg, _p(self.seg_aoff), _p(self.vox_loc), cap, _p(self.blk3), _p(self.slice_tab),
                                   _p(self.tot), cap_v, cap_f, st), "tomo_mc3_scan")

    def vertices_sort(self, cap_v):
        """Finalised rows, then the unique stage: the fused kernel, or the library path once _MC3_LARGE names this geometry."""
        L, f, cap, tot, st, dev = _lib.lib(), self.field, self.cap, self.tot, _stream(), self.field.data.device
        cum_t, ncum, adj_t, nadj = self._depth
        self.cap_v = cap_v
        self.vrec = torch.empty((cap_v, 4), dtype=torch.float32, device=dev)
        keys = torch.empty(cap_v, dtype=torch.int32, device=dev)
        self.rows = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
        self.table = torch.empty(4 * cap, dtype=torch.int32, device=dev)
        fused = FUSED_SORT and not _MC3_LARGE.get(self.hint_key)
        idx = None if fused else torch.empty(cap_v, dtype=torch.int32, device=dev)
        _lib.check(L.tomo_mc3_vertices(f.Nz, f.Ny, f.Nx, f.xorg, _p(self.vox_key), cap, _p(tot), _p(self.vox_loc), _p(self.vox_flags),
                                       _p(self.vox_f3), _p(self.vox_c3), _p(self.blk3), _p(self.slice_tab), self.z_offset, 1, _p(cum_t), ncum,
                                       _p(adj_t), nadj, *self._mm, _p(self.vrec), _p(keys), _p(idx), st), "tomo_mc3_vertices")
        if fused:
            COUNTERS["mc3_sort_fused"] += 1
            _lib.check(L.tomo_mc3_sort_rank_fused(_p(self.vrec), _p(keys), cap_v, f.Nz, f.Ny, _p(self.slice_tab), _p(tot), _p(self.rows),
                                                  _p(self.table), self.z_top, st), "tomo_mc3_sort_rank_fused")
            return
        COUNTERS["mc3_sort_library"] += 1
        wsb = L.tomo_mc3_sort_workspace_bytes(cap_v, L.tomo_mc3_sort_segments(f.Nz, f.Ny))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _lib.check(L.tomo_mc3_sort_rank_top(_p(self.vrec), _p(keys), _p(idx), cap_v, f.Nz, f.Ny, _p(self.slice_tab), _p(tot), _p(self.rows),
                                            _p(self.table), _p(ws), wsb, self.z_top, st), "tomo_mc3_sort_rank_top")

    def enqueue(self, cap, cap_v, cap_f):
        """List, eval + scan, vertices + sort into buffers of the given capacities; no count is read."""
        self.build_list(cap)
        self.eval_scan(cap_v, cap_f)
        self.vertices_sort(cap_v)
        self.cap_f = cap_f

    def faces(self, table=None, again=False, slab_map=None):
        """The final int64 triangles through `table` (default: the chain's own; a Z-slab rank passes GLOBAL indices).
        slab_map = (gathered int64 (world, 8), rank, world, ids_next int32 or None, cap_top, cap_v): the triangles leave with
        GLOBAL indices of a Z-slab job, every count taken from device memory (tomo_mc3_faces_slab)."""
        L = _lib.lib()
        f, st = self.field, _stream()
        tab = self.table if table is None else table
        if tab.dtype != torch.int32 or tab.numel() < 4 * self.cap:
            raise ValueError("table must be int32 with 4 entries per list position")
        if again:
            self.tot[5:7].zero_()                               # the counters of an earlier faces pass
        faces = torch.empty((max(self.cap_f, 1), 3), dtype=torch.int64, device=tab.device)
        args = (f.Nz, f.Ny, f.Nx, f.xorg, _p(self.vox_key), self.cap, _p(self.tot), _p(self.seg_act), _p(self.seg_aoff), _p(self.vox_loc),
                _p(self.vox_til), _p(self.vox_used), _p(self.blk3), _p(tab), _p(faces), self.cap_f)
        if slab_map is not None:
            gathered, rank, world, ids_next, cap_top, cap_v = slab_map
            _lib.check(L.tomo_mc3_faces_slab(*args, _p(gathered), rank, world, _p(ids_next), cap_top, cap_v, st), "tomo_mc3_faces_slab")
        else:
            _lib.check(L.tomo_mc3_faces(*args, st), "tomo_mc3_faces")
        return faces

    def trim(self, host, faces, count=True):
        """The triangles a faces() pass really wrote, given its counters: raises on an internal inconsistency, drops the
        triangles with fewer than three distinct vertices (count: note that in COUNTERS) -> (F', 3) int64."""
        if host[6]:
            raise _lib.TomoError("internal error: %d triangle corners reference a missing vertex" % host[6])
        faces = faces[:host[2]]
        if host[5]:
            if count:
                COUNTERS["mc3_degenerate"] += 1
            faces = drop_degenerate(faces)
        return faces

    def faces_checked(self, table=None, again=False, faces=None):
        """faces(table) + the download of the counters + trim()."""
        if faces is None:
            faces = self.faces(table, again)
        return self.trim(_download(self.tot), faces)

    def start_counters(self, faces):
        """Deferred with triangles: the ONE download of the pass starts now, finish() waits for it."""
        self._pending, self.deferred = (PendingDownload(self.tot), faces), True

    def finish(self):
        """Second half of a deferred pass with triangles (one pass late, if the caller likes) -> self, or None as resolve()."""
        (pend, faces), self._pending = self._pending, None
        return self.resolve(pend.wait(), faces, True)

    def resolve(self, host, faces, with_faces):
        """Everything after the counters of a hinted chain have arrived (host = None: no hinted chain ran): a chain that did not
        fit is redone with exact sizes, one host read per stage.  -> self, or None where the reference returns None."""
        key, tot = self.hint_key, self.tot
        if host is not None:
            if host[3]:
                COUNTERS["mc3_hint_miss"] += 1
                if host[3] & 8:
                    _MC3_LARGE[key] = True                       # a sort segment too long for the fused kernel: the library path from now on
                host = None                                      # something did not fit: redo with exact sizes
            else:
                COUNTERS["mc3_hint_hit"] += 1
        if host is None:
            self.build_list(1 << 16)                             # a token buffer: tot[0] comes out exact, nothing is written past it
            na = _download(tot)[0]
            if na == 0:
                return None
            _check_limits(na, ids=4)
            self.build_list(na)
            self.eval_scan(2 ** 31 - 2, 2 ** 31 - 2)
            host = _download(tot)
            nv, nf = host[1], host[2]
            if nv == 0:
                _MC3_HINT[key] = (na, 1, 1)
                return None
            _check_limits(na, nv, nf, ids=4)
            self.vertices_sort(nv)
            self.cap_f = max(nf, 1)
            if FUSED_SORT and not _MC3_LARGE.get(key):
                # value 8 (bit 3) of tot[3]: a segment the fused kernel cannot hold in LDS -- the library path repeats the stage and stays
                if _download(tot)[3] & 8:
                    _MC3_LARGE[key] = True
                    tot[3:5].zero_()
                    tot[7].zero_()
                    self.vertices_sort(nv)
            faces = self.faces() if with_faces else None
            host = _download(tot)
        return self.adopt(host, faces)

    def adopt(self, host, faces=None, slab=False):
        """The eight counters of a chain that fitted are on the host: check the limits, publish na / nv / nf, uniq and the size
        hint, let the general unique decide where the rows do not ascend strictly, and (faces: what faces() returned) trim the
        triangles into faces_final.  -> self, or None for an empty surface.
        slab=True -- a Z-slab rank whose deferred pass all ranks found exact, so host[4] is 0: an empty slab stays a surface (the
        rank keeps its place in the numbering), the hint is floored at 1 so that the next pass runs from hints too, and COUNTERS
        is left alone (the slab pass has never counted its exact or degenerate outcomes)."""
        na, nv, nf = self.na, self.nv, self.nf = host[0], host[1], host[2]
        if not slab and (na == 0 or nv == 0):
            return None
        _check_limits(na, nv, nf, ids=4)
        _MC3_HINT[self.hint_key] = (max(na, 1), max(nv, 1), max(nf, 1)) if slab else (na, nv, nf)
        self.uniq, self.deferred = self.rows[:nv], False
        if host[4] and not slab:
            # duplicate rows or a rounding coincidence: the general sort decides (np.unique semantics), the triangles follow
            COUNTERS["mc3_general_unique"] += 1
            self.uniq, rank = unique_rows(self.vrec[:nv, :3].contiguous())
            ids = self.vrec[:nv, 3].contiguous().view(torch.int32).to(torch.int64)
            self.table[ids] = rank
            if faces is not None:
                faces = self.faces(again=True)
                host = _download(self.tot)
        elif not slab:
            COUNTERS["mc3_exact"] += 1
        if faces is not None:
            self.faces_final = self.trim(host, faces, count=not slab)
        return self


def _mc3_caps(hint):
    """Buffer sizes of the hinted chain (last counts + 25 %), or None when they leave the 32-bit index range."""
    if not hint:
        return None
    cap, cap_v, cap_f = (int(h * 1.25) + 4096 for h in hint)
    if cap < LIST_LIMIT and cap < 2 ** 29 and cap_v < MESH_LIMIT and cap_f < MESH_LIMIT:
        return cap, cap_v, cap_f
    return None


def mc3_hint_ready(f: Field, z_offset=0):
    """Would mc3_vertices(f, ..., z_offset) run from size hints (no count read before everything is enqueued)?"""
    return bool(NA_HINTS and _mc3_caps(_MC3_HINT.get((f.Nz, f.Ny, f.Nx, int(z_offset)))))


def mc3_vertices(f: Field, slice_depths, mm_per_pixel_y, mm_per_pixel_x, add_padding=True, z_offset=0, with_faces=True,
                 z_top=None, defer=False, tot=None):
    """surface_extractor.py:55-65 + :82-113 + the vertex half of :115-126 for a manifold=True field at level 0.5: one Mc3Surface
    (see there for z_offset, z_top, tot and the states) driven as far as the caller asks -> it, or None where the reference
    returns None.  With a size hint for the geometry the whole chain -- and with_faces: the triangles -- is enqueued before any
    count is known, and ONE download follows:
      defer=False                    the counters are read here: the surface comes back resolved.
      defer=True, with_faces=True    their download has been started: the surface is `deferred` and .finish() resolves it, so a
                                     caller with several stacks can enqueue the next pass first (bench.py, extract_surface_submit).
      defer=True, with_faces=False   nothing is read: the surface is `deferred`, the caller downloads `tot` itself and calls
                                     .adopt() (slab.SlabJob; rows / table have the capacities cap_v / 4 cap).
    Without a hint the chain runs with exact sizes, one host read per stage, and comes back resolved (`deferred` stays False)."""
    if min(f.Nz, f.Ny, f.Nx) < 2:
        return None
    m = Mc3Surface(f, slice_depths, mm_per_pixel_y, mm_per_pixel_x, add_padding, z_offset, z_top, tot)
    m.classify()
    caps = _mc3_caps(_MC3_HINT.get(m.hint_key)) if NA_HINTS else None
    if not caps:
        return m.resolve(None, None, with_faces)
    m.enqueue(*caps)
    if defer and not with_faces:
        m.deferred = True
        return m
    faces = m.faces() if with_faces else None
    if defer:
        m.start_counters(faces)
        return m
    return m.resolve(_download(m.tot), faces, with_faces)


def mesh_volume_area(verts: torch.Tensor, faces: torch.Tensor):
    """calculate_mesh_volume / calculate_surface_area (surface_extractor.py:128-149) in one pass."""
    out = torch.zeros(2, dtype=torch.float64, device=verts.device)
    if faces.shape[0]:
        _lib.check(_lib.lib().tomo_mesh_volume_area(_p(verts.contiguous()), _p(faces.contiguous()), faces.shape[0],
                                                    _p(out), _stream()), "tomo_mesh_volume_area")
    vol, area = out.cpu().tolist()
    return abs(vol), area


def ellipsoid_mask(nz, ny, nx, device, z0=0, z1=None):
    """Synthetic ellipsoid stack of SURVEY.md 8(d), generated on the device in float64 (bit-identical to the
    NumPy formula used for the golden hashes).  Optionally only the slab z0 <= z < z1."""
    z1 = nz if z1 is None else z1
    cx, cy, cz = (nx - 1) / 2.0, (ny - 1) / 2.0, (nz - 1) / 2.0
    ax, ay, az = 0.42 * nx, 0.40 * ny, 0.45 * nz
    x = torch.arange(nx, dtype=torch.float64, device=device)[None, :]
    y = torch.arange(ny, dtype=torch.float64, device=device)[:, None]
    ex = ((x - cx) / ax) ** 2
    ey = ((y - cy) / ay) ** 2
    exy = (ex + ey)[None]
    z = torch.arange(z0, z1, dtype=torch.float64, device=device)[:, None, None]
    ez = ((z - cz) / az) ** 2
    out = torch.empty((z1 - z0, ny, nx), dtype=torch.bool, device=device)
    step = max(1, (1 << 26) // (ny * nx))
    for a in range(0, z1 - z0, step):
        b = min(z1 - z0, a + step)
        out[a:b] = (exy + ez[a:b]) <= 1.0
    return out


# ---- GLB export (glb_exporter.py of the reference) ----------------------------------------------------
# The orientation contract is written out in include/tomo_hip.h (trimesh's fix_normals(multibody=False) restated), and below
# it the normals contract of the optional NORMAL attribute.
GLB_MAX_BYTES = (1 << 32) - 1          # the GLB header's length field


def _layer_bounds(dtype, slice_depths, first, last, thickness):
    """(start1, end1, enable1, start2, end2, enable2) of glb_exporter.py:71-89, computed from np.cumsum exactly as there.  Each
    bound is rounded to the type this NumPy compares a `dtype` column with it in (NumPy 1.x: float32 for a float32 column,
    NumPy 2: float64), so that float64 comparisons on the device give NumPy's answer bit for bit."""
    cum = np.cumsum(np.concatenate([[0], slice_depths]))
    probe = np.zeros(1, dtype)
    out = []
    for idx in (first, last):
        if idx < len(cum) - 1:
            s = cum[idx]
            e = s + thickness
            out += [float(np.result_type(probe, s).type(s)), float(np.result_type(probe, e).type(e)), 1]
        else:
            out += [0.0, 0.0, 0]
    return out


def layer_colors(verts: torch.Tensor, slice_depths, first_section1_slice, last_section1_slice, highlight_thickness_mm=1.0,
                 out: torch.Tensor = None) -> torch.Tensor:
    """create_layer_colors (glb_exporter.py:52-91) of device vertices (V, >=1), float32 or float64: RGBA uint8 (V, 4) on the
    device, bit-exact against the reference (column 0 is the depth)."""
    if verts.dtype not in (torch.float32, torch.float64) or verts.dim() != 2:
        raise TypeError("layer_colors: vertices must be a (V, 3) float32 or float64 tensor")
    nv = verts.shape[0]
    if out is None:
        out = torch.empty((nv, 4), dtype=torch.uint8, device=verts.device)
    b = _layer_bounds(np.float64 if verts.dtype == torch.float64 else np.float32, slice_depths, first_section1_slice,
                      last_section1_slice, highlight_thickness_mm)
    _lib.check(_lib.lib().tomo_layer_colors(_p(verts), 1 if verts.dtype == torch.float64 else 0, nv, max(1, verts.stride(0)),
                                            *b, _p(out), _stream()), "tomo_layer_colors")
    return out


def edge_table(faces: torch.Tensor, nv: int):
    """tomo_mesh_edges, enqueued: (table bytes on the device, their number, counters int64 (6,) on the device)."""
    L = _lib.lib()
    nf = faces.shape[0]
    tb = L.tomo_mesh_edge_table_bytes(nf)
    if tb < 0:
        raise ValueError("too many faces for the edge table: %d" % nf)
    table = torch.empty(tb, dtype=torch.uint8, device=faces.device)
    counters = torch.empty(6, dtype=torch.int64, device=faces.device)
    _lib.check(L.tomo_mesh_edges(_p(faces), nf, nv, _p(table), tb, _p(counters), _stream()), "tomo_mesh_edges")
    return table, tb, counters


def _edge_stats(faces: torch.Tensor, nv: int):
    """Rules 1-2 of the orientation contract: (flip uint8 (F,) or None, stats).  The edge table decides; the union-find runs
    only when some manifold edge has both faces running it the same way."""
    L = _lib.lib()
    nf = faces.shape[0]
    dev = faces.device
    table, tb, counters = edge_table(faces, nv)
    c = counters.cpu().tolist()
    if c[4]:
        raise IndexError("%d faces have an index outside [0, %d)" % (c[4], nv))
    stats = {"boundary_edges": c[0], "manifold_edges": c[1], "non_manifold_edges": c[2], "inconsistent_pairs": c[3],
             "degenerate_faces": c[5], "components": None, "conflicts": 0, "fast_path": c[3] == 0}
    flip = None
    if c[3]:
        wsb = L.tomo_mesh_orient_workspace_bytes(nf)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        flip = torch.empty(nf, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(L.tomo_mesh_orient(_p(table), tb, nf, _p(ws), wsb, _p(flip), _p(counts), _stream()), "tomo_mesh_orient")
        stats["components"], stats["conflicts"] = counts.cpu().tolist()
    return flip, stats


def _glb_mesh(verts: torch.Tensor, faces: torch.Tensor):
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype not in (torch.float32, torch.float64):
        raise ValueError("vertices must be (V, 3) float32 or float64")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be (F, 3)")
    if faces.shape[0] == 0:
        raise ValueError("no faces")
    if verts.shape[0] >= (1 << 32):
        raise ValueError("%d vertices do not fit 32-bit GLB indices" % verts.shape[0])
    if faces.dtype != torch.int64:
        if faces.dtype.is_floating_point or faces.dtype == torch.bool:
            raise TypeError("faces must be integer")
        faces = faces.to(torch.int64)
    return verts.contiguous(), faces.contiguous()


def orient_faces(verts: torch.Tensor, faces: torch.Tensor):
    """fix_normals on the device (the contract in include/tomo_hip.h): (oriented int64 faces (F, 3), stats).  stats: boundary /
    manifold / non-manifold edges, inconsistent pairs, degenerate faces, components and conflicting components (None and 0 on
    the fast path, where the winding is consistent and no component is formed), fast_path, inverted, signed_volume (of the
    result, columns in the order given)."""
    verts, faces = _glb_mesh(verts, faces)
    L = _lib.lib()
    nv, nf = verts.shape[0], faces.shape[0]
    flip, stats = _edge_stats(faces, nv)
    pos = torch.empty((nv, 3), dtype=torch.float32, device=verts.device)
    scratch = torch.zeros(4, dtype=torch.float64, device=verts.device)       # [0:3] min / max (6 x f32), [3] volume
    st = _stream()
    _lib.check(L.tomo_glb_pack_positions(_p(verts), 1 if verts.dtype == torch.float64 else 0, nv, _p(pos), _p(scratch), st),
               "tomo_glb_pack_positions")
    vol = scratch[3:]
    _lib.check(L.tomo_mesh_signed_volume(_p(pos), _p(faces), nf, _p(flip), _p(vol), st), "tomo_mesh_signed_volume")
    out = torch.empty_like(faces)
    _lib.check(L.tomo_glb_pack_faces(_p(faces), nf, _p(flip), _p(vol), _p(out), 1, st), "tomo_glb_pack_faces")
    v = float(vol.item())
    stats["inverted"] = v < 0
    stats["signed_volume"] = -v if v < 0 else v
    return out, stats


def _vertex_normals_launch(pos_ptr, nv, idx_ptr, idx_i64, nf, normals_ptr, counters_ptr, dev):
    """tomo_mesh_vertex_normals with its workspace (enqueue only; the workspace is handed back to the caching allocator,
    which keeps it for this stream until the kernels are through)."""
    L = _lib.lib()
    wsb = L.tomo_mesh_vertex_normals_workspace_bytes(nv, nf)
    if wsb < 0:
        raise ValueError("the mesh is too large for the vertex-normal lists: %d vertices, %d faces" % (nv, nf))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.tomo_mesh_vertex_normals(pos_ptr, nv, idx_ptr, idx_i64, nf, _p(ws), wsb, normals_ptr, counters_ptr, _stream()),
               "tomo_mesh_vertex_normals")


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, oriented: bool = False, counts: torch.Tensor = None) -> torch.Tensor:
    """Area-weighted vertex normals on the device (the normals contract in include/tomo_hip.h): float32 (V, 3), the same
    bytes on every run.  faces: as given (orient_faces runs first) or, with oriented=True, already oriented -- then an index
    outside [0, V) is not an error here: the face enters no sum and is counted.  counts: an optional int64 (2,) device
    tensor that receives [vertices that got the default (0, 0, 1), faces skipped]; nothing here waits for the device, the
    caller reads it when it wants to."""
    verts, faces = _glb_mesh(verts, faces)
    if not oriented:
        faces, _ = orient_faces(verts, faces)
    nv, nf = verts.shape[0], faces.shape[0]
    if nv == 0:
        raise ValueError("no vertices")
    pos = verts if verts.dtype == torch.float32 else verts.to(torch.float32)      # POSITION as the file stores it
    if counts is None:
        counts = torch.empty(2, dtype=torch.int64, device=verts.device)
    elif counts.dtype != torch.int64 or counts.numel() != 2 or not counts.is_contiguous() or counts.device != verts.device:
        raise ValueError("counts must be a contiguous int64 (2,) tensor on the mesh's device")
    normals = torch.empty((nv, 3), dtype=torch.float32, device=verts.device)
    _vertex_normals_launch(_p(pos), nv, _p(faces), 1, nf, _p(normals), _p(counts), verts.device)
    return normals


@dataclass
class GlbPacked:
    """The binary chunk of a GLB on the device (`buf[:bin_len]`), with min / max of POSITION, the signed volume and (with
    normals) the normals' two counters in a tail."""
    buf: torch.Tensor
    nv: int
    nf: int
    color_cols: int          # 0 (no colours), 3 or 4
    bin_len: int
    tail: int
    stats: dict
    normals: bool = False


def glb_layout_bytes(nv: int, nf: int, color_cols: int = 0, normals: bool = False) -> int:
    """Bytes of the binary chunk: POSITION (12 V) | indices (12 F) | COLOR_0 (4 V, one 4-byte element per vertex) | NORMAL
    (12 V, last: the blocks before it sit where they sit without it)."""
    return 12 * nv + 12 * nf + (4 * nv if color_cols else 0) + (12 * nv if normals else 0)


def glb_check_sizes(nv: int, nf: int, color_cols: int = 0, normals: bool = False):
    """The limits a GLB of this mesh must fit, checked from the shapes alone (before anything is copied)."""
    if nf == 0:
        raise ValueError("no faces")
    if nv >= (1 << 32):
        raise ValueError("%d vertices do not fit 32-bit GLB indices" % nv)
    if color_cols not in (0, 3, 4):
        raise ValueError("vertex colours must be uint8 (V, 3) or (V, 4)")
    if 12 + 8 + 8 + 1024 + glb_layout_bytes(nv, nf, color_cols, normals) > GLB_MAX_BYTES:
        raise ValueError("the GLB would exceed the 4 GiB length field (%d vertices, %d faces)" % (nv, nf))


def glb_pack(verts: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor = None, normals: bool = False) -> GlbPacked:
    """Steps 2-3 of the export on the device: edge table, orientation (fast path or union-find), inversion decision, and the
    binary chunk -- positions, oriented uint32 indices, colours and (normals=True) the vertex normals of the normals
    contract, computed from the chunk's own POSITION and index blocks -- packed in one device buffer."""
    verts, faces = _glb_mesh(verts, faces)
    nv, nf = verts.shape[0], faces.shape[0]
    cc = 0
    if colors is not None:
        if colors.dtype != torch.uint8 or colors.dim() != 2 or colors.shape[0] != nv or colors.shape[1] not in (3, 4):
            raise ValueError("vertex colours must be uint8 (V, 3) or (V, 4)")
        cc = colors.shape[1]
    normals = bool(normals)
    glb_check_sizes(nv, nf, cc, normals)
    L = _lib.lib()
    flip, stats = _edge_stats(faces, nv)
    bin_len = glb_layout_bytes(nv, nf, cc, normals)
    tail = (bin_len + 7) & ~7
    buf = torch.empty(tail + (48 if normals else 32), dtype=torch.uint8, device=verts.device)
    buf[tail + 24:].zero_()
    base, st = buf.data_ptr(), _stream()
    _lib.check(L.tomo_glb_pack_positions(_p(verts), 1 if verts.dtype == torch.float64 else 0, nv, base, base + tail, st),
               "tomo_glb_pack_positions")
    _lib.check(L.tomo_mesh_signed_volume(base, _p(faces), nf, _p(flip), base + tail + 24, st), "tomo_mesh_signed_volume")
    _lib.check(L.tomo_glb_pack_faces(_p(faces), nf, _p(flip), base + tail + 24, base + 12 * nv, 0, st), "tomo_glb_pack_faces")
    if cc:
        cv = buf[12 * nv + 12 * nf: 16 * nv + 12 * nf].view(nv, 4)
        cv[:, :cc].copy_(colors)
        if cc == 3:
            cv[:, 3].zero_()
    if normals:
        _vertex_normals_launch(base, nv, base + 12 * nv, 0, nf, base + bin_len - 12 * nv, base + tail + 32, verts.device)
    return GlbPacked(buf, nv, nf, cc, bin_len, tail, stats, normals)


def glb_download(p: GlbPacked) -> np.ndarray:
    """Step 4: ONE copy of the binary chunk (and its tail) into page-locked memory."""
    host = torch.empty(p.buf.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(p.buf, non_blocking=True)
    torch.cuda.current_stream(p.buf.device).synchronize()
    return host.numpy()


def glb_json(p: GlbPacked, minmax) -> dict:
    return glb_json_counts(p.nv, p.nf, p.color_cols, p.normals, minmax)


def glb_json_counts(nv: int, nf: int, color_cols: int, normals: bool, minmax) -> dict:
    """The JSON chunk's content from the counts and POSITION's min / max alone (the Z-slab job forms it on every rank from
    the global counts)."""
    bin_len = glb_layout_bytes(nv, nf, color_cols, normals)
    attrs = {"POSITION": 0}
    views = [{"buffer": 0, "byteOffset": 0, "byteLength": 12 * nv, "target": 34962},
             {"buffer": 0, "byteOffset": 12 * nv, "byteLength": 12 * nf, "target": 34963}]
    accessors = [{"bufferView": 0, "componentType": 5126, "count": nv, "type": "VEC3",
                  "min": [float(x) for x in minmax[:3]], "max": [float(x) for x in minmax[3:]]},
                 {"bufferView": 1, "componentType": 5125, "count": 3 * nf, "type": "SCALAR"}]
    if color_cols:
        attrs["COLOR_0"] = 2
        views.append({"buffer": 0, "byteOffset": 12 * nv + 12 * nf, "byteLength": 4 * nv, "byteStride": 4, "target": 34962})
        accessors.append({"bufferView": 2, "componentType": 5121, "normalized": True, "count": nv,
                          "type": "VEC4" if color_cols == 4 else "VEC3"})
    if normals:
        attrs["NORMAL"] = len(accessors)
        views.append({"buffer": 0, "byteOffset": bin_len - 12 * nv, "byteLength": 12 * nv, "target": 34962})
        accessors.append({"bufferView": len(views) - 1, "componentType": 5126, "count": nv, "type": "VEC3"})
    return {"asset": {"version": "2.0", "generator": "tomography_3d_reconstructor_amd"},
            "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
            "meshes": [{"primitives": [{"attributes": attrs, "indices": 1, "mode": 4}]}],
            "buffers": [{"byteLength": bin_len}], "bufferViews": views, "accessors": accessors}


def glb_head(nv: int, nf: int, color_cols: int, normals: bool, minmax):
    """Everything in front of the binary chunk's data -- the 12-byte header, the JSON chunk (padded with spaces) and the
    binary chunk's 8-byte header -- and the file's total length: (bytes, total).  Raises like glb_write."""
    import json
    import struct
    if not np.isfinite(np.asarray(minmax, dtype=np.float32)).all():
        raise ValueError("vertex positions are not finite")
    bin_len = glb_layout_bytes(nv, nf, color_cols, normals)
    js = json.dumps(glb_json_counts(nv, nf, color_cols, normals, minmax), separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    total = 12 + 8 + len(js) + 8 + bin_len
    if total > GLB_MAX_BYTES:
        raise ValueError("the GLB would exceed the 4 GiB length field (%d bytes)" % total)
    return (struct.pack("<4sII", b"glTF", 2, total) + struct.pack("<II", len(js), 0x4E4F534A) + js
            + struct.pack("<II", bin_len, 0x004E4942)), total


def glb_write(path, p: GlbPacked, host: np.ndarray) -> dict:
    """Step 5: the JSON chunk (padded with spaces) and the binary chunk (padded with zeros -- its length is already a
    multiple of 4) behind the 12-byte header.  Returns the stats, `inverted` and `signed_volume` filled in."""
    minmax = host[p.tail: p.tail + 24].view(np.float32)
    vol = float(host[p.tail + 24: p.tail + 32].view(np.float64)[0])
    head, _ = glb_head(p.nv, p.nf, p.color_cols, p.normals, minmax)
    with open(path, "wb") as fh:
        fh.write(head)
        fh.write(memoryview(host)[: p.bin_len])
    stats = dict(p.stats)
    stats["inverted"] = vol < 0
    stats["signed_volume"] = -vol if vol < 0 else vol
    if p.normals:
        stats["normals_defaulted"] = int(host[p.tail + 32: p.tail + 40].view(np.uint64)[0])
    return stats


def export_glb(path, verts: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor = None, normals: bool = False) -> dict:
    """GLBExporter.export_to_glb for device tensors: orient (the contract in include/tomo_hip.h), pack, download once, write.
    Returns the orientation stats (see orient_faces); with normals=True the file carries NORMAL (the normals contract) and
    the stats `normals_defaulted`, the number of vertices that got the default (0, 0, 1)."""
    p = glb_pack(verts, faces, colors, normals)
    return glb_write(path, p, glb_download(p))
