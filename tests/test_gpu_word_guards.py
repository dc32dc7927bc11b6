"""GPU tier: the word passes and the row writers that share one front and one selected-row guard in csrc/cc_runs.h --
tomo_cc_value_max, tomo_cc_value_first, tomo_cc_value_rows, tomo_profile_stats, tomo_profile_where, tomo_profile_rows,
tomo_cc_level_hist and tomo_thin_count.  What they give per component is compared with tests/topology_reference.py's labelling and
NumPy, never with a second run; a table, a selection, a run table or a histogram that does not fit is flagged in the counter block
and nothing is written outside a table.  Every capacity that is wrong on purpose is SMALLER than the buffer it describes, and every
buffer is allocated at its full size plus padding: no launch here can reach outside an allocation, whether a guard works or not."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 77
PAD = 64
MIN_VOXELS = 8                                                   # the selection of the row writers: slot[c] != c on the noise
LEVELS = 3
# noise: two words a row with a ragged last one, 1318 components, 24 rows whose run crosses bit 63 -> 64, 576 waves; straddle: one
# word a row, a wave's rows lie in several slices; solid: whole-word runs, a carry into words 1 and 2, ONE component, so every
# word competes for one address
VOLUMES = {"noise": lambda: T.noise(0.3, (12, 24, 70), seed=41), "straddle": T.straddle,
           "solid": lambda: np.ones((4, 6, 130), dtype=bool)}
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _first_where(hit, flat, n):
    """the lowest flat index per component 1..n among the voxels `hit`"""
    idx = np.nonzero(hit)[0]
    first = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, flat[idx], idx)
    return first[1:]


def stats(flat, vals, n, skip=None):
    """lo, hi (float32 bit patterns), sum of rint(v * 65536), the first index of lo and of hi per component 1..n; skip: a voxel
    that does not count.  Components without a counted voxel keep what the entry points clear their arrays to."""
    inside = flat > 0
    if skip is not None:
        inside = inside.copy()
        inside[skip] = False
    lo = np.full(n + 1, np.inf)
    hi = np.full(n + 1, -np.inf)
    np.minimum.at(lo, flat[inside], vals[inside])
    np.maximum.at(hi, flat[inside], vals[inside])
    total = np.zeros(n + 1, dtype=np.int64)
    np.add.at(total, flat[inside], np.rint(vals[inside].astype(np.float64) * 65536.0).astype(np.int64))
    lo_first = _first_where(inside & (vals == lo[flat]), flat, n)
    hi_first = _first_where(inside & (vals == hi[flat]), flat, n)
    seen = np.isfinite(lo[1:])
    lo_bits = np.where(seen, np.where(seen, lo[1:], 0).astype(np.float32).view(np.uint32), 0xffffffff).astype(np.uint32)
    hi_bits = np.where(seen, np.where(seen, hi[1:], 0).astype(np.float32).view(np.uint32), 0).astype(np.uint32)
    return lo_bits, hi_bits, total[1:], np.where(seen, lo_first, -1), np.where(seen, hi_first, -1)


def reference(name):
    """Everything NumPy says about one volume, computed once and left unchanged."""
    if name not in _cache:
        v = np.ascontiguousarray(VOLUMES[name]())
        labels, n = T.label(v, 6)
        flat = labels.reshape(-1).astype(np.int64)
        vals = np.random.default_rng(7).integers(0, 8, v.shape).astype(np.float32)
        level = np.random.default_rng(11).integers(0, LEVELS + 1, v.shape).astype(np.int32)
        other = T.noise(0.5, v.shape, seed=43)
        sizes = np.bincount(flat, minlength=n + 1)[1:]
        per = np.zeros((n + 1, v.shape[0], LEVELS + 1), dtype=np.int64)      # voxels per component, slice and level
        z = np.repeat(np.arange(v.shape[0]), v.shape[1] * v.shape[2])
        np.add.at(per, (flat, z, level.reshape(-1)), 1)
        lo, hi, total, lo_first, hi_first = stats(flat, vals.reshape(-1), n)
        attained = np.bincount(flat[(flat > 0) & (vals.reshape(-1) == hi.view(np.float32)[np.maximum(flat - 1, 0)])], minlength=n + 1)[1:]
        _cache[name] = dict(v=v, n=n, flat=flat, vals=vals, level=level, other=other, sizes=sizes, per=per[1:], lo=lo, hi=hi, sum=total,
                            lo_first=lo_first, hi_first=hi_first, chosen=np.nonzero(sizes >= MIN_VOXELS)[0],
                            tied=int(((attained > 1) & (sizes >= MIN_VOXELS)).sum()),
                            under=np.bincount(flat[other.reshape(-1) & (flat > 0)], minlength=n + 1)[1:])
    return _cache[name]


def padded(n, dtype, dev):
    return torch.full((n + PAD,), FILL, dtype=dtype, device=dev)


def fresh(name, dev):
    """-> (a fresh ComponentRuns, its selection of the components of at least MIN_VOXELS voxels, the device copies of the maps)"""
    ref = reference(name)
    v = ref["v"]
    cr = pipeline.ComponentRuns(pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape), 6)
    picked = cr.select(MIN_VOXELS)
    assert picked is not None and picked.table.shape[0] == ref["n"] and picked.m == len(ref["chosen"])
    cr.vals = torch.from_numpy(ref["vals"]).to(dev)
    cr.level = torch.from_numpy(ref["level"]).to(dev)
    cr.other = torch.from_numpy(C.pack(ref["other"])).to(dev)
    return cr, picked


def head(cr, cap_runs=None):
    """the leading arguments of every word pass: bits, geometry, run tables (cap_runs: the capacity that is wrong on purpose), tot"""
    row_off, runs, parent, rank = cr._tables()
    return (_p(cr.bits), *cr.vol.shape, row_off, runs if cap_runs is None else cap_runs, parent, rank, _p(cr.tot))


def flags(cr):
    return int(pipeline._download(cr.tot)[2])


def host(t):
    return t.cpu().numpy()


def topo_of(n):
    """what tomo_cc_topology_rows copies: any int64 (n, 3) will do, the writer computes nothing"""
    return np.random.default_rng(13).integers(-5, 50, (n, 3)).astype(np.int64)


class Buffers:
    """every array an entry point here reads or writes, over n components, m rows and `total` histogram entries: padded, filled"""

    def __init__(self, n, m, total, dev):
        self.n, self.m, self.total = n, m, total
        self.best, self.lo, self.hi = (padded(n, torch.int32, dev) for _ in range(3))
        self.first, self.sum, self.lo_first, self.hi_first = (padded(n, torch.int64, dev) for _ in range(4))
        self.rows4, self.rows7, self.rows5 = (padded(k * m, torch.int64, dev) for k in (4, 7, 5))
        self.counts = padded(3 * m, torch.int64, dev)
        self.hist = padded((LEVELS + 1) * total, torch.int64, dev)
        self.topo = torch.from_numpy(topo_of(n)).to(dev)             # an input: never written

    def tensors(self):
        return {k: t for k, t in vars(self).items() if isinstance(t, torch.Tensor) and k != "topo"}


WORD = ("tomo_cc_value_max", "tomo_cc_value_first", "tomo_profile_stats", "tomo_profile_where")
ROWS = ("tomo_cc_value_rows", "tomo_profile_rows", "tomo_cc_topology_rows")
# what an entry point clears before its launch: (array, value); the level histogram: hist_cap entries of LEVELS + 1 words
CLEARS = {"tomo_cc_value_max": (("best", 0),), "tomo_cc_value_first": (("first", -1),),
          "tomo_profile_stats": (("lo", -1), ("hi", 0), ("sum", 0)), "tomo_profile_where": (("lo_first", -1), ("hi_first", -1))}


def call(entry, cr, picked, b, vals=None, **wrong):
    """ONE entry point with the capacities that fit, but for the ones in `wrong`"""
    k = dict(cap=b.n, cap_sel=b.m, cap_runs=cr.runs, hist_cap=b.total)
    assert set(wrong) <= set(k)
    k.update(wrong)
    L, st, h = _lib.lib(), _stream(), head(cr, k["cap_runs"])
    v = _p(cr.vals if vals is None else vals)
    rows = (k["cap"], _p(cr.tot), _p(picked.sel), _p(picked.slot))
    if entry == "tomo_cc_value_max":
        code = L.tomo_cc_value_max(*h, v, None, _p(b.best), k["cap"], st)
    elif entry == "tomo_cc_value_first":
        code = L.tomo_cc_value_first(*h, v, None, _p(b.best), _p(b.first), k["cap"], st)
    elif entry == "tomo_profile_stats":
        code = L.tomo_profile_stats(*h, v, _p(b.lo), _p(b.hi), _p(b.sum), k["cap"], st)
    elif entry == "tomo_profile_where":
        code = L.tomo_profile_where(*h, v, _p(b.lo), _p(b.hi), _p(b.lo_first), _p(b.hi_first), k["cap"], st)
    elif entry == "tomo_cc_value_rows":
        code = L.tomo_cc_value_rows(_p(picked.table), _p(b.best), _p(b.first), *rows, _p(b.rows4), k["cap_sel"], st)
    elif entry == "tomo_profile_rows":
        code = L.tomo_profile_rows(_p(picked.table), _p(b.lo), _p(b.hi), _p(b.sum), _p(b.lo_first), _p(b.hi_first), *rows, _p(b.rows7),
                                   k["cap_sel"], st)
    elif entry == "tomo_cc_topology_rows":
        code = L.tomo_cc_topology_rows(_p(picked.table), _p(b.topo), *rows, _p(b.rows5), k["cap_sel"], st)
    elif entry == "tomo_cc_level_hist":
        hh = list(cr.hist_head(picked))
        assert hh[5] == cr.runs
        hh[5] = k["cap_runs"]
        code = L.tomo_cc_level_hist(*hh, _p(b.hist), k["hist_cap"], _p(cr.level), LEVELS, st)
    else:
        assert entry == "tomo_thin_count"
        code = L.tomo_thin_count(*h, _p(cr.other), _p(picked.sel), _p(picked.slot), _p(b.counts), 1, 3, k["cap"], k["cap_sel"], st)
    _lib.check(code, entry)


def bits_of(t, n):
    return host(t)[:n].view(np.uint32)


def kept(t, n):
    """the padding behind the first n entries is intact"""
    return bool(t[n:].eq(FILL).all())


def only_cleared(b, cleared):
    """cleared: {array: (entries, value)} -- those entries hold the value, everything else in every buffer is the fill"""
    for name, t in b.tensors().items():
        k, value = cleared.get(name, (0, 0))
        if not (bool(t[:k].eq(value).all()) and kept(t, k)):
            return False
    return True


@pytest.mark.parametrize("name", list(VOLUMES))
def test_the_passes_give_what_numpy_gives_and_leave_the_padding(dev, name):
    ref = reference(name)
    v, n, chosen = ref["v"], ref["n"], ref["chosen"]
    m = len(chosen)
    assert ref["tied"] >= 1                                      # the lowest flat index among equals is exercised
    crossing = int((v[:, :, 63] & v[:, :, 64]).sum()) if v.shape[2] > 64 else 0     # rows whose run crosses from word 0 into word 1
    if name == "noise":
        assert (n, ref["tied"], int(v[:, :, 64:].sum()), crossing) == (1318, 117, 542, 24) and len(chosen) == 155
    if name == "solid":
        assert crossing == v.shape[0] * v.shape[1] and v[:, :, 127].all() and v[:, :, 128].all()       # a carry into words 1 and 2
    cr, picked = fresh(name, dev)
    total = picked.total
    b = Buffers(n, m, total, dev)
    for entry in WORD + ROWS + ("tomo_cc_level_hist", "tomo_thin_count"):
        call(entry, cr, picked, b)
        assert flags(cr) == 0, entry
    assert np.array_equal(bits_of(b.best, n), ref["hi"]) and np.array_equal(host(b.first)[:n], ref["hi_first"])
    assert np.array_equal(bits_of(b.lo, n), ref["lo"]) and np.array_equal(bits_of(b.hi, n), ref["hi"])
    assert np.array_equal(host(b.sum)[:n], ref["sum"])
    assert np.array_equal(host(b.lo_first)[:n], ref["lo_first"]) and np.array_equal(host(b.hi_first)[:n], ref["hi_first"])
    for t in (b.best, b.first, b.lo, b.hi, b.sum, b.lo_first, b.hi_first):
        assert kept(t, n)

    label, voxels = chosen + 1, ref["sizes"][chosen]
    want4 = np.stack([label, voxels, ref["hi"][chosen], ref["hi_first"][chosen]], axis=1)
    want7 = np.stack([label, voxels, ref["lo"][chosen], ref["hi"][chosen], ref["sum"][chosen], ref["lo_first"][chosen],
                      ref["hi_first"][chosen]], axis=1)
    want5 = np.concatenate([np.stack([label, voxels], axis=1), topo_of(n)[chosen]], axis=1)
    for rows, want in ((b.rows4, want4), (b.rows7, want7), (b.rows5, want5)):
        k = want.size
        assert np.array_equal(host(rows)[:k].reshape(want.shape), want) and kept(rows, k)

    got = host(b.hist)[:(LEVELS + 1) * total].reshape(total, LEVELS + 1)
    off, box = host(picked.off), host(picked.table)[:, 1:3]
    assert off[-1] == total and kept(b.hist, (LEVELS + 1) * total)
    for c in chosen:
        assert np.array_equal(got[off[c]:off[c + 1]], ref["per"][c, box[c, 0]:box[c, 1] + 1]), (c, box[c])
    assert got.sum() == ref["sizes"][chosen].sum()

    want = np.full((m, 3), FILL, dtype=np.int64)
    want[:, 1] += ref["under"][chosen]
    assert np.array_equal(host(b.counts)[:3 * m].reshape(m, 3), want) and kept(b.counts, 3 * m)


@pytest.mark.parametrize("name", ["noise", "straddle"])
def test_the_guards_flag_instead_of_writing_outside_a_table(dev, name):
    ref = reference(name)
    n, m = ref["n"], len(ref["chosen"])
    assert n > 1 and m > 1

    def guarded(entry, **wrong):
        """one entry point on a fresh ComponentRuns and fresh buffers -> (the flag word it leaves, the buffers)"""
        cr, picked = fresh(name, dev)
        assert picked.total > 1
        b = Buffers(n, m, picked.total, dev)
        call(entry, cr, picked, b, **wrong)
        return flags(cr), b

    # tables one component short: bit 1; entry n - 1 and the padding keep the fill, nothing but the clearing is written
    for entry in WORD:
        flag, b = guarded(entry, cap=n - 1)
        assert flag == 2 and only_cleared(b, {a: (n - 1, value) for a, value in CLEARS[entry]}), entry
    for entry in ROWS + ("tomo_thin_count",):
        flag, b = guarded(entry, cap=n - 1)
        assert flag == 2 and only_cleared(b, {}), entry

    # a selection one row short: bit 1, nothing is written
    for entry in ROWS + ("tomo_thin_count",):
        flag, b = guarded(entry, cap_sel=m - 1)
        assert flag == 2 and only_cleared(b, {}), entry

    # run tables one run short: bit 2 for every run, no entry changes from its cleared value
    runs = fresh(name, dev)[0].runs
    for entry in WORD:
        flag, b = guarded(entry, cap_runs=runs - 1)
        assert flag == 4 and only_cleared(b, {a: (n, value) for a, value in CLEARS[entry]}), entry
    flag, b = guarded("tomo_cc_level_hist", cap_runs=runs - 1)
    assert flag == 4 and only_cleared(b, {"hist": ((LEVELS + 1) * b.total, 0)})
    flag, b = guarded("tomo_thin_count", cap_runs=runs - 1)
    assert flag == 4 and only_cleared(b, {})

    # a level histogram one entry short: bit 1, the entries in front are zero, the entries behind keep their fill
    flag, b = guarded("tomo_cc_level_hist", hist_cap=fresh(name, dev)[1].total - 1)
    assert flag == 2 and only_cleared(b, {"hist": ((LEVELS + 1) * (b.total - 1), 0)})

    # one value that is not admitted on a set voxel: bit 3 alone, that voxel is left out and every other row is as before
    big = int(np.argmax(ref["sizes"]))
    at = int(np.nonzero(ref["flat"] == big + 1)[0][0])
    vals = ref["vals"].copy()
    vals.reshape(-1)[at] = -1.0
    flag, b = guarded("tomo_profile_stats", vals=torch.from_numpy(vals).to(dev))
    assert flag == pipeline.PROFILE_F_VALUE == 8
    others = np.arange(n) != big
    assert np.array_equal(bits_of(b.lo, n)[others], ref["lo"][others]) and np.array_equal(bits_of(b.hi, n)[others], ref["hi"][others])
    assert np.array_equal(host(b.sum)[:n][others], ref["sum"][others])
    lo, hi, total_q, _, _ = stats(ref["flat"], ref["vals"].reshape(-1), n, skip=at)
    assert (bits_of(b.lo, n)[big], bits_of(b.hi, n)[big], host(b.sum)[big]) == (lo[big], hi[big], total_q[big])
    assert kept(b.lo, n) and kept(b.hi, n) and kept(b.sum, n)
