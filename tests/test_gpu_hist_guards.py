"""GPU tier: the guards of the slice histogram passes that share the run walk with the surface and the breadth pass, whose own
guard tests are in tests/test_gpu_surface.py and tests/test_gpu_breadth.py: tomo_cc_zhist, tomo_cc_moment_hist
(csrc/component_measures.hip) and tomo_branch_hist (csrc/branches.hip).  A histogram, a run table or a box that does not fit is
flagged in the counter block and nothing is written outside a table.  The voxels per component and slice that the first word of an
entry of tomo_cc_zhist and tomo_cc_moment_hist holds are compared with SciPy's labelling, never with a second run."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import test_gpu_branches as G  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline  # noqa: E402
from tomography_3d_reconstructor_amd.pipeline import _p, _stream  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 77
WORDS = {"tomo_cc_zhist": 1, "tomo_cc_moment_hist": pipeline.MOMENT_SUMS, "tomo_branch_hist": pipeline.SURFACE_COUNTERS}
# noise: 288 rows in two workgroups, ny < 64 so that a wave's rows lie in several slices, two words a row with a ragged last one,
# hundreds of components; straddle: ny = 5, a wave's rows lie in 13 slices; edges, noise10: the volumes of the branch tests
VOLUMES = {"noise": lambda: T.noise(0.3, (12, 24, 70), seed=41), "straddle": T.straddle,
           "edges": lambda: G.volume("edges"), "noise10": lambda: G.volume("noise10")}
CASES = [(entry, name) for entry in ("tomo_cc_zhist", "tomo_cc_moment_hist") for name in ("noise", "straddle")]
CASES += [("tomo_branch_hist", name) for name in ("edges", "noise10")]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def volume(name):
    if name not in _cache:
        _cache[name] = VOLUMES[name]()
    return _cache[name]


def voxels_per_slice(name):
    """int64 (n, nz): the voxels of component c + 1 in slice z under connectivity 6, computed once and left unchanged."""
    if ("per", name) not in _cache:
        v = volume(name)
        labels, n = T.label(v, 6)
        per = np.zeros((n + 1, v.shape[0]), dtype=np.int64)
        for z in range(v.shape[0]):
            per[:, z] = np.bincount(labels[z].reshape(-1), minlength=n + 1)
        _cache["per", name] = per[1:]
    return _cache["per", name]


def runs_of(entry, name, dev):
    """-> (a fresh ComponentRuns of the volume the entry point walks, what the entry point takes behind the capacity)."""
    v = volume(name)
    vol = pipeline.BitVolume(torch.from_numpy(C.pack(v)).to(dev), v.shape)
    if entry != "tomo_branch_hist":
        return pipeline.ComponentRuns(vol, 6), ()
    regular, nodes = (pipeline.BitVolume(torch.empty_like(vol.bits), v.shape) for _ in range(2))
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().tomo_branch_split(_p(vol.bits), *v.shape, _p(regular.bits), _p(nodes.bits), _p(counters), _stream()),
               "tomo_branch_split")
    cr = pipeline.ComponentRuns(regular, 26)
    cr.whole = vol                                               # kept alive with the tables
    return cr, (_p(vol.bits),)


@pytest.mark.parametrize("entry,name", CASES)
def test_the_guards_flag_instead_of_writing_outside_a_table(dev, entry, name):
    fn, st, W = getattr(_lib.lib(), entry), _stream(), WORDS[entry]
    counts = entry != "tomo_branch_hist"

    # a histogram one entry short: bit 1, the entries in front are zero, the entries behind keep their fill
    cr, extra = runs_of(entry, name, dev)
    picked = cr.select(0, False)
    n, total = picked.table.shape[0], picked.total
    assert n > 1 and total > n                                   # some box spans more than one slice
    hist = torch.full((W * total,), FILL, dtype=torch.int64, device=dev)
    _lib.check(fn(*cr.hist_head(picked), _p(hist), total - 1, *extra, st), entry)
    assert pipeline._download(cr.tot)[2] == 2
    assert hist[:W * (total - 1)].eq(0).all() and hist[W * (total - 1):].eq(FILL).all()

    # the histogram that fits: no flag, and the voxels per slice are SciPy's
    cr, extra = runs_of(entry, name, dev)
    picked = cr.select(0, False)
    padded = torch.full((W * total + 64,), FILL, dtype=torch.int64, device=dev)
    _lib.check(fn(*cr.hist_head(picked), _p(padded), total, *extra, st), entry)
    assert pipeline._download(cr.tot)[2] == 0
    assert padded[W * total:].eq(FILL).all()
    off = picked.off.cpu().numpy()
    box = picked.table.cpu().numpy()[:, 1:3]
    assert off[-1] == total
    if counts:
        per = voxels_per_slice(name)
        assert n == len(per)
        got = padded[:W * total].cpu().numpy().reshape(total, W)
        for c in range(n):
            assert np.array_equal(got[off[c]:off[c + 1], 0], per[c, box[c, 0]:box[c, 1] + 1]), (c, box[c])
    else:
        assert padded[:W * total].ne(0).any()

    # run tables one run short: bit 2 for every run, nothing is added at all; boxes one slice late: bit 2, the voxels in front
    # of a box add nothing and no add leaves the histogram
    late = picked.table.clone()
    late[:, 1:3] += 1
    for tables, short in ((picked.table, 1), (late, 0)):
        cr, extra = runs_of(entry, name, dev)
        picked = cr.select(0, False)
        padded = torch.full((W * total + 64,), FILL, dtype=torch.int64, device=dev)
        head = list(cr.hist_head(dataclasses.replace(picked, table=tables)))
        assert head[5] == cr.runs
        head[5] = cr.runs - short                                # the one argument that is wrong on purpose
        _lib.check(fn(*head, _p(padded), total, *extra, st), entry)
        assert pipeline._download(cr.tot)[2] == 4
        assert padded[W * total:].eq(FILL).all()
        got = padded[:W * total].cpu().numpy().reshape(total, W)
        if short:
            assert not got.any()
        elif counts:
            for c in range(n):                                   # what lies inside the late box is filed where it belongs
                assert np.array_equal(got[off[c]:off[c + 1] - 1, 0], per[c, box[c, 0] + 1:box[c, 1] + 1]), (c, box[c])
                assert not got[off[c + 1] - 1].any()
