"""GPU tier: the owner lookups of the mc3 faces pass (csrc/mc.hip, far_owner_positions: the owners of a row share one offset
pair and one ballot record, rows that are not needed are not looked up, (x+1) past the last column of a segment is a lookup
of its own).  The shapes are the ones at which the list lookup can go wrong (test_list_lookup_at_segment_and_volume_borders
in test_gpu_parity.py: segment s covers float columns [256 s - 224, 256 s + 32)) and a wider one; noise at 0.5 hits every
MC33 case and centre vertices.  Each shape runs with exact sizes, from the size hint and submitted; everything is compared
with the oracle bit for bit, and no pass may count a triangle corner without a vertex."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tomography_3d_reconstructor_amd import _lib, pipeline

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 40), (3, 4, 300), (3, 3, 600), (5, 6, 530)]
MM = (0.7, 0.9)
SEG_SHIFT, KEY_XBITS = 224, 20                     # csrc/tomo_common.h, csrc/mc.hip
EDGES_X1 = (1 << 10) | (1 << 5)                    # the edges owned by (y+1, x+1) and (z+1, x+1): MC_EDGES of csrc/mc.hip
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def noise(shape, seed=0):
    """Noise at density 0.5 whose last voxel is set: the last row, column and slice are active."""
    mask = np.random.default_rng(sum(shape) + seed).random(shape) < 0.5
    mask[-1, -1, -1] = True
    return mask


def reference(shape, seed=0):
    """(mask, depths, oracle vertices, oracle faces), computed once per (shape, seed) and never modified."""
    if (shape, seed) not in _REF:
        mask, depths = noise(shape, seed), np.full(shape[0], 0.5)
        ev, ef = O.SurfaceExtractor().extract_manifold_surface(mask, depths, *MM)
        for a in (mask, ev, ef):
            a.flags.writeable = False
        _REF[(shape, seed)] = (mask, depths, ev, ef)
    return _REF[(shape, seed)]


def to_vol(arr, dev):
    return pipeline.pack(torch.from_numpy(np.array(arr).view(np.uint8)).to(dev))


def field_of(mask, dev):
    return pipeline.make_field(to_vol(mask, dev), sparse=pipeline.FIELD_SPARSE)


def same(v, f, ev, ef):
    return v.cpu().numpy().tobytes() == ev.tobytes() and np.array_equal(f.cpu().numpy(), ef)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_hinted_and_submitted_passes_equal_the_oracle(dev, shape):
    mask, depths, ev, ef = reference(shape)
    f = field_of(mask, dev)
    pipeline._MC3_HINT.pop((f.Nz, f.Ny, f.Nx, 0), None)
    # 1. no hint: exact sizes
    before = dict(pipeline.COUNTERS)
    m = pipeline.mc3_vertices(f, depths, *MM)
    assert pipeline.COUNTERS["mc3_hint_hit"] == before["mc3_hint_hit"] and pipeline.COUNTERS["mc3_hint_miss"] == before["mc3_hint_miss"]
    assert same(m.uniq, m.faces_final, ev, ef)
    assert int(m.tot[6].item()) == 0
    # what the inputs are there to reach.  The last list entry has triangles: its (x+1) test runs at i + 1 == na
    na = m.na
    til = m.vox_til[:na].cpu().numpy()
    assert til[na - 1] & 15 > 0
    # the row behind the last active row of the top slice -- where its (y+1) owners would be -- has only empty segments, as
    # has the slice above it
    spr = _lib.lib().tomo_mc_segments_per_row(f.Nx, f.xorg)
    cnt = np.diff(m.seg_aoff.cpu().numpy().view(np.uint32).astype(np.int64)).reshape(f.Nz, f.Ny, spr)
    assert cnt.sum() == na
    assert cnt[f.Nz - 2, f.Ny - 2].sum() > 0 and cnt[f.Nz - 2, f.Ny - 1].sum() == 0 and cnt[f.Nz - 1].sum() == 0
    # a cell in the last column of a segment needs an owner at x+1, the first voxel of the next segment (every shape that is
    # wide enough to have such cells in numbers)
    cc = ((m.vox_key[:na].cpu().numpy() >> 2) & ((1 << KEY_XBITS) - 1)) + f.xorg + SEG_SHIFT
    used = m.vox_used[:na].cpu().numpy().view(np.uint16)
    crossing = int((((cc & 255) == 255) & ((used & EDGES_X1) != 0) & ((til & 15) > 0)).sum())
    assert crossing > 0 or shape[2] < 300
    # 2. the same shape again: from the size hint, nothing read before the triangles are written
    before = dict(pipeline.COUNTERS)
    m2 = pipeline.mc3_vertices(field_of(mask, dev), depths, *MM)
    assert pipeline.COUNTERS["mc3_hint_hit"] == before["mc3_hint_hit"] + 1
    assert same(m2.uniq, m2.faces_final, ev, ef)
    assert int(m2.tot[6].item()) == 0
    # 3. submitted, read later
    v, fc = pipeline.extract_surface_submit(to_vol(mask, dev), depths, *MM).result()
    assert same(v, fc, ev, ef)


def test_two_submitted_passes_keep_their_own_buffers(dev):
    """submit, submit, result, result: two passes of one geometry in flight; each gets its own mesh."""
    shape = (3, 4, 300)
    a, depths, eva, efa = reference(shape)
    b, _, evb, efb = reference(shape, seed=1)
    assert (a != b).any()
    pipeline.extract_surface(to_vol(a, dev), depths, *MM)                       # the size hint of the geometry
    before = pipeline.COUNTERS["mc3_hint_hit"]
    pa = pipeline.extract_surface_submit(to_vol(a, dev), depths, *MM)
    pb = pipeline.extract_surface_submit(to_vol(b, dev), depths, *MM)
    ra, rb = pa.result(), pb.result()
    assert pipeline.COUNTERS["mc3_hint_hit"] == before + 2
    assert same(*ra, eva, efa)
    assert same(*rb, evb, efb)


def test_repeated_faces_pass_gives_the_same_triangles(dev):
    shape = (5, 6, 530)
    mask, depths, ev, ef = reference(shape)
    m = pipeline.mc3_vertices(field_of(mask, dev), depths, *MM)
    again = m.faces_checked(again=True)
    assert torch.equal(again, m.faces_final) and np.array_equal(again.cpu().numpy(), ef)
    assert int(m.tot[6].item()) == 0
