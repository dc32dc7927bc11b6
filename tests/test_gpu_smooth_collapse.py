"""GPU tier (-m gpu): the native smoothing planner (tomo_smooth) against the oracle, which runs every pass it is asked for.

pipeline.smooth(vol, n, m) must leave the bits of O.smooth(v, n, m) for every n, although the device runs at most one
closing (see the comment at tomo_smooth in csrc/bits.hip and tests/test_smooth_collapse_cpu.py for why that is legal).
Shapes are the tile-edge ones of test_gpu_parity.test_smooth_tile_edges_vs_oracle: rows beyond one 56-row tile, odd and
even word counts with the tail word in different places, nz across z chunks.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tomography_3d_reconstructor_amd import _lib, pipeline

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from morph_reference import apply_mask, volume  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(20, 130, 257), (9, 70, 262), (37, 57, 320), (12, 120, 513), (70, 9, 64), (5, 200, 1025), (3, 1, 700), (1, 90, 129),
          (20, 130, 384), (37, 57, 1090), (6, 300, 128), (50, 61, 1152)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def to_vol(arr, dev):
    return pipeline.pack(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8)).to(dev))


def to_np(vol):
    return pipeline.unpack(vol).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cm", [True, False])
def test_smooth_every_iteration_count_vs_oracle(dev, shape, cm):
    v = volume(shape, shape[2] + 17)
    vol = to_vol(v, dev)
    before = vol.bits.clone()
    for n in range(6):
        got = pipeline.smooth(vol, n, cm)
        assert got.shape == vol.shape and got.bits.data_ptr() != vol.bits.data_ptr()
        assert np.array_equal(to_np(got), O.smooth(v, n, cm)), (n, cm)
    assert torch.equal(vol.bits, before), "input must not be mutated"


@pytest.mark.parametrize("shape", [(37, 57, 320), (20, 130, 257), (5, 200, 1025)])
def test_raw_entry_overwrites_garbage(dev, shape):
    """The C entry point alone: whatever `out` held, every word of it is the result (tail bits of a row included: zero),
    for each of the four plans -- opening + closing, closing, opening, copy."""
    nz, ny, nx = shape
    v = volume(shape, 5)
    vol = to_vol(v, dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(99)
    for it, cm in [(3, True), (1, True), (4, False), (0, True), (0, False), (-2, False)]:
        out = torch.randint(-2 ** 62, 2 ** 62, vol.bits.shape, dtype=torch.int64, device=dev, generator=gen)
        _lib.check(L.tomo_smooth(vol.bits.data_ptr(), out.data_ptr(), nz, ny, nx, it, int(cm), stream), "tomo_smooth")
        want = to_vol(O.smooth(v, max(it, 0), cm), dev)
        assert torch.equal(out, want.bits), (it, cm)
    assert np.array_equal(to_np(vol), v)


def test_raw_entry_rejects_bad_arguments(dev):
    vol = to_vol(volume((4, 6, 70), 1), dev)
    L = _lib.lib()
    p = vol.bits.data_ptr()
    out = torch.empty_like(vol.bits)
    assert L.tomo_smooth(p, p, 4, 6, 70, 3, 1, None) == -1               # in place is not supported
    assert L.tomo_smooth(None, out.data_ptr(), 4, 6, 70, 3, 1, None) == -1
    assert L.tomo_smooth(p, None, 4, 6, 70, 3, 1, None) == -1
    assert L.tomo_smooth(p, out.data_ptr(), 0, 6, 70, 3, 1, None) == -1


def test_explicit_two_closings_mask_still_served(dev):
    """D E D E has no specialised kernel any more; tomo_morph_fused must still run it (generic kernel), and it must
    equal one closing."""
    shape = (20, 130, 384)
    v = volume(shape, 3)
    vol = to_vol(v, dev)
    out = torch.empty_like(vol.bits)
    _lib.check(_lib.lib().tomo_morph_fused(vol.bits.data_ptr(), out.data_ptr(), *shape, 5, 4,
                                           torch.cuda.current_stream().cuda_stream), "tomo_morph_fused")
    assert np.array_equal(to_np(pipeline.BitVolume(out, shape)), O.smooth(v, 2, False))
    assert np.array_equal(O.smooth(v, 2, False), O.smooth(v, 1, False))


def words(v):
    """Bit-packed (nz, ny, wx) int64 words of a boolean volume as the library lays them out: bits beyond nx are zero."""
    nz, ny, nx = v.shape
    wx = (nx + 63) // 64
    padded = np.zeros((nz, ny, wx * 64), np.uint8)
    padded[:, :, :nx] = v
    return np.packbits(padded, axis=2, bitorder="little").view("<u8").view(np.int64).reshape(nz, ny, wx)


# each the smallest that crosses one edge: two row tiles for both pass counts (60 and 56 own rows), five words and a
# 6-bit tail; z chunks of 16 with a remainder, whole words; one row and fewer slices than the z halo
@pytest.mark.parametrize("shape", [(9, 70, 262), (37, 57, 320), (3, 1, 700)])
def test_every_pass_mask_vs_numpy_reference(dev, shape):
    """tomo_morph_fused is the only way to a mask the planner does not emit: all 4 masks of 2 passes and all 16 of 4
    passes, into a garbage-filled `out`, word for word (tail bits zero) against tests/morph_reference.py."""
    v = volume(shape, shape[2] + 17)
    vol = to_vol(v, dev)
    assert np.array_equal(vol.bits.cpu().numpy(), words(v))
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(7)
    for nops in (2, 4):
        for ops in range(1 << nops):
            out = torch.randint(-2 ** 62, 2 ** 62, vol.bits.shape, dtype=torch.int64, device=dev, generator=gen)
            _lib.check(L.tomo_morph_fused(vol.bits.data_ptr(), out.data_ptr(), *shape, ops, nops, stream), "tomo_morph_fused")
            assert np.array_equal(out.cpu().numpy(), words(apply_mask(v, ops, nops))), (nops, ops)
    assert np.array_equal(to_np(vol), v)
