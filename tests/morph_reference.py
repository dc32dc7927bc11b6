"""NumPy reference of the 6-neighbour passes behind smooth_voxel_data (voxel_processor.py:79-97), one pass at a time.

tomo_morph_fused takes ANY pass mask, the oracle only the lists smooth_voxel_data produces; this reference covers the
rest.  tests/test_morph_masks_cpu.py pins it to the oracle on the lists both can express, so the GPU test that uses it
(tests/test_gpu_smooth_collapse.py) is not judged by the code under test."""
import numpy as np


def volume(shape, seed):
    """Noise with a solid block against the right border (the tail word) and a half-dense corner."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape) < 0.82
    v[:, : shape[1] // 3, -(shape[2] // 5 + 1):] = True          # solid block against the right border and the tail word
    v[shape[0] // 2:, shape[1] // 2:, : shape[2] // 7 + 1] = rng.random((shape[0] - shape[0] // 2, shape[1] - shape[1] // 2,
                                                                       shape[2] // 7 + 1)) < 0.5
    return v


def morph_pass(v, op):
    """One pass over the 3-D cross: op 0 = erosion, outside counts as 1; op 1 = dilation, outside counts as 0."""
    p = np.pad(np.asarray(v, bool), 1, constant_values=(op == 0))
    taps = [p[1:-1, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1],
            p[1:-1, 1:-1, :-2], p[1:-1, 1:-1, 2:]]
    return np.logical_and.reduce(taps) if op == 0 else np.logical_or.reduce(taps)


def apply_mask(v, ops, nops):
    """nops passes, bit j of `ops` = pass j (0 erosion, 1 dilation) -- the mask tomo_morph_fused takes."""
    for j in range(nops):
        v = morph_pass(v, (ops >> j) & 1)
    return v
