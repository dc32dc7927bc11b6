"""CPU tier: the NumPy pass reference (tests/morph_reference.py) against the oracle, on the pass lists the oracle can run."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_reference as M  # noqa: E402


@pytest.mark.parametrize("shape", [(9, 70, 262), (3, 1, 700)])
def test_pass_masks_match_the_oracle(shape):
    v = M.volume(shape, shape[2] + 17)
    assert np.array_equal(M.apply_mask(v, 6, 4), O.smooth(v, 1, True))       # E D | D E
    assert np.array_equal(M.apply_mask(v, 1, 2), O.smooth(v, 1, False))      # D E
    assert np.array_equal(M.apply_mask(v, 2, 2), O.smooth(v, 0, True))       # E D
    assert np.array_equal(M.apply_mask(v, 5, 4), O.smooth(v, 2, False))      # D E | D E
