"""CPU tier: repeated closings collapse to one -- the property the native smoothing planner (tomo_smooth) rests on.

The reference's closing is a dilation that pads with 0 followed by an erosion that pads with 1 (voxel_processor.py:88-91).
With exactly these border values the pair is an adjunction on the finite grid, so the closing is idempotent and
smooth(v, n, m) == smooth(v, 1, m) for every n >= 1.  Checked here against the reference-derived oracle alone (no GPU,
no product code): a change of border rule in the oracle or the reference makes these fail before the planner is wrong.
"""
import numpy as np
import pytest

from oracle import oracle as O

ITER = [1, 2, 3, 4, 5]


def assert_collapses(v):
    for cm in (True, False):
        one = O.smooth(v, 1, cm)
        for n in ITER:
            assert np.array_equal(O.smooth(v, n, cm), one), (v.shape, n, cm)


@pytest.mark.parametrize("shape", [(1, 5, 5), (5, 1, 9), (7, 6, 1), (2, 2, 2), (1, 1, 1), (2, 11, 3), (9, 2, 70), (12, 13, 14),
                                   (24, 20, 66)])
@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.8, 0.95])
def test_random_volumes(shape, density):
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[2] + int(density * 100))
    assert_collapses(rng.random(shape) < density)


@pytest.mark.parametrize("shape", [(1, 4, 6), (2, 5, 5), (6, 7, 8), (16, 16, 16)])
def test_constant_volumes(shape):
    assert_collapses(np.zeros(shape, bool))
    assert_collapses(np.ones(shape, bool))
    assert not O.smooth(np.zeros(shape, bool), 3, True).any()
    assert O.smooth(np.ones(shape, bool), 3, True).all()        # erosion pads with 1: a full box survives the opening


def test_bodies_touching_every_face():
    nz, ny, nx = 14, 15, 16
    v = np.zeros((nz, ny, nx), bool)
    v[0:3, 4:9, 5:11] = True          # z = 0 face
    v[-2:, 2:7, 3:9] = True           # z = nz - 1
    v[5:10, 0:2, 6:12] = True         # y = 0
    v[4:8, -3:, 1:6] = True           # y = ny - 1
    v[6:11, 5:10, 0:3] = True         # x = 0
    v[3:9, 8:13, -2:] = True          # x = nx - 1
    v[0, 0, 0] = v[-1, -1, -1] = v[0, -1, 0] = True     # single voxels in corners
    assert_collapses(v)
    assert_collapses(~v)              # and the complement: holes against every face
    # a shell whose wall IS the box boundary, with a cavity the closing must not fill from outside
    s = np.ones((nz, ny, nx), bool)
    s[1:-1, 1:-1, 1:-1] = False
    assert_collapses(s)
    # gaps of one and two voxels between bodies and the faces (where the border value decides the result)
    g = np.zeros((nz, ny, nx), bool)
    g[1:-1, 1:-1, 1:-1] = True
    g[2:-2:3, 3:-3, 3:-3] = False
    assert_collapses(g)
    g2 = np.zeros((nz, ny, nx), bool)
    g2[2:-2, 2:-2, 2:-2] = True
    assert_collapses(g2)


def test_noisy_ellipsoid():
    nz, ny, nx = 24, 40, 56
    v = np.stack(O.ellipsoid_masks(nz, ny, nx)).astype(bool)
    rng = np.random.default_rng(7)
    assert_collapses(v ^ (rng.random(v.shape) < 0.02))
    assert_collapses(v ^ (rng.random(v.shape) < 0.2))


def test_closing_is_a_closing():
    """The three properties behind the collapse, each on its own: extensive, increasing, idempotent -- and the opening in
    front of it does not disturb them."""
    rng = np.random.default_rng(11)
    for shape in [(3, 9, 10), (10, 11, 12), (1, 20, 20)]:
        a = rng.random(shape) < 0.4
        b = a | (rng.random(shape) < 0.2)                        # a subset of b
        ca, cb = O.smooth(a, 1, False), O.smooth(b, 1, False)
        assert (ca | a).sum() == ca.sum()                        # a subset of closing(a)
        assert (ca & ~cb).sum() == 0                             # closing(a) subset of closing(b)
        assert np.array_equal(O.smooth(ca, 1, False), ca)        # closing(closing(a)) == closing(a)
        assert np.array_equal(O.smooth(a, 0, True), O.smooth(O.smooth(a, 0, True), 0, True))    # the opening likewise
        assert np.array_equal(O.smooth(a, 4, True), O.smooth(O.smooth(a, 0, True), 1, False))
