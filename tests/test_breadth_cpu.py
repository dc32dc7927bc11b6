"""CPU tier of the Crofton mean breadth: tests/breadth_reference.py against an independent walk over every lattice plane with
Python sets and a hand-written table of the cells, against SciPy's labelling of the extracted 2-D sections, against mirror
symmetry and hand values; the factor table of pipeline.py (pure NumPy) against the reference's (SciPy's spherical Voronoi
cells); the argument checks and signatures of the new functions -- none of which needs a GPU."""
import ctypes
import inspect
import itertools
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breadth_reference as R  # noqa: E402
import topology_reference as T  # noqa: E402
from tomography_3d_reconstructor_amd import _lib, pipeline, volume_calculator  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = [(1.0, 1.0, 1.0), (0.5, 1.0, 2.0), (0.7, 0.45, 0.3)]                             # (mm_x, mm_y, h)
VARIABLE = np.array([0.5, 0.5, 1.0, 0.25, 2.0, 1.0, 0.75])

# The cells per family, written out by hand: (a_z, a_y, a_x) -> (edges, faces), a face by its corners besides the anchor.
X, Y, Z = (0, 0, 1), (0, 1, 0), (1, 0, 0)
HAND = {
    (0, 0, 1): ([Y, Z], [(Y, Z, (1, 1, 0))]),
    (0, 1, 0): ([X, Z], [(X, Z, (1, 0, 1))]),
    (1, 0, 0): ([X, Y], [(X, Y, (0, 1, 1))]),
    (0, 1, -1): ([Z, (0, 1, 1)], [(Z, (0, 1, 1), (1, 1, 1))]),
    (0, 1, 1): ([Z, (0, 1, -1)], [(Z, (0, 1, -1), (1, 1, -1))]),
    (1, -1, 0): ([X, (1, 1, 0)], [(X, (1, 1, 0), (1, 1, 1))]),
    (1, 1, 0): ([X, (1, -1, 0)], [(X, (1, -1, 0), (1, -1, 1))]),
    (1, 0, -1): ([Y, (1, 0, 1)], [(Y, (1, 0, 1), (1, 1, 1))]),
    (1, 0, 1): ([Y, (1, 0, -1)], [(Y, (1, 0, -1), (1, 1, -1))]),
    (1, -1, -1): ([(0, 1, -1), (1, 0, 1), (1, 1, 0)], [((0, 1, -1), (1, 1, 0)), ((1, 0, 1), (1, 1, 0))]),
    (1, -1, 1): ([(0, 1, 1), (1, 0, -1), (1, 1, 0)], [((0, 1, 1), (1, 1, 0)), ((1, 0, -1), (1, 1, 0))]),
    (1, 1, -1): ([(0, 1, 1), (1, -1, 0), (1, 0, 1)], [((0, 1, 1), (1, 0, 1)), ((1, -1, 0), (1, 0, 1))]),
    (1, 1, 1): ([(0, 1, -1), (1, -1, 0), (1, 0, -1)], [((0, 1, -1), (1, 0, -1)), ((1, -1, 0), (1, 0, -1))]),
}


def noise(density, seed, shape=(7, 9, 12)):
    return np.random.default_rng(seed).random(shape) < density


NOISE = {25: noise(0.25, 25), 60: noise(0.60, 60)}


def add(p, o):
    return (p[0] + o[0], p[1] + o[1], p[2] + o[2])


def walk(v):
    """Every lattice plane of every family, its cells enumerated with sets -> chi int64 (13,) of the whole volume and the
    in / cross split per slice int64 (nz, 26) from the slices of the corners."""
    pts = set(map(tuple, np.argwhere(v)))
    total = np.zeros(13, dtype=np.int64)
    split = np.zeros((v.shape[0], 26), dtype=np.int64)
    for f, m in enumerate(R.NORMALS):
        edges, faces = HAND[m]
        planes = {}
        for p in pts:
            planes.setdefault(p[0] * m[0] + p[1] * m[1] + p[2] * m[2], set()).add(p)
        for plane in planes.values():
            nv = len(plane)
            ne = sum(1 for p in plane for e in edges if add(p, e) in plane)
            nf = sum(1 for p in plane for face in faces if all(add(p, o) in plane for o in face))
            total[f] += nv - ne + nf
            for p in plane:
                split[p[0], f] += 1
                for sign, group in ((-1, [(e,) for e in edges]), (1, faces)):
                    for cell in group:
                        corners = [add(p, o) for o in cell]
                        if all(q in plane for q in corners):
                            slices = {q[0] for q in corners} | {p[0]}
                            assert min(slices) == p[0] and max(slices) <= p[0] + 1           # filed in the slice of the anchor
                            split[p[0], f + 13 * (len(slices) - 1)] += sign
    return total, split


# ----------------------------------------------------------------------------- the cells
def test_the_normals_are_the_thirteen_in_ascending_order():
    want = [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, -1), (1, -1, 0), (1, -1, 1), (1, 0, -1), (1, 0, 0), (1, 0, 1), (1, 1, -1),
            (1, 1, 0), (1, 1, 1)]
    assert list(R.NORMALS) == want
    got = pipeline.breadth_normals()
    assert got.shape == (13, 3) and got.dtype.kind == "i" and [tuple(r) for r in got.tolist()] == want
    assert pipeline.BREADTH_COLUMNS == 26


def test_every_offset_is_a_26_neighbour_and_the_anchor_is_the_raster_first_corner():
    for m in R.NORMALS:
        edges, faces = R.cells(m)
        hand_edges, hand_faces = HAND[m]
        assert sorted(e[0] for e in edges) == sorted(hand_edges), m
        assert sorted(tuple(sorted(f)) for f in faces) == sorted(tuple(sorted(f)) for f in hand_faces), m
        for cell in edges + faces:
            corners = [(0, 0, 0)] + list(cell)
            assert min(corners) == (0, 0, 0)                                                 # raster order is tuple order
            for a, b in itertools.combinations(corners, 2):
                assert max(abs(x - y) for x, y in zip(a, b)) <= 1, (m, cell)                 # corners are 26-neighbours of each other
            for o in cell:
                assert max(map(abs, o)) <= 1 and sum(x * y for x, y in zip(o, m)) == 0, (m, cell)
                # inside the forward neighbourhood: (0, 0, 1), (0, 1, *), (1, *, *)
                assert o in R.FORWARD
        sides = {e[0] for e in edges}
        for face in faces:
            if len(face) == 2:                                                               # a triangle: its three sides are edges
                a, b = face
                assert a in sides and b in sides
                d = tuple(x - y for x, y in zip(b, a))
                assert d in sides or tuple(-x for x in d) in sides


@pytest.mark.parametrize("density", [25, 60])
def test_the_reference_equals_the_walk_over_the_planes(density):
    v = NOISE[density]
    got = R.chi_whole(v)
    total, split = walk(v)
    assert np.array_equal(R.section_euler(got), total)
    assert np.array_equal(got, split)
    assert not got[-1, 13:].any() and not got[:, 13 + R.NORMALS.index((1, 0, 0))].any()


@pytest.mark.parametrize("density", [25, 60])
def test_the_rectangular_families_equal_scipy_on_the_extracted_planes(density):
    """4-connected components minus 8-connected holes of every plane of the nine families with a rectangular section lattice."""
    from scipy import ndimage
    v = NOISE[density]
    pts = np.argwhere(v)
    euler = R.section_euler(R.chi_whole(v))
    four, eight = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    seen = 0
    for f, m in enumerate(R.NORMALS):
        if sum(map(abs, m)) == 3:
            continue
        seen += 1
        (u, e), _ = HAND[m]
        u, e = np.array(u), np.array(e)
        assert u @ e == 0
        chi = 0
        level = pts @ np.array(m)
        for c in np.unique(level):
            p = pts[level == c]
            i, j = (p @ u) // (u @ u), p @ e
            assert len(np.unique(j % (e @ e))) == 1                                          # one lattice: steps of e are whole
            i, j = i - i.min(), (j - j.min()) // (e @ e)
            img = np.zeros((i.max() + 3, j.max() + 3), dtype=bool)
            img[i + 1, j + 1] = True
            chi += ndimage.label(img, four)[1] - (ndimage.label(~img, eight)[1] - 1)
        assert chi == euler[f], m
    assert seen == 9


def mirrored_family(m, axis):
    q = list(m)
    q[axis] = -q[axis]
    q = tuple(q)
    return R.NORMALS.index(q if q > (0, 0, 0) else tuple(-x for x in q))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mirror_symmetry(axis):
    """Mirroring the volume permutes section_euler within a class and leaves the breadth alone -- on noise, variable depths."""
    mm_y, mm_x = 0.45, 0.7
    for density in (25, 60):
        v = NOISE[density]
        w = np.ascontiguousarray(np.flip(v, axis))
        d = VARIABLE
        dw = d[::-1].copy() if axis == 0 else d
        a, b = R.section_euler(R.chi_whole(v)), R.section_euler(R.chi_whole(w))
        perm = [mirrored_family(m, axis) for m in R.NORMALS]
        assert sorted(perm) == list(range(13))
        for f, m in enumerate(R.NORMALS):
            assert sorted(map(abs, m)) == sorted(map(abs, R.NORMALS[perm[f]]))
        assert np.array_equal(b[perm], a)
        for directions in (13, 3):
            x = R.breadth(R.chi_whole(v), pipeline.breadth_factors(d, 7, mm_y, mm_x, directions), directions)
            y = R.breadth(R.chi_whole(w), pipeline.breadth_factors(dw, 7, mm_y, mm_x, directions), directions)
            assert abs(x - y) <= 1e-12 * abs(x), (axis, density, directions, x, y)


# ----------------------------------------------------------------------------- hand values
def test_one_voxel():
    v = np.ones((1, 1, 1), dtype=bool)
    assert R.section_euler(R.chi_whole(v)).tolist() == [1] * 13
    assert abs(R.mean_breadth(v) - 0.75102007697) < 1e-10
    assert R.mean_breadth(v, directions=3) == 1.0
    assert abs(R.mean_breadth(v, [2.0], 1.0, 0.5) - 0.91061687050) < 1e-10
    assert abs(R.breadth(R.chi_whole(v), pipeline.breadth_factors(None, 1)) - 0.75102007697) < 1e-10
    assert R.breadth(R.chi_whole(v), pipeline.breadth_factors(None, 1, directions=3), 3) == 1.0
    assert abs(R.breadth(R.chi_whole(v), pipeline.breadth_factors([2.0], 1, 1.0, 0.5)) - 0.91061687050) < 1e-10


@pytest.mark.parametrize("step", R.FORWARD)
def test_two_voxels_along_every_forward_step(step):
    """Two voxels one 26-step apart: a family whose planes hold the step sees one section with one edge where that step is one
    of its edges (chi 1) and two vertices otherwise (chi 2); every other family cuts them with two planes (chi 2)."""
    v = np.zeros((3, 3, 3), dtype=bool)
    v[1, 1, 1] = True
    v[add((1, 1, 1), step)] = True
    got = R.section_euler(R.chi_whole(v))
    for f, m in enumerate(R.NORMALS):
        want = 1 if step in HAND[m][0] else 2
        assert got[f] == want, (step, m)
    x = R.chi_whole(v)
    edge = [-1 if step in HAND[m][0] else 0 for m in R.NORMALS]
    if step[0]:                                                  # the edge leaves the slice: a cross cell of slice 1
        assert x[1, :13].tolist() == [1] * 13 and x[2, :13].tolist() == [1] * 13
        assert x[1, 13:].tolist() == edge and not x[2, 13:].any()
    else:
        assert x[1, :13].tolist() == [2 + e for e in edge] and not x[1, 13:].any() and not x[2].any()


BOXES = [(5, 8, 11), (8, 8, 8), (1, 4, 7)]


@pytest.mark.parametrize("box", BOXES)
def test_the_box_closed_form(box):
    v = np.zeros((box[0] + 2, box[1] + 2, box[2] + 1), dtype=bool)
    v[1:1 + box[0], 2:2 + box[1], :box[2]] = True
    want = [sum(abs(a) * (n - 1) for a, n in zip(m, box)) + 1 for m in R.NORMALS]
    assert R.section_euler(R.chi_whole(v)).tolist() == want
    for mm_x, mm_y, h in SPACINGS:
        nz = v.shape[0]
        got = R.mean_breadth(v, np.full(nz, h), mm_y, mm_x)
        w = R.weights(mm_x, mm_y, h)
        closed = sum(w[f] * R.spacing(m, mm_x, mm_y, h) * want[f] for f, m in enumerate(R.NORMALS))
        assert abs(got - closed) <= 1e-12 * closed
        three = R.mean_breadth(v, np.full(nz, h), mm_y, mm_x, directions=3)
        assert abs(three - (box[0] * h + box[1] * mm_y + box[2] * mm_x) / 3.0) <= 1e-12 * three


def test_the_box_and_the_cube_show_the_bias_on_flat_faces():
    a, b = np.ones((5, 8, 11), dtype=bool), np.ones((8, 8, 8), dtype=bool)
    assert abs(R.mean_breadth(a) - 10.4805616018) < 1e-9 and abs(R.mean_breadth(b) - 10.4805616018) < 1e-9
    assert abs(R.mean_breadth(a) / 12.0 - 0.873) < 1e-3
    # directions = 3: (5 + 8 + 11) / 3.  The one-lattice formula gives 8.0 itself; the per-slice sum adds thirds slice by
    # slice and is met to rounding
    assert R.one_lattice(a, directions=3) == 8.0
    assert abs(R.mean_breadth(a, directions=3) - 8.0) < 1e-12 * 8.0


@pytest.mark.parametrize("mm_x,mm_y,h", SPACINGS)
def test_uniform_depths_give_the_one_lattice_formula(mm_x, mm_y, h):
    for density in (25, 60):
        v = NOISE[density]
        for directions in (13, 3):
            a = R.mean_breadth(v, np.full(7, h), mm_y, mm_x, directions)
            b = R.one_lattice(v, h, mm_y, mm_x, directions)
            scale = sum(abs(int(e)) for e in R.section_euler(R.chi_whole(v)))
            assert abs(a - b) <= 1e-12 * scale * max(mm_x, mm_y, h)


@pytest.mark.parametrize("radius,read", [(4, 1.0046), (8, 1.0172), (16, 1.0039)])
def test_the_balls_are_within_two_and_a_half_percent(radius, read):
    n = 2 * radius + 3
    v = R.ball(radius, np.ones(n), n, n)
    got = R.mean_breadth(v) / (2.0 * radius)
    print("ball R = %d: %.5f of 2 R" % (radius, got))
    assert abs(got - 1.0) < 0.025
    assert abs(got - read) < 5e-5                                # the value the README quotes
    assert abs(R.breadth(R.chi_whole(v), pipeline.breadth_factors(None, n)) / (2.0 * radius) - got) < 1e-11


def test_the_anisotropic_and_the_variable_ball():
    v = R.ball(8.0, np.full(11, 2.0), 21, 37, 1.0, 0.5)          # spacing (2, 1, 0.5)
    got = R.mean_breadth(v, np.full(11, 2.0), 1.0, 0.5) / 16.0
    print("ball sampled with (2, 1, 0.5): %.5f of 2 R" % got)
    assert abs(got - 1.0) < 0.025
    d = np.concatenate([np.ones(10), np.full(5, 2.0)])            # 8 mm whose upper half has slices twice as deep
    zc = R.slice_centres(d, len(d)) - 10.0
    y = np.arange(21) - 10.0
    w = zc[:, None, None] ** 2 + y[None, :, None] ** 2 + y[None, None, :] ** 2 <= 64.0
    got = R.mean_breadth(w, d) / 16.0
    print("ball with the upper half twice as deep: %.5f of 2 R" % got)
    assert abs(got - 1.0) < 0.025


def test_the_torus_and_the_hollow_ball():
    t = R.torus(20, 6, 56)
    assert T.euler(t, 26) == 0
    got = R.mean_breadth(t)
    print("torus R = 20, r = 6: %.3f against pi R = %.3f" % (got, math.pi * 20))
    assert abs(got / (math.pi * 20) - 1.0) < 0.03
    z, y, x = R.grid(np.ones(37), 37, 37)
    rr = z ** 2 + y ** 2 + x ** 2
    hollow = (rr <= 256) & (rr > 64)
    got = R.mean_breadth(hollow)
    print("hollow ball 16 / 8: %.3f against 16" % got)
    assert abs(got / 16.0 - 1.0) < 0.02                          # the inner surface counts negatively


# ----------------------------------------------------------------------------- components
def test_rows_under_26_are_the_masks_and_rows_under_6_add_up():
    differ = {6: 0, 26: 0}
    for density in (25, 60):
        v = NOISE[density]
        whole = R.chi_whole(v)
        for conn in (6, 26):
            labels, n = T.label(v, conn)
            rows = R.chi(labels, n)
            assert np.array_equal(rows.sum(axis=0), whole)
            for c in range(n):
                alone = R.chi_whole(labels == c + 1)
                differ[conn] += int((R.section_euler(rows[c]) != R.section_euler(alone)).sum())
                if conn == 26:
                    assert np.array_equal(rows[c], alone)
    assert differ[26] == 0 and differ[6] > 0                     # the diagonal contacts under 6 go to the first corner


def test_a_cell_across_a_diagonal_contact_goes_to_its_first_corner():
    v = np.zeros((1, 2, 2), dtype=bool)
    v[0, 0, 0] = v[0, 1, 1] = True                               # two components under 6, touching by an edge
    labels, n = T.label(v, 6)
    assert n == 2
    rows = R.section_euler(R.chi(labels, n))
    f = R.NORMALS.index((0, 1, -1))                              # the family whose edge (0, 1, 1) joins them
    first = labels[0, 0, 0] - 1
    assert rows[first, f] == 0 and rows[1 - first, f] == 1
    assert R.section_euler(R.chi_whole(labels == first + 1))[f] == 1


# ----------------------------------------------------------------------------- the factor table
@pytest.mark.parametrize("directions", [13, 3])
def test_breadth_factors_are_the_formula(directions):
    d = np.array([0.5, 0.5, 1.0, 0.25, 2.0])
    mm_y, mm_x = 0.45, 0.7
    B = pipeline.breadth_factors(d, 5, mm_y, mm_x, directions)
    assert B.dtype == np.float64 and B.shape == (5, 26)
    classes = ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))
    no_cross = R.NORMALS.index((1, 0, 0))
    for k in range(5):
        for col in range(26):
            f, m = col % 13, R.NORMALS[col % 13]
            if col >= 13 and (k == 4 or f == no_cross):
                assert B[k, col] == 0.0 and not np.signbit(B[k, col])
                continue
            h = d[k] if col < 13 else (d[k] + d[k + 1]) / 2
            w = pipeline.crofton_weights(1 / mm_x, 1 / mm_y, 1 / h, directions)[classes.index(tuple(map(abs, m)))]
            assert B[k, col] == w * (1.0 / math.sqrt((m[0] / h) ** 2 + (m[1] / mm_y) ** 2 + (m[2] / mm_x) ** 2)), (k, col)
            assert abs(B[k, col] / R.spacing(m, mm_x, mm_y, h) - R.weights(mm_x, mm_y, h, directions)[f]) < 1e-12
        assert abs(sum(B[k, f] / R.spacing(m, mm_x, mm_y, d[k]) for f, m in enumerate(R.NORMALS)) - 1.0) < 1e-12
    assert abs(R.weights(mm_x, mm_y, 0.3).sum() - 1.0) < 1e-12
    assert np.abs(B - R.factors(d, 5, mm_y, mm_x, directions)).max() < 1e-12
    assert B[0, :13].tolist() == B[0, 13:21].tolist() + [B[0, 8]] + B[0, 22:].tolist()      # (0.5 + 0.5) / 2: the same lattice
    ones = pipeline.breadth_factors(None, 4, mm_y, mm_x, directions)
    assert ones.tobytes() == pipeline.breadth_factors(np.ones(4), 4, mm_y, mm_x, directions).tobytes()
    if directions == 3:
        others = [c for c in range(26) if c % 13 not in R.AXES]
        assert not B[:, others].any() and (B[:, list(R.AXES)] > 0).all()
        for f, side in zip(R.AXES, (mm_x, mm_y, 1.0)):          # a third of the voxel's side (1 / sqrt((1 / s)^2) rounds twice)
            assert abs(B[2, f] - side / 3) <= 4 * np.finfo(float).eps * side


def test_bad_arguments_are_refused_without_a_gpu():
    for directions in (0, 4, 7, 26):
        with pytest.raises(ValueError):
            pipeline.breadth_factors(None, 3, 1.0, 1.0, directions)
    for depths, nz in (([1.0, 0.0], 2), ([1.0, -1.0], 2), ([1.0, float("nan")], 2), ([1.0, 1.0], 3)):
        with pytest.raises(ValueError):
            pipeline.breadth_factors(depths, nz)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pipeline.breadth_factors(None, 2, bad, 1.0)
        with pytest.raises(ValueError):
            pipeline.breadth_factors(None, 2, 1.0, bad)
    v = np.ones((2, 3, 4), dtype=bool)
    d = np.ones(2)
    for bad in (v.astype(np.uint8), v[0], list(v)):
        with pytest.raises(TypeError):
            volume_calculator.mean_breadth(bad, 1.0, 1.0, d)
        with pytest.raises(TypeError):
            volume_calculator.minkowski_functionals(bad, 1.0, 1.0, d)
    # checked before the first launch: these raise where no device is present, too
    with pytest.raises(ValueError):
        volume_calculator.mean_breadth(v, 1.0, 1.0, d, directions=5)
    with pytest.raises(ValueError):
        volume_calculator.mean_breadth(v, 1.0, 0.0, d)
    with pytest.raises(ValueError):
        volume_calculator.component_properties(v, 1.0, 1.0, d, breadth=True, breadth_directions=5)
    with pytest.raises(ValueError):
        volume_calculator.minkowski_functionals(v, 1.0, 1.0, d, connectivity=18)
    with pytest.raises(ValueError):
        volume_calculator.minkowski_functionals(v, 1.0, 1.0, d, directions=4)


def test_signatures():
    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}

    names = lambda fn: list(inspect.signature(fn).parameters)   # noqa: E731
    assert names(pipeline.breadth_normals) == []
    assert names(pipeline.breadth_factors) == ["slice_depths", "nz", "mm_per_pixel_y", "mm_per_pixel_x", "directions"]
    assert defaults(pipeline.breadth_factors) == {"mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "directions": 13}
    assert names(pipeline.mean_breadth) == ["vol", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "directions"]
    assert defaults(pipeline.mean_breadth) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "directions": 13}
    assert names(pipeline.component_breadth) == ["vol", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "min_voxels",
                                                 "largest", "directions"]
    assert defaults(pipeline.component_breadth) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "connectivity": 6,
                                                    "min_voxels": 0, "largest": False, "directions": 13}
    assert names(pipeline.cavity_breadth) == ["vol", "slice_depths", "mm_per_pixel_y", "mm_per_pixel_x", "connectivity", "min_voxels",
                                              "max_voxels", "directions"]
    assert defaults(pipeline.cavity_breadth) == {"slice_depths": None, "mm_per_pixel_y": 1.0, "mm_per_pixel_x": 1.0, "connectivity": 6,
                                                 "min_voxels": 0, "max_voxels": None, "directions": 13}
    sig = inspect.signature(pipeline.ComponentRuns.breadth)
    assert list(sig.parameters) == ["self", "factors", "directions", "min_voxels", "largest", "max_voxels", "enclosed"]
    assert sig.parameters["max_voxels"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["enclosed"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [f.name for f in pipeline.MeanBreadth.__dataclass_fields__.values()] == ["mean_breadth_mm", "section_euler"]
    assert [f.name for f in pipeline.ComponentBreadth.__dataclass_fields__.values()] == ["labels", "voxels", "section_euler", "mean_breadth_mm"]
    assert names(volume_calculator.mean_breadth) == ["voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths", "directions"]
    assert defaults(volume_calculator.mean_breadth) == {"directions": 13}
    assert names(volume_calculator.minkowski_functionals) == ["voxel_data", "mm_per_pixel_x", "mm_per_pixel_y", "slice_depths",
                                                               "connectivity", "directions"]
    assert defaults(volume_calculator.minkowski_functionals) == {"connectivity": 26, "directions": 13}
    cp = names(volume_calculator.component_properties)
    assert cp[-3:] == ["caliper", "caliper_directions", "caliper_oriented"]
    # the two keywords sit in front of the chain separate_mm, separate_h_mm, skeleton, caliper .. that earlier tests pin link by link
    assert cp[cp.index("breadth"):cp.index("breadth") + 3] == ["breadth", "breadth_directions", "separate_mm"]
    assert cp[cp.index("geodesic_sweeps") + 1] == "breadth"
    d = defaults(volume_calculator.component_properties)
    assert d["breadth"] is False and d["breadth_directions"] == 13
    assert names(volume_calculator.closed_porosity)[-1] == "pore_caliper"
    assert "components_breadth" in pipeline.COUNTERS
    spec = pipeline._BREADTH
    assert spec.name == "component_breadth" and spec.hist == "tomo_cc_breadth_hist" and spec.finish == "tomo_cc_breadth"
    assert spec.counter == "components_breadth" and spec.words == pipeline.BREADTH_WORDS and spec.what


def test_the_two_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tomo_cc_breadth_hist", "tomo_cc_breadth"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["tomo_cc_breadth_hist"] == _lib.SIGNATURES["tomo_cc_surface_hist"]
    assert _lib.SIGNATURES["tomo_cc_breadth"] == _lib.SIGNATURES["tomo_cc_surface"]


# ----------------------------------------------------------------------------- the C entry points
def test_argument_checks_do_not_need_a_gpu():
    L = _lib.lib()
    a = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(a)                                      # a non-null host pointer, never dereferenced: every call is refused
    labelled = (p, 4, p, p, p, p, 4, p, p)                       # row_off, cap_runs, parent, rank, tot, table, cap, sel, off
    assert L.tomo_cc_breadth_hist(None, 2, 2, 2, *labelled, p, 8, None) == -1
    assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *labelled, None, 8, None) == -1
    for geo in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2)):
        assert L.tomo_cc_breadth_hist(p, *geo, *labelled, p, 8, None) == -1
    assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *labelled, p, 0, None) == -1
    for k in (0, 3, 4, 5, 7, 8):                                 # a table missing from the labelled form (parent alone: unlabelled)
        args = list(labelled)
        args[k] = None
        assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *args, p, 8, None) == -1
    for k in (1, 6):                                             # a size that is not positive
        args = list(labelled)
        args[k] = 0
        assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *args, p, 8, None) == -1
    unlabelled = (None, 0, None, None, None, None, 0, None, None)
    assert L.tomo_cc_breadth_hist(p, 4, 2, 2, *unlabelled, p, 3, None) == -1            # fewer entries than slices
    assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *(p, 1 << 31, p, p, p, p, 4, p, p), p, 8, None) == -3
    assert L.tomo_cc_breadth_hist(p, 2, 2, 2, *labelled, p, 1 << 60, None) == -3
    head = (p, 4, p, p, p, p)                                    # table, cap, tot, sel, off, slot
    tail = (p, p, p, 4, None)                                    # out, section_euler, labels, cap_sel, stream
    for directions in (0, 4, 26):
        assert L.tomo_cc_breadth(*head, p, 8, p, 2, directions, *tail) == -1
    for k in (2, 3, 4, 5):
        args = list(head)
        args[k] = None
        assert L.tomo_cc_breadth(*args, p, 8, p, 2, 13, *tail) == -1
    assert L.tomo_cc_breadth(*head, None, 8, p, 2, 13, *tail) == -1
    assert L.tomo_cc_breadth(*head, p, 8, None, 2, 13, *tail) == -1
    assert L.tomo_cc_breadth(*head, p, 0, p, 2, 13, *tail) == -1
    assert L.tomo_cc_breadth(*head, p, 8, p, 0, 13, *tail) == -1
    for k in (0, 1, 2):
        args = list(tail)
        args[k] = None
        assert L.tomo_cc_breadth(*head, p, 8, p, 2, 13, *args) == -1
    assert L.tomo_cc_breadth(*head, p, 8, p, 2, 13, p, p, p, 0, None) == -1
    assert L.tomo_cc_breadth(None, 0, None, None, None, None, p, 3, p, 4, 13, *tail) == -1     # unlabelled: fewer entries than slices
    assert L.tomo_cc_breadth(*head, p, 8, p, 2, 13, p, p, p, 1 << 31, None) == -3
    assert L.tomo_cc_breadth(*head, p, 1 << 60, p, 2, 13, *tail) == -3
    assert L.tomo_cc_breadth(p, 1 << 31, p, p, p, p, p, 8, p, 2, 13, *tail) == -3
