"""CPU tier: tests/scale_reference.py against the per-feature references it stands in for at a million components, on the small
fixtures of components_reference and cavities_reference, with == -- so that the scale tier's reference is no second opinion
nobody checked.  The pinned hash and counts are checked for `runs_past` only (the smallest volume); test_gpu_scale.py asserts
the others from its cached references."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavities_reference as R  # noqa: E402
import component_props_reference as P  # noqa: E402
import components_reference as C  # noqa: E402
import scale_reference as X  # noqa: E402
import surface_reference as S  # noqa: E402
import topology_reference as T  # noqa: E402

COMPONENT_FIXTURES = C.fixtures()
CAVITY_FIXTURES = R.fixtures()
MM_X, MM_Y = 0.7, 0.45
SMALL = [n for n, v in COMPONENT_FIXTURES.items() if n not in ("checkerboard", "noise_big")]
CASES = [(n, k) for n in SMALL for k in C.CONNECTIVITIES] + [("noise_big", 6), ("checkerboard", 6)]


def depths_for(nz):
    d = np.linspace(0.3, 1.7, nz)
    if nz > 2:
        d[nz // 2] = d[nz // 2 - 1]
    return d


@pytest.mark.parametrize("name,conn", CASES)
def test_sparse_slice_counts_volume_and_properties(name, conn):
    v = COMPONENT_FIXTURES[name]
    labels, n, tab = P.measure(v, conn)
    nz = v.shape[0]
    c, z, count = X.slice_entries(labels, n)
    dense = P.slice_counts(labels, n)
    assert all(a.dtype == np.int64 for a in (c, z, count))
    assert np.array_equal(np.stack([c, z], axis=1), np.argwhere(dense)) and np.array_equal(count, dense[dense != 0])
    for d in (depths_for(nz), np.ones(nz), depths_for(nz)[:max(1, nz - 1)]):
        got = X.volume_of((c, z, count), n, MM_X, MM_Y, d)
        exp = P.volume_of(dense, MM_X, MM_Y, d)
        assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes(), name
    d = depths_for(nz)
    sums = X.volume_of((c, z, count), n, MM_X, MM_Y, d)
    rules = [(0, False), (2, False), (0, True)] + ([(int(np.median(tab[:, 0])), True)] if n else [])
    for min_voxels, largest in rules:
        exp = P.properties(labels, tab, d, MM_Y, MM_X, min_voxels, largest)
        got = X.properties(tab, sums, MM_Y, MM_X, P.selected(tab[:, 0], min_voxels, largest))
        assert sorted(got) == sorted(exp)
        for k in exp:
            assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (name, k)
            assert got[k].tobytes() == exp[k].tobytes(), (name, min_voxels, largest, k)
    assert X.count_runs(v) == sum(int(np.count_nonzero(np.diff(np.concatenate([[0], row.view(np.int8)])) == 1))
                                  for row in v.reshape(-1, v.shape[2]))


@pytest.mark.parametrize("name", list(CAVITY_FIXTURES))
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_crop_serves_the_per_component_references(name, conn):
    """topology_reference.components and surface_reference.component_counts, component by component, from crop()."""
    v = CAVITY_FIXTURES[name]
    labels, n, topo = T.components(v, conn)
    tab = P.table(labels, n)
    pick = np.arange(n) if n <= 40 else np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n),
                                                                   np.argsort(tab[:, 0], kind="stable")[-24:]]))
    assert np.array_equal(X.topology_rows(labels, tab, pick, conn), topo[pick])
    per = S.component_counts(labels, n)
    for c in pick:
        mask, box = X.crop(labels, tab[c], c + 1)
        assert mask.dtype == np.bool_ and int(mask.sum()) == tab[c, 0]
        for axis in range(3):                                    # the box plus one voxel, cut at the faces of the stack
            assert box[axis].start == max(tab[c, 1 + 2 * axis] - 1, 0) and box[axis].stop == min(tab[c, 2 + 2 * axis] + 2, v.shape[axis])
        z0, counts = X.surface_counts(labels, tab, c)
        full = np.zeros((v.shape[0], 11), dtype=np.int64)
        full[z0:z0 + len(counts)] = counts
        assert np.array_equal(full, per[c]), (name, conn, int(c))


@pytest.mark.parametrize("name", list(CAVITY_FIXTURES))
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_owners_and_the_cavity_rule(name, conn):
    v = CAVITY_FIXTURES[name]
    bg_labels, n_bg, tab = R.background(v, conn)
    fg_labels, _ = T.label(v, conn)
    assert np.array_equal(X.owners(fg_labels, bg_labels, n_bg), R.owners_of(v, conn, bg_labels, n_bg))
    labels, own, sizes = R.cavities(v, conn)
    for lo, hi in ((0, None), (2, 12), (0, 1), (5, 4)):
        keep = X.cavity_rule(tab, v.shape, lo, hi) if n_bg else np.zeros(0, dtype=bool)
        assert np.array_equal(np.flatnonzero(keep) + 1, labels[R.window(sizes, lo, hi)])
        assert np.array_equal(np.concatenate([[False], keep])[bg_labels], R.cavity_mask(v, conn, lo, hi))


def test_the_pinned_volume_runs_past():
    """The smallest of the pinned volumes: its bits, its runs and its components under both connectivities."""
    name = "runs_past"
    v = X.volume(name)
    assert v.shape == X.VOLUMES[name][0] and X.digest(X.packed(name)) == X.SHA256[name]
    assert X.count_runs(v) == X.RUNS[name] > X.EDGE
    for conn in C.CONNECTIVITIES:
        assert C.label(v, conn)[1] == X.COUNTS[(name, conn)]


def test_the_shapes_cross_what_they_name():
    for name in ("rows_edge", "rows_past"):
        nz, ny, _ = X.VOLUMES[name][0]
        assert nz * ny + 1 > X.EDGE
    nz, ny, _ = X.VOLUMES["rows_edge"][0]
    assert nz * ny + 1 == X.EDGE + 1                             # tile 1025 holds only the sentinel
    assert all(X.RUNS[n] > X.EDGE for n in ("runs_past", "comps_past", "dense"))
    assert X.COUNTS[("comps_past", 6)] > X.EDGE and X.DENSE_CAVITIES > X.EDGE
    assert X.VOLUMES["dense"][:3] == X.VOLUMES["comps_past"][:3] and X.VOLUMES["dense"][3]


def test_the_cloud():
    lin, words = X.cloud()
    nz, ny, nx = X.CLOUD_SHAPE
    assert words.shape == (nz, ny, nx // 64) and words.dtype == np.int64 and words.size > 1024 * X.PC_TILE
    assert lin[0] == 0 and lin[-1] == nz * ny * nx - 1 and (np.diff(lin) > 0).all() and 49000 < len(lin) <= X.CLOUD_VOXELS
    assert int((lin >= 64 * 1024 * X.PC_TILE).sum()) >= 1000
    assert np.array_equal(np.flatnonzero(C.unpack(words[:3], (3, ny, nx))), lin[lin < 3 * ny * nx])
    assert int(np.unpackbits(words.view(np.uint8)).sum()) == len(lin)
