"""Host reference for the per-component inscribed sphere and local thickness, in plain NumPy on top of edt_reference,
thickness_reference and components_reference (which it imports and leaves alone).

per_component(): for every component c of components_reference.label(v, connectivity), from the WHOLE-volume arrays
d2 = edt_reference.edt_squared(v) and level = thickness_reference.by_levels(v, d2, ...): the maximum of float32(sqrt(d2)) over
the mask of c with its first flat index, and thickness_reference.expected(mask_c, level * mask_c, radii, weights).  That the
whole-volume arrays under the mask ARE the arrays of the mask (distance and local thickness are local to a component) is what
tests/test_component_thickness_cpu.py holds, bit for bit, with one transform per component.

enclosed(): the same for the cavities -- the components of the complement under the complementary connectivity whose box
touches no face of the stack.  select(): the keep rule.  fixtures() / pore_fixtures(): the volumes of the tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as C  # noqa: E402
import edt_reference as E  # noqa: E402
import thickness_reference as T  # noqa: E402

KINDS = ("unit", "sided", "dyadic")
# sided: off every D2 and every outside distance of the fixtures by more than 1e-9 r^2 (test_component_thickness_cpu.py holds
# it), the last one above every ball: never launched, counts 0.  unit and dyadic: every squared distance is an integer / a
# multiple of 1 / 64 and so is every r^2 here, so D2 == r^2 and |pq|^2 == r^2 are hit exactly and decided exactly.
RADII = {"unit": (1.0, 1.5, 2.0, 3.0), "sided": (0.6, 1.1, 1.7, 2.2, 9.0), "dyadic": (0.5, 1.0, 1.5, 2.5)}
RULES = ((0, False), (5, False), (0, True))


# ----------------------------------------------------------------------------- the volumes of the tests
def grains():
    """(9, 14, 131): the cases a pass over words, runs and components can get wrong, in a bed of speckle."""
    shape = (9, 14, 131)
    v = np.zeros(shape, dtype=bool)
    v[3:7, 1:5, 40:90] = True                                    # 4 x 4 x 50: the maximum sits on a plateau of 2 x 2 rows, across the word at 64
    v[1:3, 7:9, 2:4] = True                                      # two cubes that share a corner only: two components under 6,
    v[3:5, 9:11, 4:6] = True                                     # one under 26
    v |= T._ball(shape, (6, 3, 10), 2)                           # a ball and a box inside ONE 64-bit word, the ball on the face z = 8
    v[5:8, 1:4, 16:22] = True
    v[7:9, 10:13, :] = True                                      # touches x = 0 and x = 130, its runs cross the words at 64 and 128
    v |= T._ball(shape, (3, 8, 110), 3)                          # touches z = 0
    v[0:2, 12:14, 60:130] = True                                # a second run across 64 and 128, on the face z = 0
    keep = np.zeros(shape, dtype=bool)                           # the plateau and the corner contact stay as designed
    keep[2:8, 0:6, 39:91] = keep[0:6, 6:12, 1:7] = True
    noise = np.random.default_rng(29).random(shape) < 0.012
    return v ^ (noise & ~keep)


def fixtures():
    """name -> bool volume, in a fixed order: grains and six of thickness_reference's; none has more than 6 500 set voxels."""
    t = T.fixtures()
    out = {"grains": grains()}
    for name in ("dumbbell", "shell", "edge", "one", "empty", "full"):
        out[name] = t[name]
    for name, v in out.items():
        assert v.sum() <= 6500, name
    return out


def pore_box():
    """(9, 12, 70): a solid box with two cavities of different shape -- a 3 x 3 x 3 cube and a crack one voxel thin, 4 x 16, across
    the word at 64 -- and a void that reaches the face x = 69 (no cavity)."""
    v = np.zeros((9, 12, 70), dtype=bool)
    v[1:8, 1:11, 2:70] = True
    v[3:6, 3:6, 8:11] = False
    v[4, 4:8, 52:68] = False
    v[2, 2, 66:70] = False
    return v


def pore_fixtures():
    return {"shell": T.fixtures()["shell"], "pore_box": pore_box()}


# ----------------------------------------------------------------------------- the reference
def whole(v, kind, radii):
    """(tables, d2, level map or None) of the whole volume."""
    tabs = T.tables(v.shape, kind)
    d2 = E.edt_squared(v, *tabs, True)
    level = None
    if radii is not None:
        r = np.asarray(radii, dtype=np.float64)
        level = T.by_levels(v, d2, tabs, r * r)
    return tabs, d2, level


def rows_of(v, labels, n, kind, radii, arrays=None):
    """One dict per label 1 .. n, from the whole-volume arrays of v under the mask `labels == c`."""
    v = np.asarray(v) != 0
    tabs, d2, level = whole(v, kind, radii) if arrays is None else arrays
    dist = np.sqrt(d2).astype(np.float32)
    weights = T.slice_weights(v.shape, kind)
    zt, yt, xt = tabs
    out = []
    for c in range(1, n + 1):
        mask = labels == c
        flat = int(np.argmax(np.where(mask, dist, np.float32(-1)).reshape(-1)))      # the first maximum
        k, j, i = (int(a) for a in np.unravel_index(flat, v.shape))
        row = {"label": c, "voxels": int(mask.sum()), "radius_mm": float(dist[k, j, i]), "center_index": (k, j, i),
               "center_mm": (float(zt[k + 1]), float(yt[j + 1]), float(xt[i + 1]))}
        assert mask[k, j, i] and row["radius_mm"] > 0
        if radii is not None:
            e = T.expected(mask, level * mask, radii, weights)
            for key in ("level_voxels", "level_volume_mm3", "uncovered_voxels", "mean_mm", "std_mm", "max_mm"):
                row[key] = e[key]
        out.append(row)
    return out


def per_component(v, connectivity, kind, radii=None):
    labels, n = C.label(v, connectivity)
    return rows_of(v, labels, n, kind, radii)


def select(rows, min_voxels=0, largest=False):
    """The keep rule on the rows: at least min_voxels voxels; largest: only the largest of those, the lowest label among equals."""
    kept = [r for r in rows if r["voxels"] >= min_voxels]
    if largest and kept:
        top = max(r["voxels"] for r in kept)
        kept = [next(r for r in kept if r["voxels"] == top)]
    return kept


def enclosed(v, connectivity, kind, radii=None):
    """The rows of the cavities of v: the reference applied to the complement, the components of it under 32 - connectivity
    whose inclusive index box touches no face of the stack; the labels are the complement's."""
    outside = ~(np.asarray(v) != 0)
    labels, n = C.label(outside, 32 - connectivity)
    rows = rows_of(outside, labels, n, kind, radii)
    out = []
    for r in rows:
        idx = np.nonzero(labels == r["label"])
        if all(a.min() > 0 and a.max() < s - 1 for a, s in zip(idx, outside.shape)):
            out.append(r)
    return out
