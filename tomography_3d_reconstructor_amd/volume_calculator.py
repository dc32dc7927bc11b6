"""Drop-in for the reference's volume_calculator.py (/root/reference/volume_calculator.py:10-132; SURVEY.md 8f row
N1), written against its contract: class and method names, argument order, the keys of the returned dicts and the four
report lines.  The two reductions over the volume -- voxel counts per slice and the index bounding box -- run on the
bit-packed copy that is already resident on the MI355X (tomo_slice_popcounts / tomo_bbox: 1 bit per voxel read once,
where np.sum per slice + np.where move 1 B per voxel and 24 B per set voxel); everything after them is a handful of
float64 operations on the host, done in the order that makes every returned number bit-identical to the reference's
(tests/golden/consumers.npz).

The host arithmetic is exposed as plain functions of (slice counts, index box) so that a Z-slab job can feed it the
all-gathered per-rank reductions (slab.SlabJob.voxel_volume / bounding_box) and get the very same numbers.
"""
import math

import numpy as np

from . import pipeline
from .voxel_processor import to_device_volume

_EMPTY_BOX = {'x': (0, 0), 'y': (0, 0), 'z': (0, 0), 'dimensions': (0, 0, 0)}


# ----------------------------------------------------------------------------- host arithmetic on the reductions
def volume_from_slice_counts(counts, mm_per_pixel_x, mm_per_pixel_y, slice_depths):
    """Volume in mm^3 of a stack whose slice z holds counts[z] set voxels of depth slice_depths[z] (:23-35).
    The reference adds count * (mm_x * mm_y * depth) slice by slice into a float; a cumulative sum performs the same
    additions in the same order, so the last partial sum is that float."""
    n = min(len(counts), len(slice_depths))
    if n == 0:
        return 0.0
    depth = np.asarray(slice_depths, dtype=np.float64)[:n]
    per_slice = np.asarray(counts[:n], dtype=np.int64) * (mm_per_pixel_x * mm_per_pixel_y * depth)
    return np.cumsum(per_slice)[-1]


def _span(lo, hi):
    return (lo, hi), hi - lo


def box_record(extent_x, extent_y, extent_z):
    """The dict both bounding-box methods return, from the three (low, high) extents in mm."""
    (x, dx), (y, dy), (z, dz) = _span(*extent_x), _span(*extent_y), _span(*extent_z)
    return {'x': x, 'y': y, 'z': z, 'dimensions': (dx, dy, dz)}


def box_uniform_depth(box, mm_per_pixel_x, mm_per_pixel_y, mm_per_slice):
    """:37-57 for an index box (zmin, zmax, ymin, ymax, xmin, xmax) of np.int64."""
    z0, z1, y0, y1, x0, x1 = box
    return box_record((x0 * mm_per_pixel_x, x1 * mm_per_pixel_x), (y0 * mm_per_pixel_y, y1 * mm_per_pixel_y),
                      (z0 * mm_per_slice, z1 * mm_per_slice))


def box_variable_depth(box, mm_per_pixel_x, mm_per_pixel_y, slice_depths):
    """:59-94: x / y as above, z from the running sum of the slice depths -- the lower face of the first occupied slice
    to the upper face of the last one (clamped to the table)."""
    if box is None or len(slice_depths) == 0:
        return dict(_EMPTY_BOX)
    z0, z1, y0, y1, x0, x1 = box
    edges = np.cumsum(np.concatenate([[0], slice_depths]))
    top = min(z1 + 1, len(edges) - 1)
    return box_record((x0 * mm_per_pixel_x, x1 * mm_per_pixel_x), (y0 * mm_per_pixel_y, y1 * mm_per_pixel_y),
                      (edges[z0], edges[top]))


# ----------------------------------------------------------------------------- the two reductions
def _on_device(a):
    return isinstance(a, np.ndarray) and a.dtype == np.bool_ and a.ndim == 3


def slice_counts(voxel_data):
    """np.sum(voxel_data[z]) for every z -> int64 (nz,)."""
    if _on_device(voxel_data):
        return pipeline.slice_counts(to_device_volume(voxel_data)).cpu().numpy()
    return np.asarray([np.sum(voxel_data[z]) for z in range(voxel_data.shape[0])])      # other dtypes: plain host sums


def index_box(voxel_data):
    """min / max index of the set voxels per axis as (zmin, zmax, ymin, ymax, xmin, xmax) of np.int64; None if empty."""
    if _on_device(voxel_data):
        b = pipeline.bounding_box(to_device_volume(voxel_data))
        return None if b is None else tuple(np.int64(i) for i in b)
    idx = np.nonzero(voxel_data)
    if len(idx[0]) == 0:
        return None
    return tuple(f(axis) for axis in idx for f in (np.min, np.max))


def largest_inscribed_sphere(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths):
    """The largest sphere that fits inside the object, in millimetres (no counterpart in the reference): the maximum of the
    exact Euclidean distance to the background (pipeline.inscribed_sphere: per-slice depths honoured, everything outside the
    stack is background) -> {'radius_mm', 'diameter_mm', 'center_index': (z, y, x), 'center_mm': (z_mm, y_mm, x_mm)}.
    An empty volume has radius 0.0 and no centre (None).  voxel_data: the bool (nz, ny, nx) array the other calculations
    take; anything else is a TypeError -- there is no host path for this one."""
    if not _on_device(voxel_data):
        raise TypeError("largest_inscribed_sphere needs a bool (nz, ny, nx) array")
    found = pipeline.inscribed_sphere(to_device_volume(voxel_data), slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    if found is None:
        return {'radius_mm': 0.0, 'diameter_mm': 0.0, 'center_index': None, 'center_mm': None}
    radius, (z, y, x) = found
    nz, ny, nx = voxel_data.shape
    zt, yt, xt = pipeline.distance_positions(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x, ny, nx)
    return {'radius_mm': radius, 'diameter_mm': 2 * radius, 'center_index': (z, y, x),
            'center_mm': (float(zt[z + 1]), float(yt[y + 1]), float(xt[x + 1]))}


def thickness_statistics(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, radii_mm=None):
    """How thick the object is, and where the volume sits in that scale (no counterpart in the reference): the local thickness
    of Hildebrand & Ruegsegger -- at a voxel the diameter of the largest ball that fits inside the object and contains it
    (pipeline.local_thickness: per-slice depths honoured, everything outside the stack is background) -> {'mean_mm', 'std_mm',
    'max_mm', 'uncovered_voxels', 'histogram': [(diameter_mm, voxels, volume_mm3), ...]}, the histogram in ascending diameter,
    one entry per level.  radii_mm=None: the exact thickness, for thin structures and unit or binary-fraction spacings (a
    ValueError names radii_mm where the object has too many distinct distances); otherwise the ascending ball radii to
    measure with -- the granulometry used to choose a smoothing radius.  An empty volume gives zeros and, in exact mode, an
    empty histogram.  voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError -- there
    is no host path for this one."""
    if not _on_device(voxel_data):
        raise TypeError("thickness_statistics needs a bool (nz, ny, nx) array")
    if radii_mm is not None:
        pipeline._check_radii(radii_mm)                          # the argument checks, before anything is uploaded
    pipeline.distance_positions(slice_depths, voxel_data.shape[0], mm_per_pixel_y, mm_per_pixel_x)
    t = pipeline.local_thickness(to_device_volume(voxel_data), slice_depths, mm_per_pixel_y, mm_per_pixel_x, radii_mm)
    return {'mean_mm': t.mean_mm, 'std_mm': t.std_mm, 'max_mm': t.max_mm, 'uncovered_voxels': t.uncovered_voxels,
            'histogram': [(2.0 * float(r), int(n), float(v)) for r, n, v in zip(t.radii_mm, t.level_voxels, t.level_volume_mm3)]}


def sphericity(volume_mm3, surface_area_mm2):
    """pi^(1/3) (6 V)^(2/3) / S in float64: 1 for a ball, smaller for everything else (up to the estimator's error); 0.0
    where there is no surface."""
    v, s = float(volume_mm3), float(surface_area_mm2)
    return float(np.pi ** (1.0 / 3.0) * (6.0 * v) ** (2.0 / 3.0) / s) if s > 0.0 else 0.0


def surface_area(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, directions=13):
    """The surface area of the whole volume without a mesh (no counterpart in the reference, whose calculate_surface_area needs
    the marching-cubes triangles): the discretised Crofton formula on the voxels (pipeline.surface_area: per-slice depths
    honoured, everything outside the stack is background; directions=13, or 3 for the axis directions alone) ->
    {'surface_area_mm2', 'voxel_volume_mm3', 'sphericity'}; voxel_volume_mm3 is calculate_voxel_volume_variable_depth's number
    and sphericity = pi^(1/3) (6 V)^(2/3) / S.  An axis-aligned flat face is underestimated by about 14 %: the known bias of the
    estimator.  voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError -- there is
    no host path for this one."""
    if not _on_device(voxel_data):
        raise TypeError("surface_area needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline.surface_factors(depths, voxel_data.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)   # the argument checks
    vol = to_device_volume(voxel_data)
    s = pipeline.surface_area(vol, depths, mm_per_pixel_y, mm_per_pixel_x, directions).surface_area_mm2
    v = float(volume_from_slice_counts(pipeline.slice_counts(vol).cpu().numpy(), mm_per_pixel_x, mm_per_pixel_y, depths))
    return {'surface_area_mm2': s, 'voxel_volume_mm3': v, 'sphericity': sphericity(v, s)}


def mean_breadth(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, directions=13):
    """The mean breadth of the whole volume in mm (no counterpart in the reference): the fourth Minkowski functional by the
    discretised Crofton formula on the voxels (pipeline.mean_breadth: per-slice depths honoured, everything outside the stack
    is background; directions=13, or 3 for the axis normals alone) -> a Python float; 2 pi times it is the integral of mean
    curvature.  voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError -- there is
    no host path for this one."""
    if not _on_device(voxel_data):
        raise TypeError("mean_breadth needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline.breadth_factors(depths, voxel_data.shape[0], mm_per_pixel_y, mm_per_pixel_x, directions)   # the argument checks
    return pipeline.mean_breadth(to_device_volume(voxel_data), depths, mm_per_pixel_y, mm_per_pixel_x, directions).mean_breadth_mm


def minkowski_functionals(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity=26, directions=13):
    """The four Minkowski functionals (intrinsic volumes) of the volume and of its components (no counterpart in the
    reference) -> {'volume_mm3', 'surface_area_mm2', 'mean_breadth_mm', 'mean_curvature_integral_mm' (2 pi mean_breadth_mm),
    'euler_number'} of the whole volume -- slice_counts, pipeline.surface_area, pipeline.mean_breadth and pipeline.euler_number
    under `connectivity`, none of which labels anything -- then the four densities per mm^3 of the stack ('volume_fraction',
    'surface_density_per_mm', 'mean_curvature_density_per_mm2', 'euler_density_per_mm3'; the stack is nx mm_x by ny mm_y by the
    sum of the depths) and 'components': the dicts of component_properties(..., connectivity, topology=True, surface=True,
    breadth=True) with `directions` for both estimators.  Every additive, motion-invariant measure of a grain or a pore is a
    combination of the four.  Arguments are checked before the first launch; voxel_data: a bool (nz, ny, nx) array, else a
    TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("minkowski_functionals needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    nz, ny, nx = voxel_data.shape
    pipeline._check_connectivity(connectivity)
    pipeline.surface_factors(depths, nz, mm_per_pixel_y, mm_per_pixel_x, directions)                    # the argument checks
    pipeline.breadth_factors(depths, nz, mm_per_pixel_y, mm_per_pixel_x, directions)
    vol = to_device_volume(voxel_data)
    v = float(volume_from_slice_counts(pipeline.slice_counts(vol).cpu().numpy(), mm_per_pixel_x, mm_per_pixel_y, depths))
    s = pipeline.surface_area(vol, depths, mm_per_pixel_y, mm_per_pixel_x, directions).surface_area_mm2
    b = pipeline.mean_breadth(vol, depths, mm_per_pixel_y, mm_per_pixel_x, directions).mean_breadth_mm
    e = int(pipeline.euler_number(vol, connectivity))
    stack = float(nx * float(mm_per_pixel_x) * (ny * float(mm_per_pixel_y)) * float(np.sum(depths)))
    m = 2.0 * math.pi * b
    return {'volume_mm3': v, 'surface_area_mm2': s, 'mean_breadth_mm': b, 'mean_curvature_integral_mm': m, 'euler_number': e,
            'volume_fraction': v / stack, 'surface_density_per_mm': s / stack, 'mean_curvature_density_per_mm2': m / stack,
            'euler_density_per_mm3': e / stack,
            'components': component_properties(voxel_data, mm_per_pixel_x, mm_per_pixel_y, depths, connectivity, topology=True,
                                               surface=True, surface_directions=directions, breadth=True,
                                               breadth_directions=directions)}


CHORD_QUANTILES = (0.1, 0.5, 0.9)


def _chord_phase_report(c):
    """The dict of one phase of chord_report from a pipeline.ChordLengths."""
    total = int(c.chords.sum())
    try:
        f = c.fabric()
        fabric = {'tensor': f['tensor'].tolist(), 'principal_mil_mm': f['principal_mil_mm'].tolist(), 'axes': f['axes'].tolist(),
                  'degree_of_anisotropy': f['degree_of_anisotropy']}
    except ValueError:                                           # chords in fewer than six directions, or no ellipsoid fits
        fabric = None
    return {'voxels': c.voxels, 'chords': c.chords.tolist(), 'mil_mm': c.mean_chord_mm.tolist(),
            'mean_chord_mm': float(np.sum(c.total_length_mm) / total) if total else float('nan'),
            'fabric': fabric, 'lineal_path': c.lineal_path(),
            'quantiles_mm': {'fractions': CHORD_QUANTILES, 'values': c.quantiles_mm(CHORD_QUANTILES)}}


def chord_report(voxel_data, slice_depths, mm_per_pixel_y, mm_per_pixel_x, background=True):
    """Which way the structure runs and how far one can go through it in a straight line (no counterpart in the reference):
    the chord lengths of the volume as a whole along the 13 lattice directions (pipeline.chord_lengths: no labelling, per-slice
    depths honoured, everything outside the stack is background) -> {'directions': the 13 steps (dz, dy, dx), 'object': {...},
    'background': {...} or None with background=False}.  A phase holds 'voxels', 'chords' and 'mil_mm' per direction (the mean
    intercept length: Tb.Th / Tb.Sp by intercepts, the chord-length pore size), 'mean_chord_mm' over all directions, 'fabric'
    (pipeline.ChordLengths.fabric as lists: 'tensor', 'principal_mil_mm', 'axes', 'degree_of_anisotropy'; None where fewer than
    six directions have a chord or no ellipsoid fits), 'lineal_path' float64 (13, L + 1) and 'quantiles_mm': the 10 / 50 / 90 %
    quantiles of the chord length per direction by number of chords, float64 (13, 3).  One upload serves both phases.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError -- there is no host path
    for this one."""
    if not _on_device(voxel_data):
        raise TypeError("chord_report needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline.chord_steps(depths, voxel_data.shape[0], mm_per_pixel_y, mm_per_pixel_x)                   # the argument checks
    vol = to_device_volume(voxel_data)
    report = {'directions': [tuple(int(v) for v in s) for s in pipeline.chord_directions()], 'background': None}
    for phase in pipeline.CHORD_PHASES if background else pipeline.CHORD_PHASES[:1]:
        report[phase] = _chord_phase_report(pipeline.chord_lengths(vol, depths, mm_per_pixel_y, mm_per_pixel_x, phase))
    return {key: report[key] for key in ('directions', 'object', 'background')}


def _two_point_phase_report(t):
    """The dict of one phase of two_point_report from a pipeline.TwoPoint."""
    centres, values, lags = t.radial(max(t.spacing))
    return {'volume_fraction': t.volume_fraction(),
            'specific_surface_per_mm': t.specific_surface_per_mm() if min(t.max_lag) >= 1 else None,
            'correlation_length_mm': t.correlation_length_mm().tolist(), 'directional': t.directional(),
            'radial': {'bin_mm': max(t.spacing), 'centres_mm': centres, 'values': values, 'lags': lags}}


def two_point_report(voxel_data, slice_depths, mm_per_pixel_y, mm_per_pixel_x, max_lag=16, background=True):
    """How the structure is correlated with itself (no counterpart in the reference): the two-point probability S2(h) of the
    volume as a whole over the box of integer lags max_lag (an int or (Rz, Ry, Rx), Rx <= 63; pipeline.two_point: no
    labelling, no wrap-around, the spacing enters on the host) -> {'max_lag': (Rz, Ry, Rx), 'object': {...}, 'background':
    {...} or None with background=False, 'cross'}.  A phase holds 'volume_fraction' (S2(0)), 'specific_surface_per_mm' (the
    slope at the origin by Crofton's weights; None unless every R >= 1), 'correlation_length_mm' per direction of
    pipeline.chord_directions() (where the correlation first falls below 1 / e; NaN if not inside the box), 'directional'
    float64 (13, R + 1) (S2 along those directions) and 'radial': the orientation average in shells of 'bin_mm' = the largest
    spacing, 'centres_mm', 'values', 'lags'.  'cross': the symmetrised chance that of two points a lag apart ONE lies in the object
    and one in the background, (P - N_object - N_background) / (2 P) as a float64 table over the box, NaN where P = 0; None
    without the background.  One upload serves both phases.  voxel_data: the bool (nz, ny, nx) array the other calculations
    take; anything else is a TypeError -- there is no host path for this one."""
    if not _on_device(voxel_data):
        raise TypeError("two_point_report needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline.distance_positions(depths, voxel_data.shape[0], mm_per_pixel_y, mm_per_pixel_x)            # the argument checks
    box = pipeline.two_point_box(max_lag)
    vol = to_device_volume(voxel_data)
    tables = {phase: pipeline.two_point(vol, box, depths, mm_per_pixel_y, mm_per_pixel_x, phase)
              for phase in (pipeline.CHORD_PHASES if background else pipeline.CHORD_PHASES[:1])}
    report = {'max_lag': box, 'object': _two_point_phase_report(tables['object']), 'background': None, 'cross': None}
    if background:
        report['background'] = _two_point_phase_report(tables['background'])
        P = tables['object'].inside()
        cross = np.full(P.shape, np.nan, dtype=np.float64)
        np.divide((P - tables['object'].pairs - tables['background'].pairs).astype(np.float64), (2 * P).astype(np.float64), out=cross,
                  where=P > 0)
        report['cross'] = cross
    return report


def closed_porosity(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity=6, min_voxels=0, max_voxels=None,
                    pore_size=False, pore_geodesic=False, pore_caliper=False):
    """The enclosed voids of the volume, listed and added up (no counterpart in the reference): pipeline.cavity_table -- a
    cavity is a component of the complement, under the complementary connectivity, that reaches no face of the stack; per-slice
    depths honoured -> {'cavities', 'cavity_voxels', 'cavity_volume_mm3', 'voxel_volume_mm3', 'closed_porosity', 'table'}.
    table: one dict per cavity with min_voxels <= voxels <= max_voxels (None: no upper bound) in ascending label: {'label',
    'owner' (the label of the component that encloses it), 'voxels', 'volume_mm3', 'bounding_box': {'x', 'y', 'z'},
    'dimensions', 'centroid_mm': (z, y, x), 'centroid_index': (z, y, x), 'equivalent_diameter_mm'} -- volume, box and centroids
    as component_properties gives them for the mask of the cavity, equivalent_diameter_mm = cbrt(6 V / pi).
    cavity_volume_mm3: the rows' volumes added in that order; voxel_volume_mm3: calculate_voxel_volume_variable_depth's number
    for the solid; closed_porosity = cavity / (solid + cavity), 0.0 for an empty volume.  pore_size=True: every row also carries
    'inscribed_diameter_mm' -- twice the largest inside distance of the cavity, the widest ball that fits in the pore: for a
    crack-shaped pore the size that equivalent_diameter_mm is not -- and 'inscribed_center_index' (z, y, x), and the report
    'largest_pore_diameter_mm' (0.0 without pores): pipeline.cavity_sizes, ONE transform of the complement for all pores together.
    pore_caliper=True: every row also carries 'max_caliper_mm' and 'min_caliper_mm' -- the largest and the smallest caliper
    (Feret) diameter of the pore over pipeline.caliper_directions(), voxel extents included (pipeline.ComponentRuns.caliper on the
    complement's tables): the length and the opening of a crack -- and the report 'longest_pore_mm', the largest 'max_caliper_mm'
    of the rows (0.0 without pores).  pore_geodesic=True (a keyword, like the other flags): every row also carries
    'geodesic_length_mm' -- the length of the pore along itself, the repeated farthest-point search of pipeline.cavity_geodesic on
    the complement's tables, centre to centre: a lower bound of its geodesic diameter on the lattice metric -- and 'tortuosity',
    that length over the straight distance of its two ends, and the report 'longest_pore_path_mm' (0.0 without pores).
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError -- there is no host path
    for this one."""
    if not _on_device(voxel_data):
        raise TypeError("closed_porosity needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline._check_connectivity(connectivity)                  # the argument checks, before anything is uploaded
    pipeline._check_size_window(min_voxels, max_voxels)
    pipeline._slice_weights(depths, len(voxel_data), mm_per_pixel_y, mm_per_pixel_x)
    if pore_geodesic:
        pipeline._geodesic_tables(voxel_data.shape, depths, mm_per_pixel_y, mm_per_pixel_x)
    vol = to_device_volume(voxel_data)
    if pore_caliper or pore_geodesic:                            # the steps of cavity_table / cavity_sizes on ONE object
        lo, hi = pipeline._check_size_window(min_voxels, max_voxels)
        runs = pipeline.ComponentRuns(vol, connectivity)
        bg = runs.background()
        tables = pipeline._slice_weights(depths, len(voxel_data), mm_per_pixel_y, mm_per_pixel_x)
        t = pipeline._cavities_from(runs, bg.properties(tables, mm_per_pixel_y, mm_per_pixel_x, lo, max_voxels=hi, enclosed=True))
        if pore_size:
            size = bg.thickness(depths, mm_per_pixel_y, mm_per_pixel_x, None, lo, max_voxels=hi, enclosed=True)
        if pore_caliper:
            feret = bg.caliper(depths, mm_per_pixel_y, mm_per_pixel_x, min_voxels=lo, max_voxels=hi, enclosed=True)
        if pore_geodesic:
            path = bg.geodesic(depths, mm_per_pixel_y, mm_per_pixel_x, min_voxels=lo, max_voxels=hi, enclosed=True)
    elif pore_size:
        t, size = pipeline.cavity_sizes(vol, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_voxels, max_voxels)
    else:
        t = pipeline.cavity_table(vol, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_voxels, max_voxels)
    solid = float(volume_from_slice_counts(pipeline.slice_counts(vol).cpu().numpy(), mm_per_pixel_x, mm_per_pixel_y, depths))
    boxes = [box_variable_depth(tuple(b), mm_per_pixel_x, mm_per_pixel_y, depths) for b in t.index_box]
    table = [{'label': int(t.labels[i]), 'owner': int(t.owner[i]), 'voxels': int(t.voxels[i]), 'volume_mm3': float(t.volume_mm3[i]),
              'bounding_box': {axis: box[axis] for axis in ('x', 'y', 'z')}, 'dimensions': box['dimensions'],
              'centroid_mm': tuple(float(v) for v in t.centroid_mm[i]),
              'centroid_index': tuple(float(v) for v in t.centroid_index[i]),
              'equivalent_diameter_mm': float(np.cbrt(6.0 * t.volume_mm3[i] / np.pi))} for i, box in enumerate(boxes)]
    cavity = 0.0
    for row in table:
        cavity += row['volume_mm3']
    whole = solid + cavity
    report = {'cavities': len(table), 'cavity_voxels': int(t.voxels.sum()), 'cavity_volume_mm3': cavity, 'voxel_volume_mm3': solid,
              'closed_porosity': cavity / whole if whole else 0.0, 'table': table}
    if pore_size:                                                # row i of both answers: one selection of the complement's tables
        assert np.array_equal(size.labels, t.labels)
        for i, row in enumerate(table):
            row['inscribed_diameter_mm'] = 2 * float(size.radius_mm[i])
            row['inscribed_center_index'] = tuple(int(v) for v in size.center_index[i])
        report['largest_pore_diameter_mm'] = max((row['inscribed_diameter_mm'] for row in table), default=0.0)
    if pore_caliper:
        assert np.array_equal(feret.labels, t.labels)
        for i, row in enumerate(table):
            row['max_caliper_mm'], row['min_caliper_mm'] = float(feret.max_mm[i]), float(feret.min_mm[i])
        report['longest_pore_mm'] = max((row['max_caliper_mm'] for row in table), default=0.0)
    if pore_geodesic:
        assert np.array_equal(path.labels, t.labels)
        for i, row in enumerate(table):
            row['geodesic_length_mm'], row['tortuosity'] = float(path.length_mm[i]), float(path.tortuosity[i])
        report['longest_pore_path_mm'] = max((row['geodesic_length_mm'] for row in table), default=0.0)
    return report


def separate_grains(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, radius_mm, connectivity=6, min_marker_voxels=1):
    """Touching objects taken apart (no counterpart in the reference): pipeline.separate_components -- the cores left by a ball
    erosion of radius_mm millimetres are grown back through the object, and the object is cut where two growths meet; per-slice
    depths honoured -> {'volume' (the separated volume, a NumPy bool array of the input's shape), 'components_before',
    'components_after' (under `connectivity`), 'markers' (cores of at least min_marker_voxels voxels), 'cut_voxels', 'cut_share'
    (cut voxels over the set voxels of the input; 0.0 for an empty volume)}.  An object thinner than the radius everywhere has no
    core and stays whole; a fixed radius cuts an elongated grain whose erosion falls into two cores (pipeline.geodesic_zones takes
    markers made by another rule).  component_properties(..., separate_mm=radius_mm) measures the separated grains.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("separate_grains needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline._separation_args(voxel_data.shape, radius_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels)
    return _separation_report(to_device_volume(voxel_data), connectivity, lambda vol: pipeline.separate_components(
        vol, radius_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels))


def _separation_report(vol, connectivity, separate):
    """separate_grains' dict for separate(vol) -> pipeline.Separation."""
    before = int(pipeline.ComponentRuns(vol, connectivity).sizes().shape[0])
    solid = int(pipeline.popcount_async(vol).item())
    sep = separate(vol)
    after = int(pipeline.ComponentRuns(sep.volume, connectivity).sizes().shape[0])
    return {'volume': pipeline.unpack(sep.volume).cpu().numpy(), 'components_before': before, 'components_after': after,
            'markers': sep.markers, 'cut_voxels': sep.cut_voxels, 'cut_share': sep.cut_voxels / solid if solid else 0.0}


def separate_grains_by_height(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, h_mm, connectivity=6, min_marker_voxels=1,
                              min_radius_mm=0.0):
    """separate_grains with h-maxima markers (no counterpart in the reference): pipeline.separate_by_height -- one marker on every
    dome of the inside distance that stands at least h_mm millimetres above its saddle, so grains of different sizes are split
    by one parameter and surface roughness below h_mm splits nothing; min_radius_mm > 0 drops the markers of debris thinner
    than that -> the dict of separate_grains.  component_properties(..., separate_h_mm=h_mm) measures the separated grains.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("separate_grains_by_height needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline._height_args(voxel_data.shape, h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm)
    return _separation_report(to_device_volume(voxel_data), connectivity, lambda vol: pipeline.separate_by_height(
        vol, h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm))


def grain_contacts(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, radius_mm, connectivity=6, min_marker_voxels=1):
    """Which grains touch, and how (no counterpart in the reference): pipeline.separate_with_contacts -- the separation of
    separate_grains, then the contact table of its zones -> {'grains' (the markers), 'contacts' (zone pairs in contact under
    `connectivity`), 'mean_coordination' (contacts per grain, 0.0 without grains), 'coordination' (a list, the neighbours of marker
    label 1 .. n), 'table': one dict per contact, sorted by its zones: {'zones' (a, b), 'contact_voxel_pairs',
    'contact_area_mm2' (the Crofton estimate of the interface), 'throat_diameter_mm' (twice the largest inside distance on the
    interface), 'throat_index' ((z, y, x) of the voxel that attains it), 'path_mm' (the shortest way from core to core across
    the interface), 'at_index' ((z, y, x) of the first voxel of the interface)}}.  The pore network of the closed pores is the
    same call on the pore space -- pipeline.separate_with_contacts(pipeline.cavity_volume(vol), ...) on a resident volume: pore
    bodies, throats and ways; there is no second wrapper.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("grain_contacts needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline._separation_args(voxel_data.shape, radius_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels)
    vol = to_device_volume(voxel_data)
    return _contact_report(*pipeline.separate_with_contacts(vol, radius_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity,
                                                            min_marker_voxels))


def _contact_report(sep, c):
    """grain_contacts' dict for a pipeline.Separation and the pipeline.ZoneContacts of its zones."""
    _, neighbours, _ = c.coordination(np.arange(1, sep.markers + 1))
    table = [{'zones': (int(c.zone_a[i]), int(c.zone_b[i])), 'contact_voxel_pairs': int(c.pairs[i]),
              'contact_area_mm2': float(c.area_mm2[i]), 'throat_diameter_mm': 2.0 * float(c.value_max[i]),
              'throat_index': tuple(int(a) for a in c.value_index[i]), 'path_mm': float(c.path_mm[i]),
              'at_index': tuple(int(a) for a in c.first_index[i])} for i in range(len(c))]
    return {'grains': sep.markers, 'contacts': len(c), 'mean_coordination': float(neighbours.sum()) / sep.markers if sep.markers else 0.0,
            'coordination': neighbours.tolist(), 'table': table}


def grain_contacts_by_height(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, h_mm, connectivity=6, min_marker_voxels=1,
                             min_radius_mm=0.0):
    """grain_contacts for the separation of separate_grains_by_height (no counterpart in the reference):
    pipeline.separate_by_height_with_contacts -> the dict of grain_contacts.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("grain_contacts_by_height needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    pipeline._height_args(voxel_data.shape, h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, min_marker_voxels, min_radius_mm)
    vol = to_device_volume(voxel_data)
    return _contact_report(*pipeline.separate_by_height_with_contacts(vol, h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity,
                                                                      min_marker_voxels, min_radius_mm))


def skeleton_report(voxel_data, connectivity=26, curve=True):
    """The skeleton of a volume by homotopic thinning (no counterpart in the reference): pipeline.skeleton and
    pipeline.skeleton_nodes -> {'skeleton': bool (nz, ny, nx) array, 'voxels', 'end_points', 'junction_voxels', 'isolated',
    'iterations'} (Python ints; iterations counts the last one, which cleared nothing; an empty volume reads 0).  The thinning
    is in voxel steps: it takes no spacing.  curve=True with connectivity=6 is a ValueError, before the first launch.
    voxel_data: the bool (nz, ny, nx) array the other calculations take; anything else is a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("skeleton_report needs a bool (nz, ny, nx) array")
    connectivity = pipeline._check_connectivity(connectivity)
    if curve and connectivity == 6:
        raise ValueError("curve=True needs connectivity=26: the curve skeleton is not defined under 6")
    vol = to_device_volume(voxel_data)
    skel, iterations = pipeline._skeleton(vol, bool(curve), connectivity, None)
    nodes = pipeline.skeleton_nodes(skel)
    return {'skeleton': pipeline.unpack(skel).cpu().numpy(), 'voxels': int(nodes.voxels), 'end_points': int(nodes.end_points),
            'junction_voxels': int(nodes.junction_voxels), 'isolated': int(nodes.isolated), 'iterations': int(iterations)}


def _branch_report_args(what, voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity, curve, prune_mm, prune_rounds):
    """The argument checks the branch reports share, all on the host -> (connectivity, prune_mm, prune_rounds)."""
    if not _on_device(voxel_data):
        raise TypeError("%s needs a bool (nz, ny, nx) array" % what)
    connectivity = pipeline._check_connectivity(connectivity)
    if curve and connectivity == 6:
        raise ValueError("curve=True needs connectivity=26: the curve skeleton is not defined under 6")
    prune_mm = float(prune_mm)
    if not prune_mm >= 0.0:
        raise ValueError("prune_mm must be non-negative")
    prune_rounds = pipeline._check_rounds(prune_rounds)
    nz = np.asarray(voxel_data).shape[0]
    pipeline.branch_steps(slice_depths, nz, mm_per_pixel_y, mm_per_pixel_x)            # the argument checks
    return connectivity, prune_mm, prune_rounds


def _branch_report(t, removed):
    """skeleton_branch_report's dict from a SkeletonBranches and the number of pruned branches."""
    b, n = t.branches, t.nodes
    total = 0.0
    for v in b.length_mm:                                               # in ascending label
        total += float(v)
    branch_table = [{'label': int(b.label[i]), 'voxels': int(b.voxels[i]), 'length_mm': float(b.length_mm[i]),
                     'chord_mm': float(b.chord_mm[i]), 'tortuosity': float(b.tortuosity[i]), 'kind': int(b.kind[i]),
                     'nodes': tuple(int(v) for v in b.nodes[i]), 'attach_index': tuple(int(v) for v in b.attach_index[i])}
                    for i in range(len(b))]
    node_table = [{'label': int(n.label[i]), 'voxels': int(n.voxels[i]), 'end_voxels': int(n.end_voxels[i]),
                   'junction_voxels': int(n.junction_voxels[i]), 'branches': int(n.branches[i]), 'free_end': bool(n.free_end[i]),
                   'centroid_mm': tuple(float(v) for v in n.centroid_mm[i])} for i in range(len(n))]
    return {'branches': len(b), 'nodes': len(n), 'free_ends': int(n.free_end.sum()),
            'junctions': int((~n.free_end & (n.branches > 0)).sum()), 'cycles': int((b.kind == 0).sum()), 'total_length_mm': total,
            'mean_branch_length_mm': total / len(b) if len(b) else 0.0, 'removed_branches': int(removed),
            'branch_table': branch_table, 'node_table': node_table}


def skeleton_branch_report(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity=26, curve=True, prune_mm=0.0,
                           prune_rounds=1):
    """The branch table of the skeleton of a volume (no counterpart in the reference; AnalyzeSkeleton of BoneJ answers the same
    question): the volume is thinned as skeleton_report thins it, short spurs are pruned when prune_mm > 0
    (pipeline.prune_skeleton: terminal branches shorter than prune_mm, prune_rounds rounds, None = until nothing goes), then
    pipeline.skeleton_branches -> {'branches', 'nodes', 'free_ends', 'junctions' (nodes that are no free end and have branches),
    'cycles', 'total_length_mm', 'mean_branch_length_mm' (0.0 without a branch), 'removed_branches', 'branch_table': one dict
    per branch {'label', 'voxels', 'length_mm', 'chord_mm', 'tortuosity', 'kind', 'nodes': (a, b), 'attach_index': (lo, hi)},
    'node_table': one dict per node {'label', 'voxels', 'end_voxels', 'junction_voxels', 'branches', 'free_end',
    'centroid_mm': (z, y, x)}}.  Lengths are in mm under the slice depths; the thinning itself is in voxel steps.  curve=True
    with connectivity=6 is a ValueError, before the first launch.  voxel_data: the bool (nz, ny, nx) array the other
    calculations take; anything else is a TypeError."""
    connectivity, prune_mm, prune_rounds = _branch_report_args("skeleton_branch_report", voxel_data, mm_per_pixel_x, mm_per_pixel_y,
                                                               slice_depths, connectivity, curve, prune_mm, prune_rounds)
    vol = to_device_volume(voxel_data)
    skel, _ = pipeline._skeleton(vol, bool(curve), connectivity, None)
    removed = 0
    if prune_mm > 0.0:
        pruned = pipeline.prune_skeleton(skel, prune_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x, prune_rounds)
        skel, removed = pruned.volume, pruned.removed_branches
    return _branch_report(pipeline.skeleton_branches(skel, slice_depths, mm_per_pixel_y, mm_per_pixel_x), removed)


def skeleton_thickness_report(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity=26, curve=True, prune_factor=1.0,
                              prune_mm=0.0, prune_rounds=None):
    """How wide the object is along its skeleton (no counterpart in the reference; Tb.Th along the skeleton in BoneJ, channel and
    throat radii of a pore-network model): the volume is thinned as skeleton_report thins it, pipeline.distance_transform of the
    OBJECT gives the radius at every voxel, spurs are pruned relative to it when prune_factor > 0 or prune_mm > 0
    (pipeline.prune_skeleton_relative: a terminal branch goes when it is shorter than max(prune_mm, prune_factor * the radius
    where it leaves its junction); prune_rounds rounds, None = until nothing goes), then pipeline.skeleton_branch_profile ->
    skeleton_branch_report's dict with, per branch, 'min_radius_mm', 'throat_index' (the flat index of the first voxel that
    attains it), 'max_radius_mm', 'mean_radius_mm' and 'component' -- the label under label_components(connectivity) of the
    object's component that holds the throat voxel --, per node 'radius_mm' (the largest over its voxels) and 'component', and
    overall 'mean_thickness_mm' = 2 (sum of sum_q / 65536) / (sum of voxels) over all branches (0.0 without one) and 'narrowest':
    {'label', 'radius_mm', 'index'} of the branch with the smallest throat, the lowest label among equals (None without a
    branch).  Argument errors are skeleton_branch_report's, and prune_factor negative or nan is a ValueError; all of them come
    before the first launch."""
    connectivity, prune_mm, prune_rounds = _branch_report_args("skeleton_thickness_report", voxel_data, mm_per_pixel_x, mm_per_pixel_y,
                                                               slice_depths, connectivity, curve, prune_mm, prune_rounds)
    prune_factor = pipeline._check_factor(prune_factor)
    vol = to_device_volume(voxel_data)
    skel, _ = pipeline._skeleton(vol, bool(curve), connectivity, None)
    radius = pipeline.distance_transform(vol, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    removed = 0
    if prune_factor > 0.0 or prune_mm > 0.0:
        pruned = pipeline.prune_skeleton_relative(skel, radius, prune_factor, prune_mm, slice_depths, mm_per_pixel_y, mm_per_pixel_x,
                                                  prune_rounds)
        skel, removed = pruned.volume, pruned.removed_branches
    profile = pipeline.skeleton_branch_profile(skel, radius, slice_depths, mm_per_pixel_y, mm_per_pixel_x)
    b, n = profile.branches, profile.nodes
    report = _branch_report(profile.table, removed)
    runs = pipeline.ComponentRuns(vol, connectivity)
    owner = runs.label_at(np.concatenate([b.min_index, n.max_index])).cpu().numpy()
    if runs.runs:
        runs._checked()                                                 # the guards of the lookup
    for i, row in enumerate(report['branch_table']):
        row.update({'min_radius_mm': float(b.min[i]), 'throat_index': int(b.min_index[i]), 'max_radius_mm': float(b.max[i]),
                    'mean_radius_mm': float(b.mean[i]), 'component': int(owner[i])})
    for i, row in enumerate(report['node_table']):
        row.update({'radius_mm': float(n.max[i]), 'component': int(owner[len(b) + i])})
    voxels = int(b.voxels.sum())
    report['mean_thickness_mm'] = 2.0 * (float(int(b.sum_q.sum())) / 65536.0) / voxels if voxels else 0.0
    report['narrowest'] = None
    if len(b):
        i = int(np.argmin(b.min))                                       # the first of equals: the lowest label
        report['narrowest'] = {'label': int(b.label[i]), 'radius_mm': float(b.min[i]), 'index': int(b.min_index[i])}
    return report


def component_properties(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, connectivity=6, min_voxels=0, largest=False,
                         shape=False, topology=False, surface=False, surface_directions=13, porosity=False, thickness=False,
                         thickness_radii_mm=None, geodesic=False, geodesic_sweeps=3, breadth=False, breadth_directions=13,
                         separate_mm=None, separate_h_mm=None, skeleton=False, caliper=False,
                         caliper_directions=None, caliper_oriented=False):
    """The calculations of the class per connected component (no counterpart in the reference, which would be handed the mask
    `labels == c` once per component) -> a list of dicts, one per component with at least min_voxels voxels (largest: only the
    largest of those), in label order: {'label', 'voxels', 'voxel_volume_mm3', 'bounding_box': {'x', 'y', 'z'}, 'dimensions',
    'centroid_mm': (z, y, x), 'centroid_index': (z, y, x)}.  voxel_volume_mm3, bounding_box and dimensions are the numbers
    calculate_voxel_volume_variable_depth / calculate_bounding_box_variable_depth return for that mask; centroid_mm is in the
    coordinates of largest_inscribed_sphere.  shape=True: every dict also carries the second moments of the component as a
    body of point masses, one per voxel, weighted with the voxel's volume (pipeline.component_moments; vectors in (z, y, x)
    order): 'center_of_mass_mm', 'covariance_mm2' (3 x 3 nested tuples), 'principal_variances_mm2' (descending),
    'principal_axes' (3 rows, unit vectors in that order) and 'ellipsoid_axes_mm' (the full axes of the solid ellipsoid with
    the same second moments).  topology=True: every dict also carries 'euler_number', 'cavities' (enclosed voids; one that
    reaches a face of the stack is none) and 'handles' (tunnels) of the component as Python ints (pipeline.component_topology:
    a ball reads 1, 0, 0, a hollow shell 2, 1, 0, a ring 0, 0, 1; the background has the complementary connectivity).
    surface=True: every dict also carries 'surface_area_mm2' -- the discretised Crofton formula on the component's voxels
    (pipeline.component_surface; surface_directions = 13 or 3; a voxel of another component is not background) -- and
    'sphericity' = pi^(1/3) (6 voxel_volume_mm3)^(2/3) / surface_area_mm2 as Python floats.  porosity=True: every dict also
    carries 'cavity_voxels' (int), 'cavity_volume_mm3' -- the volumes of the cavities the component owns (closed_porosity's
    table), added in ascending cavity label -- and 'closed_porosity' = cavity / (voxel_volume_mm3 + cavity).  thickness=True:
    every dict also carries the inscribed sphere of the component -- 'inscribed_radius_mm', 'inscribed_diameter_mm',
    'inscribed_center_index' (z, y, x) and 'inscribed_center_mm', as largest_inscribed_sphere gives them for the mask -- and, with
    thickness_radii_mm (ascending ball radii), its local thickness as thickness_statistics gives it for the mask:
    'thickness_mean_mm', 'thickness_std_mm', 'thickness_max_mm', 'thickness_uncovered_voxels' and 'thickness_histogram' =
    [(diameter_mm, voxels, volume_mm3), ...] (pipeline.component_thickness: one transform of the whole volume, never one per
    component).  caliper=True: every dict also carries the caliper (Feret) diameters of the component over caliper_directions
    (float (M, 3) unit vectors; None: pipeline.caliper_directions()), voxel extents included (pipeline.component_caliper):
    'max_caliper_mm', 'max_caliper_direction' (z, y, x), 'min_caliper_mm', 'min_caliper_direction', and with caliper_oriented
    also 'oriented_box_mm' -- the extents along the component's principal axes -- and 'oriented_box_center_mm' (z, y, x).
    geodesic=True (a keyword, like the other flags): every dict also carries 'geodesic_length_mm' -- the length of the component
    along itself, the repeated farthest-point search of pipeline.component_geodesic with geodesic_sweeps searches (at least 2) and
    the steps of `connectivity`, centre to centre: a lower bound of its geodesic diameter on the lattice metric --
    'geodesic_ends_index' (the two ends, (z, y, x) each) and 'tortuosity', that length over the straight distance of the ends.
    separate_mm=r (a keyword; None: off, nothing new is launched): touching objects are separated first -- the uploaded volume is
    replaced by pipeline.separate_components(volume, r, ..., connectivity).volume BEFORE the one labelling, so the rows, and every
    flag above, measure the separated grains (separate_grains returns that volume and its counts).  separate_h_mm=h (a keyword;
    None: off, nothing new is launched): the same with pipeline.separate_by_height(volume, h, ..., connectivity), the h-maxima
    markers of separate_grains_by_height; giving both separate_mm and separate_h_mm is a ValueError.
    skeleton=True (a keyword; off: nothing new is launched): every dict also carries 'skeleton_voxels', 'skeleton_ends' and
    'skeleton_junctions' as Python ints -- the voxels, free ends and junction voxels of the component's piece of the curve
    skeleton (pipeline.component_skeleton: ONE thinning of the whole volume under `connectivity`, counted under the runs of the
    one labelling; in voxel steps, the spacing plays no part).  The curve skeleton needs connectivity=26: skeleton=True with
    connectivity=6 is a ValueError.
    breadth=True (a keyword; off: nothing new is launched): every dict also carries 'mean_breadth_mm' -- the fourth Minkowski
    functional by the discretised Crofton formula on the component's voxels (pipeline.component_breadth; breadth_directions =
    13 or 3; for a convex grain the caliper diameter averaged over all directions) -- and 'mean_curvature_integral_mm' =
    2 pi mean_breadth_mm as Python floats.
    Whatever the
    flags, the volume is uploaded and labelled ONCE, and so is its complement: one pipeline.ComponentRuns serves all the
    measurements and owns the one selection their rows come from.  Arguments are checked before the first launch.  voxel_data: a bool (nz, ny, nx) array, else a TypeError."""
    if not _on_device(voxel_data):
        raise TypeError("component_properties needs a bool (nz, ny, nx) array")
    depths = np.asarray(slice_depths, dtype=np.float64).reshape(-1)
    rule = (min_voxels, largest)
    pipeline._check_connectivity(connectivity)
    tables = pipeline._slice_weights(depths, len(voxel_data), mm_per_pixel_y, mm_per_pixel_x)
    factors = pipeline.surface_factors(depths, len(voxel_data), mm_per_pixel_y, mm_per_pixel_x, surface_directions) if surface else None
    breadth_factors = pipeline.breadth_factors(depths, len(voxel_data), mm_per_pixel_y, mm_per_pixel_x, breadth_directions) if breadth else None
    if thickness:
        pipeline._component_thickness_args(voxel_data.shape, depths, mm_per_pixel_y, mm_per_pixel_x, thickness_radii_mm)
    if caliper:
        pipeline._caliper_args(voxel_data.shape, depths, mm_per_pixel_y, mm_per_pixel_x, caliper_directions, "voxels")
    if geodesic:
        pipeline._geodesic_search_sweeps(geodesic_sweeps)
        pipeline._geodesic_tables(voxel_data.shape, depths, mm_per_pixel_y, mm_per_pixel_x)
    if skeleton and connectivity == 6:
        raise ValueError("skeleton=True needs connectivity=26: the curve skeleton is not defined under 6")
    if separate_mm is not None and separate_h_mm is not None:
        raise ValueError("separate_mm and separate_h_mm are two marker rules: give one of them")
    if separate_mm is not None:
        pipeline._separation_args(voxel_data.shape, separate_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, 1)
    if separate_h_mm is not None:
        pipeline._height_args(voxel_data.shape, separate_h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity, 1, 0.0)
    vol = to_device_volume(voxel_data)
    if separate_mm is not None:
        vol = pipeline.separate_components(vol, separate_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity).volume
    if separate_h_mm is not None:
        vol = pipeline.separate_by_height(vol, separate_h_mm, depths, mm_per_pixel_y, mm_per_pixel_x, connectivity).volume
    runs = pipeline.ComponentRuns(vol, connectivity)
    if runs.select(*rule) is None:
        return []
    p = runs.properties(tables, mm_per_pixel_y, mm_per_pixel_x, *rule)
    boxes = [box_variable_depth(tuple(b), mm_per_pixel_x, mm_per_pixel_y, depths) for b in p.index_box]
    out = [{'label': int(p.labels[i]), 'voxels': int(p.voxels[i]), 'voxel_volume_mm3': float(p.volume_mm3[i]),
            'bounding_box': {axis: box[axis] for axis in ('x', 'y', 'z')}, 'dimensions': box['dimensions'],
            'centroid_mm': tuple(float(v) for v in p.centroid_mm[i]),
            'centroid_index': tuple(float(v) for v in p.centroid_index[i])} for i, box in enumerate(boxes)]
    q = runs.moments(tables, mm_per_pixel_y, mm_per_pixel_x, *rule) if shape else None
    t = runs.topology_rows(*rule) if topology else None
    a = runs.surface(factors, surface_directions, *rule) if surface else None
    h = runs.thickness(depths, mm_per_pixel_y, mm_per_pixel_x, thickness_radii_mm, *rule) if thickness else None
    f = runs.caliper(depths, mm_per_pixel_y, mm_per_pixel_x, caliper_directions, "voxels", caliper_oriented, *rule) if caliper else None
    g = runs.geodesic(depths, mm_per_pixel_y, mm_per_pixel_x, geodesic_sweeps, *rule) if geodesic else None
    k = runs.skeleton(*rule) if skeleton else None
    w = runs.breadth(breadth_factors, breadth_directions, *rule) if breadth else None
    pores = {}
    if porosity:                                                 # every cavity of the volume, credited to its owner
        c = pipeline._cavities_from(runs, runs.background().properties(tables, mm_per_pixel_y, mm_per_pixel_x, enclosed=True))
        for owner, n, v in zip(c.owner, c.voxels, c.volume_mm3):
            have = pores.get(int(owner), (0, 0.0))
            pores[int(owner)] = (have[0] + int(n), have[1] + float(v))
    for i, d in enumerate(out):                                  # row i of every answer: they come from the one selection of `runs`
        if shape:
            d['center_of_mass_mm'] = tuple(float(v) for v in q.center_of_mass_mm[i])
            d['covariance_mm2'] = tuple(tuple(float(v) for v in row) for row in q.covariance_mm2[i])
            d['principal_variances_mm2'] = tuple(float(v) for v in q.principal_variances_mm2[i])
            d['principal_axes'] = tuple(tuple(float(v) for v in row) for row in q.principal_axes[i])
            d['ellipsoid_axes_mm'] = tuple(float(v) for v in q.ellipsoid_axes_mm[i])
        if topology:
            d['euler_number'], d['cavities'], d['handles'] = int(t.euler[i]), int(t.cavities[i]), int(t.handles[i])
        if surface:
            d['surface_area_mm2'] = float(a.surface_area_mm2[i])
            d['sphericity'] = sphericity(d['voxel_volume_mm3'], d['surface_area_mm2'])
        if porosity:
            d['cavity_voxels'], d['cavity_volume_mm3'] = pores.get(d['label'], (0, 0.0))
            whole = d['voxel_volume_mm3'] + d['cavity_volume_mm3']
            d['closed_porosity'] = d['cavity_volume_mm3'] / whole if whole else 0.0
        if thickness:
            d['inscribed_radius_mm'] = float(h.radius_mm[i])
            d['inscribed_diameter_mm'] = 2 * d['inscribed_radius_mm']
            d['inscribed_center_index'] = tuple(int(v) for v in h.center_index[i])
            d['inscribed_center_mm'] = tuple(float(v) for v in h.center_mm[i])
            if h.radii_mm is not None:
                d['thickness_mean_mm'], d['thickness_std_mm'] = float(h.mean_mm[i]), float(h.std_mm[i])
                d['thickness_max_mm'], d['thickness_uncovered_voxels'] = float(h.max_mm[i]), int(h.uncovered_voxels[i])
                d['thickness_histogram'] = [(2.0 * float(r), int(n), float(v))
                                            for r, n, v in zip(h.radii_mm, h.level_voxels[i], h.level_volume_mm3[i])]
        if caliper:
            d['max_caliper_mm'] = float(f.max_mm[i])
            d['max_caliper_direction'] = tuple(float(v) for v in f.max_direction[i])
            d['min_caliper_mm'] = float(f.min_mm[i])
            d['min_caliper_direction'] = tuple(float(v) for v in f.min_direction[i])
            if caliper_oriented:
                d['oriented_box_mm'] = tuple(float(v) for v in f.oriented_extent_mm[i])
                d['oriented_box_center_mm'] = tuple(float(v) for v in f.oriented_center_mm[i])
        if geodesic:
            d['geodesic_length_mm'] = float(g.length_mm[i])
            d['geodesic_ends_index'] = tuple(tuple(int(v) for v in end) for end in g.ends_index[i])
            d['tortuosity'] = float(g.tortuosity[i])
        if skeleton:
            d['skeleton_voxels'], d['skeleton_ends'] = int(k.skeleton_voxels[i]), int(k.end_points[i])
            d['skeleton_junctions'] = int(k.junction_voxels[i])
        if breadth:
            d['mean_breadth_mm'] = float(w.mean_breadth_mm[i])
            d['mean_curvature_integral_mm'] = 2.0 * math.pi * d['mean_breadth_mm']
    return out


class VolumeCalculator:
    """Handles volume calculations and object property analysis (reference: volume_calculator.py:10)."""

    def __init__(self):
        pass

    def calculate_voxel_volume(self, voxel_data: np.ndarray, mm_per_pixel_x: float,
                               mm_per_pixel_y: float, mm_per_slice: float) -> float:
        """:16-21: number of set voxels times the volume of one."""
        if _on_device(voxel_data):
            n_set = np.int64(int(pipeline.popcount_async(to_device_volume(voxel_data)).item()))
        else:
            n_set = np.sum(voxel_data)
        return n_set * (mm_per_pixel_x * mm_per_pixel_y * mm_per_slice)

    def calculate_voxel_volume_variable_depth(self, voxel_data: np.ndarray, mm_per_pixel_x: float,
                                              mm_per_pixel_y: float, slice_depths: np.ndarray) -> float:
        """:23-35."""
        if len(slice_depths) == 0:
            return 0.0
        return volume_from_slice_counts(slice_counts(voxel_data), mm_per_pixel_x, mm_per_pixel_y, slice_depths)

    def calculate_bounding_box(self, voxel_data: np.ndarray, mm_per_pixel_x: float,
                               mm_per_pixel_y: float, mm_per_slice: float) -> dict:
        """:37-57.  An empty volume is an error there too (the minimum of an empty index array)."""
        box = index_box(voxel_data)
        if box is None:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        return box_uniform_depth(box, mm_per_pixel_x, mm_per_pixel_y, mm_per_slice)

    def calculate_bounding_box_variable_depth(self, voxel_data: np.ndarray, mm_per_pixel_x: float,
                                              mm_per_pixel_y: float, slice_depths: np.ndarray) -> dict:
        """:59-94: all zeros for an empty volume or an empty depth table."""
        return box_variable_depth(index_box(voxel_data), mm_per_pixel_x, mm_per_pixel_y, slice_depths)

    def calculate_density(self, volume: float, x_length_mm: float,
                          y_length_mm: float, total_depth_mm: float) -> float:
        """:96-100: the share of the x * y * depth block the volume fills."""
        return volume / (x_length_mm * y_length_mm * total_depth_mm)

    def analyze_object_properties(self, voxel_data: np.ndarray, processed_volume: float,
                                  mesh_volume: float, surface_area: float,
                                  mm_per_pixel_x: float, mm_per_pixel_y: float,
                                  slice_depths: np.ndarray, x_length_mm: float,
                                  y_length_mm: float, total_depth_mm: float) -> dict:
        """:102-132: the report (four lines, the surface-area line only for a non-zero area) and the property dict.
        The density is taken over the summed slice depths, not over `total_depth_mm`; the mesh volume, when there is
        one, is the headline volume."""
        box = self.calculate_bounding_box_variable_depth(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths)
        dims = box['dimensions']
        headline = processed_volume if mesh_volume is None else mesh_volume
        fill = self.calculate_density(headline, x_length_mm, y_length_mm, np.sum(slice_depths))
        report = [f"Volume: {headline:.4f} mm³", f"Dimensions: {dims[0]:.2f} x {dims[1]:.2f} x {dims[2]:.2f} mm"]
        if surface_area:
            report.append(f"Surface Area: {surface_area:.4f} mm²")
        report.append(f"Density: {100*fill:.1f}% of total space")
        print("\n".join(report))
        return {
            'volume_mm3': headline,
            'voxel_volume_mm3': self.calculate_voxel_volume_variable_depth(voxel_data, mm_per_pixel_x, mm_per_pixel_y,
                                                                          slice_depths),
            'processed_voxel_volume_mm3': processed_volume,
            'mesh_volume_mm3': mesh_volume,
            'bounding_box': {axis: box[axis] for axis in ('x', 'y', 'z')},
            'dimensions': dims,
            'surface_area_mm2': surface_area,
            'density': fill,
        }
