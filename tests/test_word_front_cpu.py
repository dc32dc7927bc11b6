"""CPU tier of the word passes and the row writers: one refusal table for the entry points whose kernels share the word pass front
and the selected-row guard of csrc/cc_runs.h -- tomo_cc_value_max, tomo_cc_value_first, tomo_cc_value_rows, tomo_profile_stats,
tomo_profile_where, tomo_profile_rows, tomo_cc_level_hist, tomo_cc_topology_rows, tomo_cc_caliper_rows, tomo_thin_count,
tomo_branch_attach and tomo_branch_clear.  Every call is refused before anything is launched, so the pointers are host pointers
that are never dereferenced and no GPU is needed.  -1: an argument is wrong, -3: a size is beyond what the kernels index.  The code
of every case is the one the library answered before the kernels got their shared front; where the entry points differ in the ORDER
of their checks the table says so: tomo_cc_value_first refuses best == first before it judges the geometry, tomo_branch_attach
judges its arguments before the geometry, everything else the geometry first, then the arguments, then the sizes.
tomo_cc_caliper_rows' bound cap_sel * M < 2^57 cannot fire on its own (cap_sel < 2^31 and M <= 65535 * 8 keep the product below
2^50), so only the bound on M has a case.  What tests/test_branch_profile_cpu.py, test_component_thickness_cpu.py,
test_caliper_cpu.py, test_skeleton_cpu.py, test_branches_cpu.py and test_topology_cpu.py assert already is left to them (ASSERTED)."""
import ctypes

import pytest

from tomography_3d_reconstructor_amd import _lib

_BUFS = [(ctypes.c_uint64 * 8)() for _ in range(20)]
_PTR = [ctypes.addressof(b) for b in _BUFS]                       # distinct, non-null, never dereferenced

RUNS = ["bits", "nz", "ny", "nx", "row_off", "cap_runs", "parent", "rank", "tot"]
ENTRIES = {
    "tomo_cc_value_max": RUNS + ["dist", "d2", "best", "cap"],
    "tomo_cc_value_first": RUNS + ["dist", "d2", "best", "first", "cap"],
    "tomo_cc_value_rows": ["table", "best", "first", "cap", "tot", "sel", "slot", "out", "cap_sel"],
    "tomo_profile_stats": RUNS + ["values", "lo", "hi", "sum", "cap"],
    "tomo_profile_where": RUNS + ["values", "lo", "hi", "lo_first", "hi_first", "cap"],
    "tomo_profile_rows": ["table", "lo", "hi", "sum", "lo_first", "hi_first", "cap", "tot", "sel", "slot", "out", "cap_sel"],
    "tomo_cc_level_hist": RUNS + ["table", "cap", "sel", "off", "hist", "hist_cap", "level", "levels"],
    "tomo_cc_topology_rows": ["table", "topo", "cap", "tot", "sel", "slot", "out", "cap_sel"],
    "tomo_cc_caliper_rows": ["table", "cap", "tot", "sel", "slot", "hi", "lo", "M", "width", "rows", "ext", "cap_sel"],
    "tomo_thin_count": RUNS + ["other", "sel", "slot", "out", "column", "columns", "cap", "cap_sel"],
    "tomo_branch_attach": RUNS + ["other", "sel", "slot", "attach", "attach_count", "cap", "cap_sel"],
    "tomo_branch_clear": RUNS + ["flagged", "n_flagged", "in", "out"],
}
SCALARS = {"nz": 4, "ny": 4, "nx": 4, "cap_runs": 8, "cap": 8, "hist_cap": 8, "cap_sel": 8, "levels": 3, "M": 3, "column": 0,
           "columns": 3, "n_flagged": 8, "d2": None}              # d2: a good call brings dist, and d2 NULL
CAPACITIES = ("cap_runs", "cap", "hist_cap", "cap_sel", "n_flagged")
BOUNDED = ("cap_runs", "cap", "cap_sel")                          # refused at 2^31
BIG = {"nz": 1 << 12, "ny": 1 << 13, "nx": 1 << 12}              # 2^25 rows of 2^6 words

_GEOMETRY = {"nz = 0", "ny = 0", "nx = 0", "nz = -1", "2^31 words"}


def _all(name, *skip):
    """every pointer null, every capacity zero, negative and at 2^31: what the loops of the older files cover"""
    told = {"null " + p for p in ENTRIES[name] if p not in SCALARS}
    told |= {"%s %s" % (how, p) for p in CAPACITIES if p in ENTRIES[name] for how in ("zero", "negative")}
    told |= {"%s at 2^31" % p for p in BOUNDED if p in ENTRIES[name]}
    return told - set(skip)


ASSERTED = {                                                      # (entry point, case) that another CPU test asserts
    "tomo_cc_value_max": {"null bits", "null dist", "dist and d2 both given", "null best", "zero cap", "ny = 0", "cap_runs at 2^31"},
    "tomo_cc_value_first": {"null first", "first is best", "null dist"},
    "tomo_cc_value_rows": {"null table", "zero cap_sel", "cap at 2^31"},
    "tomo_profile_stats": _all("tomo_profile_stats") | _GEOMETRY | {"hi is lo", "sum is lo", "sum is hi", "lo is bits", "hi is bits",
                                                                    "sum is bits", "lo is values", "hi is values", "sum is values"},
    "tomo_profile_where": _all("tomo_profile_where") | _GEOMETRY | {"%s is %s" % (x, y) for i, x in enumerate(("lo", "hi", "lo_first", "hi_first"))
                                                                    for y in ("bits", "values", "lo", "hi", "lo_first")[:2 + i]},
    "tomo_profile_rows": _all("tomo_profile_rows") | {"%s is %s" % (x, y) for i, x in enumerate(("lo", "hi", "sum", "lo_first", "hi_first", "out"))
                                                      for y in ("table", "lo", "hi", "sum", "lo_first", "hi_first")[:1 + i]},
    "tomo_cc_level_hist": {"null hist", "null level", "hist is level", "levels = -1", "zero hist_cap"},
    "tomo_cc_topology_rows": {"null table", "null out", "zero cap", "zero cap_sel", "cap at 2^31", "cap_sel at 2^31"},
    "tomo_cc_caliper_rows": {"null table", "hi is lo", "M = 0", "null width", "null rows", "null ext", "zero cap_sel", "cap_sel at 2^31",
                             "cap at 2^31"},
    "tomo_thin_count": _all("tomo_thin_count", "negative cap", "negative cap_sel") | _GEOMETRY
                       | {"zero columns", "column = -1", "column = columns", "out is bits", "out is other"},
    "tomo_branch_attach": _all("tomo_branch_attach") | _GEOMETRY | {"attach_count is attach", "attach is bits", "attach_count is other"},
    "tomo_branch_clear": _all("tomo_branch_clear") | _GEOMETRY | {"out is in", "out is bits", "n_flagged above cap_runs"},
}


def good(name):
    return {p: SCALARS[p] if p in SCALARS else _PTR[i] for i, p in enumerate(ENTRIES[name])}


def _alias(name, x, y, code=-1):
    return ("%s is %s" % (x, y), {x: _PTR[ENTRIES[name].index(y)]}, code)


def refusals(name):
    """(case, the arguments that differ from a good call, the code the entry point answers)."""
    params = ENTRIES[name]
    word_side = "bits" in params
    out = []
    for p in params:
        if p not in SCALARS:
            out.append(("null " + p, {p: None}, -1))
    for p in CAPACITIES:
        if p in params:
            out.append(("zero " + p, {p: 0}, -1))
            out.append(("negative " + p, {p: -1}, -1))
    for p in ("nz", "ny", "nx"):
        if p in params:
            out.append(("%s = 0" % p, {p: 0}, -1))
            out.append(("%s = -1" % p, {p: -1}, -1))
    for p in BOUNDED:
        if p in params:
            out.append(("%s at 2^31" % p, {p: 1 << 31}, -3))
    size = "cap" if "cap" in params else "cap_runs"
    out.append(("an argument before a size", {size: 1 << 31, "tot": None}, -1))
    if not word_side:
        out.append(("both capacities at 2^31", {"cap": 1 << 31, "cap_sel": 1 << 31}, -3))
    if word_side:
        out.append(("2^31 words", BIG, -3))
        # tomo_branch_attach alone judges its arguments before the geometry
        out.append(("the geometry before an argument", dict(BIG, row_off=None), -1 if name == "tomo_branch_attach" else -3))
        out.append(("the geometry before a size", dict(BIG, cap_runs=1 << 31), -3))
        out.append(("a bad shape before an argument", {"ny": 0, "rank": None}, -1))
    if name in ("tomo_cc_value_max", "tomo_cc_value_first"):
        both = _PTR[params.index("d2")]
        out.append(("dist and d2 both given", {"d2": both}, -1))
        out.append(("d2 alone, then a size", {"dist": None, "d2": both, "cap": 1 << 31}, -3))      # d2 alone is a good call
        out.append(("both maps before a size", {"d2": both, "cap": 1 << 31}, -1))
        out.append(("the geometry before both maps", dict(BIG, d2=both), -3))
    if name == "tomo_cc_value_first":
        out.append(_alias(name, "first", "best"))
        # ... and that refusal stands in front of the geometry and of the sizes
        out.append(("first is best before the geometry", dict(BIG, first=_PTR[params.index("best")]), -1))
        out.append(("first is best before a bad shape", {"nz": 0, "first": _PTR[params.index("best")]}, -1))
        out.append(("first is best before a size", {"cap_runs": 1 << 31, "first": _PTR[params.index("best")]}, -1))
    if name in ("tomo_profile_stats", "tomo_profile_where"):
        arrays = params[params.index("lo"):params.index("cap")]
        for i, x in enumerate(arrays):
            for y in ["bits", "values"] + arrays[:i]:
                out.append(_alias(name, x, y))
        out.append(("an alias before a size", {"hi": _PTR[params.index("lo")], "cap": 1 << 31}, -1))
        out.append(("a null before an alias", {"hi": _PTR[params.index("lo")], "row_off": None}, -1))
        out.append(("the geometry before an alias", dict(BIG, hi=_PTR[params.index("lo")]), -3))
    if name == "tomo_profile_rows":
        arrays = ["lo", "hi", "sum", "lo_first", "hi_first", "out"]
        for i, x in enumerate(arrays):
            for y in ["table"] + arrays[:i]:
                out.append(_alias(name, x, y))
        out.append(("an alias before a size", {"out": _PTR[params.index("lo")], "cap_sel": 1 << 31}, -1))
    if name == "tomo_cc_level_hist":
        out.append(_alias(name, "hist", "level"))
        out.append(("levels = -1", {"levels": -1}, -1))
        out.append(("levels = -1 before a size", {"levels": -1, "cap": 1 << 31}, -1))
        out.append(("hist_cap at the bound", {"hist_cap": (1 << 60) // 4}, -3))                # levels + 1 words per entry
        out.append(("hist_cap at the bound of one level", {"hist_cap": 1 << 60, "levels": 0}, -3))
        out.append(("an alias before a size", {"hist": _PTR[params.index("level")], "hist_cap": 1 << 60}, -1))
    if name == "tomo_cc_caliper_rows":
        out.append(_alias(name, "hi", "lo"))
        out.append(("M = 0", {"M": 0}, -1))
        out.append(("M = -1", {"M": -1}, -1))
        out.append(("M past the grid's rows", {"M": 65535 * 8 + 1}, -3))
        out.append(("M = 0 before a size", {"M": 0, "cap_sel": 1 << 31}, -1))
        out.append(("an alias before a size", {"hi": _PTR[params.index("lo")], "cap": 1 << 31}, -1))
    if name == "tomo_thin_count":
        out.append(("zero columns", {"columns": 0}, -1))
        out.append(("negative columns", {"columns": -1}, -1))
        out.append(("column = -1", {"column": -1}, -1))
        out.append(("column = columns", {"column": 3}, -1))
        out.append(("column past columns", {"column": 4}, -1))
        out.append(("column = columns = 1", {"column": 1, "columns": 1}, -1))
        out.append(("column before a size", {"column": 3, "cap_sel": 1 << 31}, -1))
        out.append(_alias(name, "out", "bits"))
        out.append(_alias(name, "out", "other"))
        out.append(("an alias before a size", {"out": _PTR[0], "cap": 1 << 31}, -1))
    if name == "tomo_branch_attach":
        for x, y in (("attach_count", "attach"), ("attach", "bits"), ("attach", "other"), ("attach_count", "bits"),
                     ("attach_count", "other")):
            out.append(_alias(name, x, y))
        out.append(("an alias before the geometry", dict(BIG, attach=_PTR[0]), -1))
        out.append(("an alias before a size", {"attach": _PTR[0], "cap_sel": 1 << 31}, -1))
        out.append(("a zero capacity before the geometry", dict(BIG, cap=0), -1))
    if name == "tomo_branch_clear":
        out.append(_alias(name, "out", "in"))
        out.append(_alias(name, "out", "bits"))
        out.append(("n_flagged above cap_runs", {"n_flagged": 9}, -1))
        out.append(("n_flagged above cap_runs before a size", {"n_flagged": (1 << 31) + 1, "cap_runs": 1 << 31}, -1))
        out.append(("n_flagged = cap_runs at 2^31", {"n_flagged": 1 << 31, "cap_runs": 1 << 31}, -3))
        out.append(("an alias before a size", {"out": _PTR[0], "n_flagged": 1 << 31, "cap_runs": 1 << 31}, -1))
    return [case for case in out if case[0] not in ASSERTED[name]]


CASES = [(name, *case) for name in ENTRIES for case in refusals(name)]


def test_the_table_names_cases_of_every_entry_point_and_only_new_ones():
    for name in ENTRIES:
        told = {c[1] for c in CASES if c[0] == name}
        assert told and not told & ASSERTED[name], name
        assert len(_lib.SIGNATURES[name][1]) == len(ENTRIES[name]) + 1, name          # + the stream
        codes = {c[3] for c in CASES if c[0] == name}
        assert codes == {-1, -3}, name                               # every entry point here has both
    assert len(CASES) == len({c[:2] for c in CASES})


@pytest.mark.parametrize("name,case,change,code", CASES, ids=["%s-%s" % (c[0][5:], c[1].replace(" ", "_")) for c in CASES])
def test_a_bad_call_is_refused_without_a_gpu(name, case, change, code):
    args = good(name)
    assert set(change) <= set(args), (name, case)
    args.update(change)
    assert getattr(_lib.lib(), name)(*args.values(), None) == code, (name, case)
