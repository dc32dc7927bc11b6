"""CPU tier of the slice histogram passes: one refusal table for the histogram entry points tomo_cc_zhist, tomo_cc_moment_hist and
tomo_branch_hist and the finishing entry points tomo_cc_zsums, tomo_cc_moments and tomo_cc_level_sums (csrc/cc_runs.h: the
shared argument checks).  Every call is refused before anything is launched, so the pointers are host pointers that are never
dereferenced and no GPU is needed.  -1: an argument is wrong, -3: a size is beyond what the kernels index; the geometry is judged
first, then the arguments, then the sizes.  What tests/test_component_props_cpu.py, test_component_moments_cpu.py,
test_component_thickness_cpu.py and test_branches_cpu.py assert already is left to them (ASSERTED)."""
import ctypes

import pytest

from tomography_3d_reconstructor_amd import _lib

_BUFS = [(ctypes.c_uint64 * 8)() for _ in range(16)]
_PTR = [ctypes.addressof(b) for b in _BUFS]                       # distinct, non-null, never dereferenced

HIST = ["bits", "nz", "ny", "nx", "row_off", "cap_runs", "parent", "rank", "tot", "table", "cap", "sel", "off", "hist", "hist_cap"]
FINISH = ["table", "cap", "tot", "sel", "off", "slot", "hist", "hist_cap"]
ENTRIES = {                                                       # name: (parameters, uint64 per histogram entry)
    "tomo_cc_zhist": (HIST, 1),
    "tomo_cc_moment_hist": (HIST, 6),
    "tomo_branch_hist": (HIST + ["other"], 11),
    "tomo_cc_zsums": (FINISH + ["w", "zc", "nz", "out", "labels", "cap_sel"], 1),
    "tomo_cc_moments": (FINISH + ["w", "zc", "nz", "mm_y", "mm_x", "out", "labels", "cap_sel"], 6),
    "tomo_cc_level_sums": (FINISH + ["w", "nz", "levels", "voxels", "volume", "labels", "cap_sel"], 4),        # levels + 1
}
SCALARS = {"nz": 4, "ny": 4, "nx": 4, "cap_runs": 8, "cap": 8, "hist_cap": 8, "cap_sel": 8, "mm_y": 1.0, "mm_x": 1.0, "levels": 3}
CAPACITIES = ("cap_runs", "cap", "hist_cap", "cap_sel")

ASSERTED = {                                                      # (entry point, case) that another CPU test asserts
    "tomo_cc_zhist": {"null bits", "null hist", "zero hist_cap", "nx = -1", "cap at 2^31", "hist_cap at the bound"},
    "tomo_cc_moment_hist": {"null bits", "null hist", "null sel", "zero hist_cap", "nx = -1", "zero cap_runs", "cap at 2^31",
                            "cap_runs at 2^31", "2^31 words", "past the 63-bit bound"},
    "tomo_branch_hist": {"null " + p for p in HIST + ["other"] if p not in SCALARS}
                        | {"zero " + p for p in CAPACITIES} | {"negative " + p for p in CAPACITIES} | {"nz = 0", "ny = 0", "nx = 0", "nz = -1", "2^31 words", "cap at 2^31",
                                                               "cap_runs at 2^31", "hist_cap at the bound", "hist is bits", "hist is other"},
    "tomo_cc_zsums": {"null table", "null w", "null labels", "nz = 0", "zero cap_sel", "cap_sel at 2^31"},
    "tomo_cc_moments": {"null table", "null hist", "null w", "null labels", "zero cap", "zero hist_cap", "nz = 0", "zero cap_sel",
                        "cap at 2^31", "cap_sel at 2^31", "mm_y = 0", "mm_x = 0", "mm_y = nan", "mm_x = nan", "mm_y = inf", "mm_x = inf"},
    "tomo_cc_level_sums": {"null hist", "null w", "null volume", "levels = -1", "nz = 0", "cap_sel at 2^31"},
}


def good(name):
    params = ENTRIES[name][0]
    return {p: SCALARS[p] if p in SCALARS else _PTR[i] for i, p in enumerate(params)}


def refusals(name):
    """(case, the arguments that differ from a good call, the code the entry point answers)."""
    params, words = ENTRIES[name]
    hist_side = "bits" in params
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
    for p in ("cap_runs", "cap", "cap_sel"):
        if p in params:
            out.append(("%s at 2^31" % p, {p: 1 << 31}, -3))
    out.append(("hist_cap at the bound", {"hist_cap": (1 << 60) // words}, -3))     # 2^60 itself for one word
    out.append(("an argument before a size", {"cap": 1 << 31, "sel": None}, -1))
    if hist_side:
        big = {"nz": 1 << 12, "ny": 1 << 13, "nx": 1 << 12}        # 2^25 rows of 2^6 words
        out.append(("2^31 words", big, -3))
        out.append(("the geometry before an argument", dict(big, row_off=None), -3))
    if name == "tomo_branch_hist":
        out.append(("hist is bits", {"hist": _PTR[0]}, -1))
        out.append(("hist is other", {"hist": _PTR[params.index("other")]}, -1))
        out.append(("an alias before a size", {"hist": _PTR[0], "cap_runs": 1 << 31}, -1))
    if name == "tomo_cc_moment_hist":                             # ny * nx * max(ny, nx)^2 >= 2^63, in far fewer than 2^31 words
        out.append(("past the 63-bit bound", {"nz": 1, "ny": 1 << 21, "nx": 1 << 21}, -3))
        out.append(("2^63 exactly", {"nz": 1, "ny": 1, "nx": 1 << 21}, -3))
        out.append(("an argument before the 63-bit bound", {"nz": 1, "ny": 1, "nx": 1 << 21, "rank": None}, -1))
        out.append(("one voxel below 2^63, then a null", {"nz": 1, "ny": 1, "nx": (1 << 21) - 1, "off": None}, -1))
    if name == "tomo_cc_moments":
        for p in ("mm_y", "mm_x"):
            for what, bad in (("0", 0.0), ("-1", -1.0), ("nan", float("nan")), ("inf", float("inf"))):
                out.append(("%s = %s" % (p, what), {p: bad}, -1))
    if name == "tomo_cc_level_sums":
        out.append(("levels = -1", {"levels": -1}, -1))
        out.append(("levels = -1 before a size", {"levels": -1, "cap": 1 << 31}, -1))
        out.append(("more threads than a grid", {"cap": 1 << 30, "levels": (1 << 31) - 2}, -3))
    return [case for case in out if case[0] not in ASSERTED[name]]


CASES = [(name, *case) for name in ENTRIES for case in refusals(name)]


def test_the_table_names_cases_of_every_entry_point_and_only_new_ones():
    for name in ENTRIES:
        told = {c[1] for c in CASES if c[0] == name}
        assert told and not told & ASSERTED[name], name
        assert len(_lib.SIGNATURES[name][1]) == len(ENTRIES[name][0]) + 1, name      # + the stream
    assert len(CASES) == len({c[:2] for c in CASES})


@pytest.mark.parametrize("name,case,change,code", CASES, ids=["%s-%s" % (c[0][5:], c[1].replace(" ", "_")) for c in CASES])
def test_a_bad_call_is_refused_without_a_gpu(name, case, change, code):
    args = good(name)
    assert set(change) <= set(args), (name, case)
    args.update(change)
    assert getattr(_lib.lib(), name)(*args.values(), None) == code, (name, case)
