"""Which engine a call takes, on the device: plan.last_run_info()["engine"] at the smallest shape that reaches each engine of the fixed-step, the adaptive and
the capture entry points, against a literal table.  The rules themselves are opticomlib_amd/csrc/ssfm_route.hpp (tests/test_route_cpu.py holds them to the
host file's earlier decisions without a GPU); tools/route_sweep.py runs the cells and, under a kernel trace, lists the launches behind them.

An engine whose workgroups meet inside one launch may find the chip shared and repeat its run on another engine (`fell_back`).  Such a cell asserts the
documented fallback engine instead and counts as not checked; more than a quarter of the one-launch cells in that state fails the file."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import route_sweep  # noqa: E402

pytestmark = pytest.mark.gpu

# cell -> (engine, the engine a run that fell back is repeated on)
FIXED = {
    "fixed small":                 ("small", None),
    "fixed medium":                ("medium", "two_kernel"),                 # 8192 x 2
    # 2^14 x 2 with one distinct step: complex64 has the one-XCD engine up to 2^17 samples in all, complex128 the two-kernel engine with tables
    "fixed medium 2^14":           ("medium", "two_kernel"),
    "fixed two_kernel one step":   ("two_kernel", None),
    "fixed two_kernel fly":        ("two_kernel", None),                     # kMaxTables + 1 distinct steps
    "fixed two_kernel snapshots":  ("two_kernel", None),
    "fixed small snapshots":       ("small", None),
    "fixed split":                 ("split", None),                          # 2^21 x 1 under SSFM_SPLIT_ABOVE=20
}
ADAPTIVE = {
    "adaptive small":              ("small_adaptive", None),                 # 2048 x 2
    "adaptive medium":             ("medium_adaptive", "adaptive_3_launches"),      # 4096 x 2
    "adaptive fused":              ("adaptive_fused", "adaptive_3_launches"),       # 2^16 x 2 complex128
    "adaptive 3 launches capture": ("adaptive_3_launches", None),            # 2^16 x 2 with capture
    "adaptive split":              ("split_adaptive", None),
}
CAPTURE = {"capture two_kernel": ("two_kernel", None)}                       # propagate_fixed_capture at 2^14 x 2
fell_back_cells = []


def _check(table):
    assert set(table) <= set(route_sweep.CELLS)
    for cell, (engine, fallback) in table.items():
        info = route_sweep.run_cell(cell)
        print(cell, info["engine"], "fell_back" if info["fell_back"] else "", info["launches"])
        if info["fell_back"]:
            assert engine in route_sweep.ONE_LAUNCH and fallback is not None and info["engine"] == fallback, (cell, info)
            fell_back_cells.append(cell)
        else:
            assert info["engine"] == engine, (cell, info)
    one_launch = [c for t in (FIXED, ADAPTIVE, CAPTURE) for c, (e, _) in t.items() if e in route_sweep.ONE_LAUNCH]
    assert 4 * len(fell_back_cells) <= len(one_launch), ("too many one-launch cells fell back", fell_back_cells)


def test_fixed_step_routes():
    _check(FIXED)


def test_adaptive_routes():
    _check(ADAPTIVE)


def test_capture_route():
    _check(CAPTURE)


def test_every_cell_of_the_sweep_is_in_a_table():
    assert set(route_sweep.CELLS) == set(FIXED) | set(ADAPTIVE) | set(CAPTURE)
