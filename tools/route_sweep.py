"""Walk the plan's routes: one short run at the smallest shape that reaches each engine of the fixed-step, the adaptive and the capture entry points
(opticomlib_amd/csrc/ssfm_route.hpp decides them; tests/test_routes_gpu.py holds the engines to a literal table).

    python tools/route_sweep.py                                   # prints one line per cell: name, engine, fell_back, launches
    rocprofv3 --kernel-trace --stats -- python tools/route_sweep.py    # ... and the kernels behind every route, with their template arguments and call counts

Two builds take the same routes exactly when the kernel names and their call counts of the second form agree (the lane-rating probes apart: how many of them
a plan launches depends on the hardware queue the runtime hands its second stream).  One process, nothing else traced."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_TABLES = 4          # csrc/ssfm_route.hpp kMaxTables: a schedule of more distinct step sizes forms exp(D~ h) in the row kernel
ONE_LAUNCH = ("small", "medium", "small_adaptive", "medium_adaptive", "adaptive_fused")       # engines whose workgroups meet inside the launch

# name -> (kind, log2 n, rows, precision, what the run asks for, environment set before the plan is made)
CELLS = {
    "fixed small":                 ("fixed", 8, 1, "c64", {}, {}),
    "fixed medium":                ("fixed", 13, 2, "c64", {}, {}),
    "fixed medium 2^14":           ("fixed", 14, 2, "c64", {}, {}),
    "fixed two_kernel one step":   ("fixed", 14, 2, "c128", {}, {}),
    "fixed two_kernel fly":        ("fixed", 14, 2, "c64", {"distinct": MAX_TABLES + 1}, {}),
    "fixed two_kernel snapshots":  ("fixed", 14, 2, "c64", {"snapshots": True}, {}),
    "fixed small snapshots":       ("fixed", 8, 1, "c64", {"snapshots": True}, {}),
    "fixed split":                 ("fixed", 21, 1, "c64", {}, {"SSFM_SPLIT_ABOVE": "20"}),
    "adaptive small":              ("adaptive", 11, 2, "c64", {}, {}),
    "adaptive medium":             ("adaptive", 12, 2, "c64", {}, {}),
    "adaptive fused":              ("adaptive", 16, 2, "c128", {}, {}),
    "adaptive 3 launches capture": ("adaptive", 16, 2, "c64", {"snapshots": True}, {}),
    "adaptive split":              ("adaptive", 21, 1, "c64", {}, {"SSFM_SPLIT_ABOVE": "20"}),
    "capture two_kernel":          ("capture", 14, 2, "c64", {}, {}),
}
KNOBS = ("SSFM_SPLIT_ABOVE", "SSFM_SPLIT_LOG2M", "SSFM_E", "SSFM_EF", "SSFM_EF_FLY", "SSFM_LANES", "SSFM_SMALL", "SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_MEDIUM_SPLIT",
         "SSFM_ADAPT_FUSED", "SSFM_PHASE_TABLE", "SSFM_FORCE_FLY", "SSFM_FUSED_PATIENCE_TICKS")


def run_cell(name):
    """One cell: a plan of its own, a fibre's operator, a weak QPSK field, three fixed steps or an adaptive run of a short fibre with max_steps 64.
    Returns the plan's last_run_info() with `launches` added."""
    import opticomlib_amd as oa
    from opticomlib_amd import _lib, workloads
    from opticomlib_amd.typing import gv
    kind, log2n, rows, prec, ask, env = CELLS[name]
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    oa.devices.release_plans()
    try:
        n = 1 << log2n
        gv(**workloads.BENCH_GV)
        P, cd, rt = (_lib.C64, np.complex64, np.float32) if prec == "c64" else (_lib.C128, np.complex128, np.float64)
        a = workloads.qpsk_field(n, seed=7, n_pol=2, power_w=5e-3)[:rows].astype(cd)
        p = _lib.Plan(n, rows, P)
        try:
            p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, P))
            p.set_field(a)
            if kind == "fixed":
                hs = np.array([0.25] * 3 if "distinct" not in ask else [0.25 / (1 + i) for i in range(ask["distinct"])], dtype=rt)
                p.propagate_fixed(1.3, hs, snapshots=ask.get("snapshots", False))
            elif kind == "capture":
                p.propagate_fixed_capture(1.3, np.array([0.25] * 3, dtype=rt), every=2)
            else:
                p.propagate_adaptive(1.3, 0.5, 0.004, False, max_steps=64, snapshots=ask.get("snapshots", False))
            p.get_field()                                   # (waits for the run: a one-launch engine's verdict is in)
            info = dict(p.last_run_info())
            info["launches"] = p.last_propagate_ms()[1]
            return info
        finally:
            p.close()
    finally:
        oa.devices.release_plans()
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


if __name__ == "__main__":
    for cell in CELLS:
        r = run_cell(cell)
        print("%-30s %-22s fell_back=%d launches=%d" % (cell, r["engine"], r["fell_back"], r["launches"]), flush=True)
