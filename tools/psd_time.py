#!/usr/bin/env python3
"""Time get_psd on the GPU on device-resident inputs: the issue's SciPy figures (2^20 float64, 2 x 2^20 complex64 / complex128 at nperseg = 2048,
3.2 M complex128 at 8192 -- the reference's linewidth demo) and the other routes (nperseg = 3000 and 17 on the chirp-z route, 7 and the dual-polarisation default nperseg = 2 on the direct one).
Reports the wall time per call after a first call and the HIP-event time of a call on the default stream (torch; launches, kernels, the result's
copy).  With ``--stats`` (a rocprofv3 --kernel-trace --stats CSV of this script) the fast-path cases also get their kernels' average time and the
fraction of the HBM read floor (input bytes / 6.3 TB/s) it reaches.

    python tools/psd_time.py [--reps 20] [--out FILE]
    python tools/psd_time.py --merge profiles/psd_time.json --stats profiles/psd_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12        # measured stream read rate of the MI355X
# name, rows, n, dtype, nperseg, SciPy on the build host [ms] (8 cores, SciPy 1.15.3), the line length of the route-1 kernel
CASES = [
    ("f64_2^20_2048", 1, 1 << 20, "float64", 2048, 112.0, 2048),
    ("c64_2x2^20_2048", 2, 1 << 20, "complex64", 2048, 92.0, 2048),
    ("c128_2x2^20_2048", 2, 1 << 20, "complex128", 2048, 193.0, 2048),
    ("c128_3.2M_8192", 1, 3_200_000, "complex128", 8192, 244.0, 8192),
    ("c128_2x2^20_3000", 2, 1 << 20, "complex128", 3000, None, None),
    ("c128_2x2^20_17", 2, 1 << 20, "complex128", 17, None, None),
    ("c128_2x2^20_7", 2, 1 << 20, "complex128", 7, None, None),
    ("c64_2x2^20_default2", 2, 1 << 20, "complex64", None, None, None),
]


def run(reps):
    import torch
    import opticomlib_amd as oa
    from opticomlib_amd import _lib
    rows_out = []
    for name, rows, n, dt, nperseg, scipy_ms, _ in CASES:
        rng = np.random.default_rng(0)
        shape = (n,) if rows == 1 else (rows, n)
        x = rng.standard_normal(shape)
        if dt.startswith("complex"):
            x = x + 1j * rng.standard_normal(shape)
        d = _lib.DeviceArray.from_host(x.astype(dt))
        sig = oa.optical_signal.from_device(d)
        oa.get_psd(sig, 1.0, nperseg)                                  # first call: code objects, tables, plans
        wall, ev = [], []
        for _ in range(reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            f, p = oa.get_psd(sig, 1.0, nperseg)
            end.record()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(start.elapsed_time(end))
        row = {"case": name, "rows": rows, "n": n, "dtype": dt, "nperseg": nperseg if nperseg is not None else "default (2)",
               "input_bytes": int(d.nbytes), "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)),
               "event_ms_median": float(np.median(ev)), "scipy_ms_build_host": scipy_ms,
               "speedup_vs_scipy": None if scipy_ms is None else round(scipy_ms / float(np.median(wall)), 1)}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    return rows_out


def _pow2_kernel(name, dtype, L):
    """Is `name` (a demangled kernel name of the stats) k_welch_pow2 for this input type and line length?"""
    if "k_welch_pow2<" not in name or f", {L}>" not in name:
        return False
    if dtype == "float64":
        return "k_welch_pow2<double," in name
    if dtype == "complex64":
        return "float" in name
    return "double" in name and "k_welch_pow2<double," not in name


def merge(rows, stats_path):
    with open(stats_path) as fh:
        stats = list(csv.DictReader(fh))
    for row in rows:
        L = next((c[6] for c in CASES if c[0] == row["case"]), None)
        hit = [r for r in stats if L and _pow2_kernel(r["Name"], row["dtype"], L)]
        if not hit:
            continue
        ns = float(hit[0]["AverageNs"])
        row["kernel_name"] = hit[0]["Name"]
        row["kernel_avg_us"] = round(ns / 1e3, 2)
        row["hbm_read_floor_us"] = round(row["input_bytes"] / HBM_BPS * 1e6, 2)
        row["fraction_of_hbm_roofline"] = round(row["input_bytes"] / HBM_BPS / (ns * 1e-9), 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="add the kernel figures of --stats to this JSON file (no GPU needed)")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as fh:
            rows = json.load(fh)
        rows = merge(rows, a.stats)
        with open(a.merge, "w") as fh:
            json.dump(rows, fh, indent=1)
        return
    rows = run(a.reps)
    if a.stats:
        rows = merge(rows, a.stats)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
