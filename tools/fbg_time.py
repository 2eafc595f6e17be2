#!/usr/bin/env python3
"""Time FBG on the GPU at N = 2^12, 2^16 and 2^20: a uniform grating (fs = 100 GHz, vdneff = 1e-4, kL = 16) and a chirped one (fs = 400 GHz,
kL = 16, F = 20, rcos), print_params off.  Reports the wall time per call (median over --reps after one warm-up call), the accepted and
attempted RK45 steps and the blocking host waits of the solve, as JSON lines.

    python tools/fbg_time.py [--reps 3] [--max-log2n 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opticomlib_amd as oa  # noqa: E402
from opticomlib_amd.typing import gv, optical_signal  # noqa: E402

CASES = (("uniform", 100e9, dict(vdneff=1e-4, kL=16)), ("chirped", 400e9, dict(vdneff=1e-4, kL=16, F=20, apodization="rcos")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-log2n", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for log2n in (12, 16, 20):
        if log2n > a.max_log2n:
            continue
        n = 1 << log2n
        for name, fs, kw in CASES:
            gv(fs=fs)
            x = optical_signal(np.ones(n, complex))
            oa.FBG(x, fc=gv.f0, print_params=False, **kw)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                oa.FBG(x, fc=gv.f0, print_params=False, **kw)
                ts.append(time.perf_counter() - t)
            rec = dict(case=name, n=n, fs=fs, wall_s=float(np.median(ts)), steps=oa.FBG.last_steps, attempts=oa.FBG.last_attempts,
                       host_waits=oa.FBG.last_waits)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
