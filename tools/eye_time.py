#!/usr/bin/env python3
"""Time the OOK receiver on the GPU: GET_EYE(nslots=8192, sps_resamp=128) and ook.DSP on a Gaussian DAC word with sigma = 0.05 noise,
at 1024 and 8192 bits x 64 samples per bit (the inputs of the CPU figures in DESIGN.md).  Reports the wall time per call after a first
call, the kernel time of a call between two HIP events on the default stream (torch), and the host round trips of GET_EYE.

    python tools/eye_time.py [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opticomlib_amd as oa  # noqa: E402
from opticomlib_amd import ook  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rows = []
    for bits in (1024, 8192):
        oa.gv(sps=64, R=1e9, N=bits)
        x = oa.DAC(oa.PRBS(order=15, len=bits), pulse_shape="gaussian")
        v = np.real(np.asarray(x.signal)) + np.random.default_rng(0).normal(0, 0.05, x.size)
        dev_sig = oa.devices._wrap_out(oa.electrical_signal, oa._lib.DeviceArray.from_host(v, np.float64), oa.NULL)
        row = {"bits": bits, "samples": int(v.size)}
        for name, fn in (("GET_EYE", lambda s: oa.GET_EYE(s, nslots=8192, sps_resamp=128)), ("DSP", lambda s: ook.DSP(s))):
            fn(dev_sig)                                                    # first call: plans, chirp tables, code objects
            wall, kern = [], []
            for _ in range(a.reps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                start.record()
                res = fn(dev_sig)
                end.record()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(start.elapsed_time(end))
            e = res if name == "GET_EYE" else res[1]
            row[name] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "event_ms_median": float(np.median(kern)),
                         "round_trips": e.round_trips, "t_opt": e.t_opt, "i": e.i}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
