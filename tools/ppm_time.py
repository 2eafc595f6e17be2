#!/usr/bin/env python3
"""Time the PPM receiver on the GPU: ppm.DSP soft, hard with the estimated threshold (GET_EYE(nslots=8192) + THRESHOLD_EST) and hard with a
given threshold, each hard variant with rng="numpy" and rng="device", at M = 16 and M = 256 on 2^20 slots x 32 samples per slot (rectangular
pulses of height 1 and sigma = 0.2 Gaussian noise, float64, device-resident).  Reports the wall time per call after a first call, the time
between two HIP events on the default stream (torch) and the bit errors against the transmitted word.

    python tools/ppm_time.py [--reps 5] [--slots 1048576] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opticomlib_amd as oa  # noqa: E402
from opticomlib_amd import ppm  # noqa: E402

SPS, SIGMA = 32, 0.2


def make_input(M, slots, seed=0):
    """(bits, signal) of `slots` PPM slots: host arrays, the same for any library that times them."""
    rng = np.random.default_rng(seed)
    k = int(np.log2(M))
    bits = rng.integers(0, 2, slots // M * k).astype(np.uint8)
    v = bits.reshape(-1, k).astype(np.int64) @ (1 << np.arange(k)[::-1])
    s = np.zeros(slots, np.float64)
    s[np.arange(v.size) * M + v] = 1.0
    return bits, np.repeat(s, SPS) + rng.normal(0, SIGMA, slots * SPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rows = []
    oa.device_rng_seed(1)
    for M in (16, 256):
        oa.gv(sps=SPS, R=1e9)
        bits, v = make_input(M, a.slots)
        dev_sig = oa.devices._wrap_out(oa.electrical_signal, oa._lib.DeviceArray.from_host(v, np.float64), oa.NULL)
        tx = oa.binary_sequence.from_device(oa._lib.DeviceArray.from_host(bits, np.uint8))
        row = {"M": M, "slots": a.slots, "sps": SPS, "samples": int(v.size), "sigma": SIGMA}
        cases = (("soft", dict(decision="soft")), ("hard_est_numpy", dict(decision="hard")), ("hard_est_device", dict(decision="hard", rng="device")),
                 ("hard_thr_numpy", dict(decision="hard", threshold=0.5)), ("hard_thr_device", dict(decision="hard", threshold=0.5, rng="device")))
        for name, kw in cases:
            np.random.seed(0)
            ppm.DSP(dev_sig, M, **kw)                                      # first call: code objects, pool
            wall, kern = [], []
            for _ in range(a.reps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                start.record()
                rx = ppm.DSP(dev_sig, M, **kw)
                end.record()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(start.elapsed_time(end))
            errs = round(ppm.BER_analizer("counter", Tx=tx, Rx=rx) * rx.size)
            row[name] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "event_ms_median": float(np.median(kern)),
                         "bit_errors": int(errs), "bits": int(rx.size), "rth": None if rx.rth is None else float(rx.rth)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
