#!/usr/bin/env python3
"""Time ``utils.eye_density`` on device-resident records of 2^20 and 2^24 samples (sps = 16, 200 bins, sigma = 5, every trace) beside two things:
a device-to-device ``ssfm_device_copy`` of the record's bytes (what one pass over the record costs at best), and the route a caller had before --
download the record, ``np.histogram2d``, ``scipy.ndimage.gaussian_filter`` on the host.

The device figures are HIP events around the call on the default stream, where the library's kernels run (torch supplies the events and nothing
else); they include the call's host-side work between its launches.  The host route is a host clock.  Median (min) over --reps calls after two
untimed ones, in ms.

    python tools/eye_density_time.py [--reps 20] [--out profiles/eye_density_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, utils  # noqa: E402


def by_events(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(np.min(t))


def by_clock(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: nothing is measured without one")
    torch.cuda.init()                                              # (before the library's first call, as tools/signal_ops_times.py does)
    from scipy.ndimage import gaussian_filter
    sps, B, sigma = 16, 200, 5
    rng = np.random.default_rng(0)
    lines = [f"sps = {sps}, {B} bins, sigma = {sigma}, every trace; {args.reps} timed calls after two untimed ones; ms: median (min)"]
    for log2n in (20, 24):
        n = 1 << log2n
        h = rng.integers(0, 2, n).astype(np.float64) + 0.1 * rng.standard_normal(n)
        d = _lib.DeviceArray.from_host(h)
        dst = _lib.DeviceArray((n,), np.float64)
        lines.append(f"n = 2^{log2n} samples ({8 * n >> 20} MiB)")
        med, mn = by_events(lambda: _lib.api.ssfm_device_copy(0, dst, d, 8 * n, _lib.COPY_D2D), args.reps)
        lines.append(f"  {'device-to-device copy':<44} {med:9.4f} ({mn:9.4f})   [device events]")
        med, mn = by_events(lambda: utils.eye_density(d, sps, None, B, sigma), args.reps)
        lines.append(f"  {'eye_density':<44} {med:9.4f} ({mn:9.4f})   [device events]")
        med, mn = by_events(lambda: utils.eye_density(d, sps, 4096, B, sigma, colors=True), args.reps)
        lines.append(f"  {'eye_density, 4096 traces, colors=True':<44} {med:9.4f} ({mn:9.4f})   [device events]")

        def host_route():
            y = d.to_host()
            Y = y[sps // 2:sps // 2 + (n - 2 * (sps // 2)) // (2 * sps) * 2 * sps]
            X = np.tile(np.linspace(-1, 1 - 1 / sps, 2 * sps), Y.size // (2 * sps))
            return gaussian_filter(np.histogram2d(X, Y, bins=B)[0], sigma=sigma)
        med, mn = by_clock(host_route, max(3, args.reps // 5))
        lines.append(f"  {'download + histogram2d + gaussian_filter':<44} {med:9.4f} ({mn:9.4f})   [host clock]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
