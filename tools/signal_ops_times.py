#!/usr/bin/env python3
"""Time the device algebra of electrical_signal against what a user did before it existed (to_host, NumPy, upload), on one MI355X.

    python tools/signal_ops_times.py [out.txt]

For 2^20 and 2^24 float64 samples with noise (and filter() at the largest size it takes) (complex128 for phase()): the device events around `reps` calls of x * y, x * 2 + 1, x[::2],
x.power(), x.phase() and x.filter(h) with 129 taps; the host clock around the same result by download, NumPy / SciPy and upload; the bytes
each operation must move (inputs read once, outputs written once) over the device time, against the 6.29 TB/s copy rate of VERDICT.md.  The
entry points synchronise, so an event pair brackets whole calls (launch, kernel and the wait), not a kernel alone."""
import sys
import time

import numpy as np
import torch

from opticomlib_amd import NULL, _lib, electrical_signal

COPY_RATE = 6.29e12


def dev(s, n):
    up = lambda a: _lib.DeviceArray.from_host(np.ascontiguousarray(a))       # noqa: E731
    return electrical_signal.from_device(up(s), up(n))


RUNS = 7                     # timed windows per figure: the median is reported with the smallest and the largest


def device_ms(fn, reps):
    """(median, min, max) over RUNS windows of `reps` calls between two device events, after a warm-up of `reps` calls."""
    for _ in range(reps):
        fn()
    out = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def host_ms(fn, reps):
    """(median, min, max) over 3 windows of `reps` round trips by the host clock (each ends in a blocking copy)."""
    fn()
    out = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t) * 1e3 / reps)
    out.sort()
    return out[1], out[0], out[-1]


def roundtrip(x, f):
    """What the parent commit offers: copy signal and noise to the host, NumPy there, upload the result."""
    h = electrical_signal(x._raw("signal").to_host(), x._raw("noise").to_host())
    r = f(h)
    if isinstance(r, electrical_signal):
        dev(r.signal, r.noise if r.noise is not NULL else r.signal)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    torch.cuda.init()
    rng = np.random.default_rng(0)
    taps = np.hanning(129) / 64
    print(f"# device: {torch.cuda.get_device_name(0)}; times per call; bytes = inputs read once + outputs written once; share = bytes / time / 6.29 TB/s", file=out)
    print(f"# device ms: median (min - max) of {RUNS} windows of 50 (2^20) or 10 (larger) calls; host ms: median (min - max) of 3 windows; GB/s and share: of the median."
          "  Clocks and power state were not read; other work shares the host", file=out)
    print("# op | n | device ms | host round trip ms | bytes | GB/s | share of the copy rate", file=out)
    for n in (1 << 20, (1 << 22) - 128, 1 << 24):
        reps = 50 if n == 1 << 20 else 10
        x = dev(rng.standard_normal(n), rng.standard_normal(n) * 0.05)
        y = dev(rng.standard_normal(n), rng.standard_normal(n) * 0.05)
        z = dev(rng.standard_normal(n) + 1j * rng.standard_normal(n), (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05)
        hy = electrical_signal(y._raw("signal").to_host(), y._raw("noise").to_host())
        ops = [("x * y", x, lambda a: a * (y if a.on_device else hy), 6 * 8 * n),
               ("x * 2 + 1", x, lambda a: a * 2 + 1, 2 * 4 * 8 * n),
               ("x[::2]", x, lambda a: a[::2], 2 * 8 * n + 2 * 8 * (n // 2)),
               ("x.power()", x, lambda a: a.power(), 2 * 8 * n),
               ("x.phase() c128", z, lambda a: a.phase(), 2 * 16 * n + 8 * n),
               ("x.filter(h129)", x, lambda a: a.filter(taps), 4 * 8 * n)]
        if n == (1 << 22) - 128:                 # the largest signal filter() takes with 129 taps (a plan of 2^22 points): that row alone
            ops = ops[-1:]
        for name, sig, f, nbytes in ops:
            try:
                d, dlo, dhi = device_ms(lambda: f(sig), reps)
            except ValueError as e:              # filter(): the plan sizes end at 2^22 points
                print(f"{name} | {n} | not run: {e}", file=out)
                continue
            h, hlo, hhi = host_ms(lambda: roundtrip(sig, f), max(2, reps // 5))
            rate = nbytes / (d * 1e-3)
            print(f"{name} | {n} | {d:.4f} ({dlo:.4f} - {dhi:.4f}) | {h:.3f} ({hlo:.3f} - {hhi:.3f}) | {nbytes} | {rate / 1e9:.1f} | {rate / COPY_RATE:.3f}", file=out)
    print("# at 2^20 samples a call is a launch and a wait for it (tens of microseconds): the share of the copy rate there says nothing about the kernels;"
          " phase() and filter() are several launches (angle, wraps, a three-launch scan, the sum; two FFT passes and a table), their bytes are the"
          " minimum of the operation, not what those launches move", file=out)


if __name__ == "__main__":
    main()
