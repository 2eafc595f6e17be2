#!/usr/bin/env python3
"""Time the optical_signal algebra on the GPU at 2 x 2^20 samples, complex64 and complex128: ``x + y``, ``x - y``, ``x * y`` (with and
without noise), ``x + row`` (an ``(N,)`` field over both polarisations), ``x * 1.5``, ``-x``, ``x.conj()``, ``x / (2 - 1j)``, ``x ** 2``,
``x[:, ::-1]``, ``x[1, a:b]``, ``x == y`` and ``x.power()`` on device-resident fields, beside a device-to-device ``ssfm_device_copy`` of one
field's bytes taken in the same run.  These are streaming kernels, so the copy is the yardstick: per case the file states the bytes the
operation must move, its time, its ratio to the copy's time and to the time the copy would need for those bytes.

Per case: the median and the least wall time of a call (a host clock around work that ends in a device synchronise -- every entry point has
finished when it returns) over --reps calls after two untimed ones.  A call includes its allocations from the library's pool and its launch.

    python tools/field_ops_time.py [--reps 30] [--out profiles/field_ops_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, optical_signal  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    rng = np.random.default_rng(0)
    n = 1 << args.log2n
    lines = [f"{args.reps} timed calls after two untimed ones; wall time of a call that has finished on the device when it returns [ms]: median (min); "
             "ratio = median / the copy's median; per byte = the same with the copy scaled to the bytes the operation must move; GB/s = those bytes / median"]
    for dtype in (np.complex64, np.complex128):
        item = np.dtype(dtype).itemsize
        mk = lambda shape: ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 0.1).astype(dtype)      # noqa: E731
        up = lambda a: _lib.DeviceArray.from_host(a)                                                                  # noqa: E731
        x, y = optical_signal.from_device(up(mk((2, n)))), optical_signal.from_device(up(mk((2, n))))
        xn, yn = optical_signal.from_device(up(mk((2, n))), up(mk((2, n)))), optical_signal.from_device(up(mk((2, n))), up(mk((2, n))))
        row = optical_signal.from_device(up(mk((n,))))
        F = 2 * n * item                                           # one field's bytes
        src, dst = x._raw("signal"), _lib.DeviceArray((2, n), dtype)
        copy = lambda: _lib.api.ssfm_device_copy(0, dst, src, F, _lib.COPY_D2D)          # noqa: E731
        c_med, c_min = timed(copy, args.reps)
        lines.append(f"{np.dtype(dtype).name}, 2 x 2^{args.log2n} samples ({F / 2 ** 20:.0f} MiB a field)")
        lines.append(f"  {'device-to-device copy':<30} {c_med:9.4f} ({c_min:9.4f})  ratio  1.00  per byte  1.00  {2 * F / c_med / 1e6:8.1f} GB/s")
        g = np.float32(1.5) if dtype == np.complex64 else 1.5      # (a Python float widens a complex64 field, as in the reference)
        cases = [("x + y", lambda: x + y, 3 * F), ("x - y", lambda: x - y, 3 * F), ("x * y", lambda: x * y, 3 * F),
                 ("x + y, both with noise", lambda: xn + yn, 6 * F), ("x * y, both with noise", lambda: xn * yn, 6 * F),
                 ("x + row (N,)", lambda: x + row, 2.5 * F), (f"x * {type(g).__name__}(1.5)", lambda: x * g, 2 * F), ("-x", lambda: -x, 2 * F),
                 ("x.conj()", lambda: x.conj(), 2 * F), ("x / (2 - 1j)", lambda: x / (2 - 1j), 2 * F), ("x ** 2", lambda: x ** 2, 2 * F),
                 ("x[:, ::-1]", lambda: x[:, ::-1], 2 * F), ("x[1, n/4:3n/4]", lambda: x[1, n // 4: 3 * n // 4], F / 2),
                 ("x == y (and its read)", lambda: x == y, 2 * F + 2 * n), ("x.power()", lambda: x.power(), F)]
        for name, fn, moved in cases:
            med, mn = timed(fn, args.reps)
            lines.append(f"  {name:<30} {med:9.4f} ({mn:9.4f})  ratio {med / c_med:5.2f}  per byte {med / (c_med * moved / (2 * F)):5.2f}  {moved / med / 1e6:8.1f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
