#!/usr/bin/env python3
"""Time the binary_sequence algebra on the GPU at 2^20 and 2^26 bits: ``~a``, ``a ^ b``, ``a + b``, ``a * 16`` (of n / 16 bits, so the result
has n), ``a[::-1]``, ``a[3:]`` and ``.ones`` on device-resident sequences, beside a device-to-device ``ssfm_device_copy`` of n bytes (the
yardstick: ``~a`` and ``a[3:]`` move exactly a copy's traffic, ``a ^ b`` 1.5 times it, ``.ones`` half of it) and beside the route a caller had
before the class had operators: ``to_host``, NumPy, ``from_host``.

Per case: the median and the least wall time of a call (a host clock around work that ends in a device synchronise -- every entry point has
finished when it returns) over --reps calls after two untimed ones, its ratio to the copy's median, and the bytes the operation must move over
the median time.  A call includes its allocation from the library's pool and its launch.

    python tools/bits_time.py [--reps 30] [--out profiles/bits_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, binary_sequence  # noqa: E402


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    rng = np.random.default_rng(0)
    lines = [f"{args.reps} timed calls after two untimed ones; wall time of a call that has finished on the device when it returns [ms]: median (min); "
             "ratio = median / the copy's median; GB/s = the bytes the operation must move / median"]
    for log2n in (20, 26):
        n = 1 << log2n
        ha, hb = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
        up = lambda h: binary_sequence.from_device(_lib.DeviceArray.from_host(h))        # noqa: E731
        a, b, half, small = up(ha), up(hb), up(ha[: n // 2]), up(ha[: n // 16])
        dst = _lib.DeviceArray((n,), np.uint8)
        src = a._raw()
        copy = lambda: _lib.api.ssfm_device_copy(0, dst, src, n, _lib.COPY_D2D)          # noqa: E731
        c_med, c_min = timed(copy, args.reps)
        lines.append(f"n = 2^{log2n} bits")
        lines.append(f"  {'device-to-device copy':<28} {c_med:9.4f} ({c_min:9.4f})  ratio  1.00  {2 * n / c_med / 1e6:8.1f} GB/s")
        cases = [("~a", lambda: ~a, 2 * n), ("a ^ b", lambda: a ^ b, 3 * n), ("a + b (n/2 each)", lambda: half + half, 2 * n),
                 ("a * 16 (n/16 bits)", lambda: small * 16, n + n // 16), ("a[::-1]", lambda: a[::-1], 2 * n), ("a[3:]", lambda: a[3:], 2 * n),
                 (".ones", lambda: a.ones, n)]
        for name, fn, moved in cases:
            med, mn = timed(fn, args.reps)
            lines.append(f"  {name:<28} {med:9.4f} ({mn:9.4f})  ratio {med / c_med:5.2f}  {moved / med / 1e6:8.1f} GB/s")
        host = {"~a": lambda x: 1 - x, "a[3:]": lambda x: x[3:], ".ones": None}
        for name, f in host.items():                             # the earlier route: download, NumPy, upload
            def route():
                h = a._raw().to_host()
                if f is None:
                    return int(h.sum())
                return _lib.DeviceArray.from_host(np.ascontiguousarray(f(h)))
            med, mn = timed(route, max(3, args.reps // 6))
            lines.append(f"  {name + ' via the host':<28} {med:9.4f} ({mn:9.4f})  ratio {med / c_med:5.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
