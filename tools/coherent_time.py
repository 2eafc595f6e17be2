#!/usr/bin/env python3
"""Time the blind phase search (``coherent.CPR``, ``ssfm_cpr_search``) on the GPU beside a device-to-device ``ssfm_device_copy`` of the same
record, the project's usual yardstick, and the whole receiver ``coherent.DSP`` on a field of ``sps`` samples per symbol.

The search is not a streaming kernel: per symbol it forms ``B`` distances once and reads ``B (2 W + 1)`` of them back from LDS, so the file also
states the LDS bytes read per call and their rate.  Per case: the median and the least wall time of a call (a host clock around work that has
finished on the device when the call returns) over --reps calls after two untimed ones; a call includes its allocations from the library's pool
and its three launches.

    python tools/coherent_time.py [--reps 20] [--out profiles/coherent_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, coherent, gv, optical_signal  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t))


def record(rows, n, M, rng):
    k, L, a = coherent._ORDERS[M][0], coherent._ORDERS[M][1], coherent._half_spacing(M)
    lv = lambda: a * (2 * rng.integers(0, L, (rows, n)) - (L - 1))                  # noqa: E731
    theta = np.cumsum(rng.standard_normal((rows, n)) * 0.01, axis=1)
    return (lv() + 1j * lv()) * np.exp(1j * theta) + 0.03 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    rng = np.random.default_rng(0)
    lines = [f"{args.reps} timed calls after two untimed ones; wall time of a call that has finished on the device when it returns [ms]: median (min); "
             "copies = median / the median of a device-to-device copy of the record; LDS = B (2 W + 1) 8 bytes per symbol read back by the window sums"]
    for rows, log2n, M, B, W, dtype in ((2, 16, 16, 32, 32, np.complex128), (2, 16, 16, 32, 32, np.complex64), (2, 20, 16, 32, 32, np.complex128),
                                        (2, 20, 4, 32, 16, np.complex128), (2, 20, 64, 64, 32, np.complex128), (2, 20, 16, 32, 256, np.complex128),
                                        (1, 20, 16, 32, 0, np.complex128)):
        n = 1 << log2n
        x = _lib.DeviceArray.from_host(record(rows, n, M, rng).astype(dtype))
        dst = _lib.DeviceArray(x.shape, dtype)
        c_med, c_min = timed(lambda: _lib.api.ssfm_device_copy(0, dst, x, x.nbytes, _lib.COPY_D2D), args.reps)
        scale = np.ones(rows)
        med, mn = timed(lambda: coherent._search(x, rows, n, 0, 1, n, scale, M, B, W, 0), args.reps)
        lds = rows * n * B * (2 * W + 1) * 8
        lines.append(f"{rows} x 2^{log2n} symbols {np.dtype(dtype).name}, {M}-QAM, B = {B}, W = {W} ({x.nbytes / 2 ** 20:.0f} MiB a record)")
        lines.append(f"  {'device-to-device copy':<34} {c_med:9.4f} ({c_min:9.4f})  {2 * x.nbytes / c_med / 1e6:8.1f} GB/s")
        lines.append(f"  {'ssfm_cpr_search (three launches)':<34} {med:9.4f} ({mn:9.4f})  = {med / c_med:7.1f} copies   {rows * n / med / 1e3:8.1f} Msymbol/s   LDS {lds / med / 1e9:7.2f} TB/s")
        if W == 32 and B == 32 and dtype == np.complex128:
            p_med, p_min = timed(lambda: coherent._row_power(x, rows, n, 0, 1, n), args.reps)
            lines.append(f"  {'ssfm_cpr_power':<34} {p_med:9.4f} ({p_min:9.4f})  = {p_med / c_med:7.1f} copies")
    sps, log2n, M = 16, 20, 16
    gv(sps=sps, R=32e9)
    n = (1 << log2n) // sps
    sym = record(2, n, M, rng)
    field = np.zeros((2, 1 << log2n), np.complex64)
    field[:, sps // 2::sps] = sym
    f = optical_signal.from_device(_lib.DeviceArray.from_host(field))
    ref = tuple(coherent.QAM_ENCODER(coherent.QAM_DECODER(s, M), M) for s in sym)          # the nearest points: device-resident symbols
    d_med, d_min = timed(lambda: coherent.DSP(f, M, ref=ref), args.reps)
    lines.append(f"coherent.DSP of a 2 x 2^{log2n} complex64 field at {sps} samples per symbol, {M}-QAM, B = 32, W = 32, with ref (power, search, and per row: two sums, one decision)")
    lines.append(f"  {'DSP':<34} {d_med:9.4f} ({d_min:9.4f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
