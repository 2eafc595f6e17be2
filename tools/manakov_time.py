#!/usr/bin/env python3
"""Time the Manakov line (``FIBER(coupling="manakov")``, csrc/manakov.hip) at 2 x 2^20 samples: us per step, complex64 and complex128, with a fixed step and
with the adaptive rule, beside the scalar ``FIBER`` of the same plan on the same schedule and beside a device-to-device copy of the field's bytes taken in
the same run (the convention of tools/field_ops_time.py: the pointwise pass of a step is a streaming kernel, so the copy is its yardstick).

A fixed-step run is timed at the plan level -- the field is in the plan, ``--steps`` steps are queued, the clock stops when the plan's stream has drained --
so that neither upload nor download is in the figure.  The adaptive runs are whole calls on a device-resident input; their step count is the run's own.
Per case: the median and the least of --reps runs after two untimed ones.

    python tools/manakov_time.py [--steps 200] [--reps 7] [--out profiles/manakov_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, devices, gv, workloads  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    gv(**workloads.BENCH_GV)
    n = 1 << args.log2n
    a = workloads.qpsk_field(n, seed=1, power_w=10e-3)
    smf = workloads.SMF
    lines = [f"2 x 2^{args.log2n} samples, {args.reps} timed runs after two untimed ones; us per step: median (min); fixed step: {args.steps} steps of 0.1 km queued on a "
             "plan that holds the field, clock stopped when its stream has drained; adaptive: length 30 km, phi_max 0.01, the run's own step count"]
    for prec, dtype in ((_lib.C64, np.complex64), (_lib.C128, np.complex128)):
        rt = np.float32 if prec == _lib.C64 else np.float64
        F = 2 * n * np.dtype(dtype).itemsize
        x = _lib.DeviceArray.from_host(a.astype(dtype))
        dst = _lib.DeviceArray((2, n), dtype)
        c_med, c_min = timed(lambda: _lib.api.ssfm_device_copy(0, dst, x, F, _lib.COPY_D2D), args.reps)
        lines.append(f"{np.dtype(dtype).name} ({F / 2 ** 20:.0f} MiB a field)")
        lines.append(f"  {'device-to-device copy of the field':<44} {c_med:9.1f} ({c_min:9.1f}) us  {2 * F / c_med / 1e3:8.1f} GB/s")
        plan = devices.get_plan(n, 2, prec)
        g = float(rt(rt(smf["gamma"]) * rt(devices.MANAKOV_KAPPA)))
        hs = np.full(args.steps, rt(0.1), dtype=rt)
        with plan.lock:
            plan.set_linear_operator(devices.linear_operator(n, gv.dt, smf["alpha"], smf["beta_2"], smf["beta_3"], prec))

            def fixed(run):
                plan.set_field_device(x.ptr)
                plan.synchronize()
                t0 = time.perf_counter()
                run()
                plan.synchronize()
                return 1e6 * (time.perf_counter() - t0) / args.steps

            def series(run):
                fixed(run)
                fixed(run)
                t = [fixed(run) for _ in range(args.reps)]
                return float(np.median(t)), float(np.min(t))

            for name, run in (("manakov, fixed step", lambda: plan.manakov_propagate(g, hs)), ("scalar FIBER, fixed step", lambda: plan.propagate_fixed(smf["gamma"], hs))):
                med, mn = series(run)
                lines.append(f"  {name:<44} {med:9.2f} ({mn:9.2f}) us per step  = {med / c_med:5.2f} copies  [{plan.last_run_info()['engine']}]")

            def adaptive(run):
                plan.set_field_device(x.ptr)
                plan.synchronize()
                t0 = time.perf_counter()
                steps = run()
                plan.synchronize()
                return 1e6 * (time.perf_counter() - t0) / steps, steps

            for name, run in (("manakov, adaptive", lambda: plan.manakov_propagate(g, None, length=30.0, phi_max=0.01)[0]),
                              ("scalar FIBER, adaptive", lambda: plan.propagate_adaptive(smf["gamma"], 30.0, 0.01, False)[0])):
                adaptive(run)
                adaptive(run)
                got = [adaptive(run) for _ in range(args.reps)]
                t = [v[0] for v in got]
                lines.append(f"  {name:<44} {np.median(t):9.2f} ({np.min(t):9.2f}) us per step  = {np.median(t) / c_med:5.2f} copies  "
                             f"[{plan.last_run_info()['engine']}, {got[0][1]} steps]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
