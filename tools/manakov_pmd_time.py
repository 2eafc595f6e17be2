#!/usr/bin/env python3
"""Time the Manakov-PMD line (``FIBER(coupling="manakov", pmd=...)``, csrc/manakov.hip ``ssfm_manakov_pmd_propagate``) at 2 x 2^20 samples: us per fixed
step and per adaptive step, complex64 and complex128, beside the plain Manakov line (``ssfm_manakov_propagate``, whose kernels this library builds as the
parent commit built them) on the same schedule in the same run, and beside a device-to-device copy of the field's bytes (the convention of
tools/manakov_time.py).  Nothing is asserted and no speed is claimed: the figures say what the per-row tables and the unitary cost.

A fixed-step run is timed at the plan level -- the field is in the plan, ``--steps`` steps are queued, the clock stops when the plan's stream has drained.
The PMD run's figure includes what a call stages once (w brought into table order, the quaternions of an adaptive run), spread over its steps.
The adaptive runs' step count is the run's own.  Per case: the median and the least of --reps runs after two untimed ones.

    python tools/manakov_pmd_time.py [--steps 200] [--reps 7] [--out profiles/manakov_pmd_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticomlib_amd import _lib, devices, gv, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--dp", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    gv(**workloads.BENCH_GV)
    n = 1 << args.log2n
    a = workloads.qpsk_field(n, seed=1, power_w=10e-3)
    smf = workloads.SMF
    max_steps = 1 << 12
    lines = [f"2 x 2^{args.log2n} samples, D_p = {args.dp} ps/sqrt(km), {args.reps} timed runs after two untimed ones; us per step: median (min); fixed step: "
             f"{args.steps} steps of 0.1 km queued on a plan that holds the field, clock stopped when its stream has drained; adaptive: length 30 km, "
             f"phi_max 0.01, max_steps {max_steps}, the run's own step count"]
    for prec, dtype in ((_lib.C64, np.complex64), (_lib.C128, np.complex128)):
        rt = np.float32 if prec == _lib.C64 else np.float64
        F = 2 * n * np.dtype(dtype).itemsize
        x = _lib.DeviceArray.from_host(a.astype(dtype))
        dst = _lib.DeviceArray((2, n), dtype)

        def copy():
            t0 = time.perf_counter()
            _lib.api.ssfm_device_copy(0, dst, x, F, _lib.COPY_D2D)
            return 1e6 * (time.perf_counter() - t0)

        copy(), copy()
        c = [copy() for _ in range(args.reps)]
        c_med = float(np.median(c))
        lines.append(f"{np.dtype(dtype).name} ({F / 2 ** 20:.0f} MiB a field)")
        lines.append(f"  {'device-to-device copy of the field':<44} {c_med:9.1f} ({np.min(c):9.1f}) us  {2 * F / c_med / 1e3:8.1f} GB/s")
        plan = devices.get_plan(n, 2, prec)
        g = float(rt(rt(smf["gamma"]) * rt(devices.MANAKOV_KAPPA)))
        hs = np.full(args.steps, rt(0.1), dtype=rt)
        w = devices._grid_w(n, float(gv.dt), prec)
        U_fixed, U_adaptive = devices.pmd_sections(1, args.steps), devices.pmd_sections(1, max_steps)
        pmd = dict(dp=args.dp, w=w)
        with plan.lock:
            plan.set_linear_operator(devices.linear_operator(n, gv.dt, smf["alpha"], smf["beta_2"], smf["beta_3"], prec))

            def once(run):
                plan.set_field_device(x.ptr)
                plan.synchronize()
                t0 = time.perf_counter()
                steps = run()[0]
                plan.synchronize()
                return 1e6 * (time.perf_counter() - t0) / steps, steps

            cases = (("manakov, fixed step", lambda: plan.manakov_propagate(g, hs)),
                     ("manakov-pmd, fixed step", lambda: plan.manakov_pmd_propagate(g, hs, sections=U_fixed, **pmd)),
                     ("manakov-pmd, fixed step, no scattering", lambda: plan.manakov_pmd_propagate(g, hs, **pmd)),
                     ("manakov, adaptive", lambda: plan.manakov_propagate(g, None, length=30.0, phi_max=0.01, max_steps=max_steps)),
                     ("manakov-pmd, adaptive", lambda: plan.manakov_pmd_propagate(g, None, sections=U_adaptive, length=30.0, phi_max=0.01, max_steps=max_steps, **pmd)))
            for name, run in cases:
                once(run), once(run)
                got = [once(run) for _ in range(args.reps)]
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
