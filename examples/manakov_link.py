#!/usr/bin/env python3
"""A polarisation-multiplexed field through 20 km of standard fibre, twice: with the reference's model (each polarisation a scalar fibre of its own) and
with Manakov coupling, ``FIBER(coupling="manakov")`` -- the nonlinear phase of each polarisation follows the power in both.

Prints how far apart the two results are, and the one property that tells the models apart without a reference: a fixed rotation of the
polarisation axes ahead of the fibre is the same rotation behind it for the Manakov model, and not for the per-polarisation one.

    python examples/manakov_link.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticomlib_amd import DBP, FIBER, gv, optical_signal, workloads  # noqa: E402


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def main():
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 16, seed=1, power_w=10e-3)                       # (2, N): 10 mW per polarisation
    fibre = dict(length=20, h=0.5, **workloads.SMF)
    scalar = FIBER(optical_signal(a), **fibre)
    manakov = FIBER(optical_signal(a), coupling="manakov", **fibre)                # kappa = 8/9
    print(f"engines: {scalar.engine} / {manakov.engine}")
    print(f"Manakov against per-polarisation, max|d|/peak: {rel(manakov.signal, scalar.signal):.3f}")
    theta, phi = 0.7, 0.4
    U = np.array([[np.cos(theta), -np.sin(theta) * np.exp(-1j * phi)], [np.sin(theta) * np.exp(1j * phi), np.cos(theta)]])
    for name, kw in (("per polarisation", {}), ("manakov", {"coupling": "manakov"})):
        turned_first = FIBER(optical_signal(U @ a), **fibre, **kw).signal
        turned_after = U @ FIBER(optical_signal(a), **fibre, **kw).signal
        print(f"FIBER(U A) against U FIBER(A), {name}: {rel(turned_first, turned_after):.2e}")
    back = DBP(manakov, coupling="manakov", **fibre)                               # the result never left the GPU
    print(f"DBP(FIBER(A)) against A, manakov: {rel(back.signal, a):.2e}")
    z, A_z = FIBER(optical_signal(a), length=20, phi_max=0.05, return_steps=True, z_list=[0, 5, 10, 20], coupling="manakov", **workloads.SMF)
    print("adaptive run, snapshots at z =", np.round(z, 3), "mean power [mW]:", np.round(1e3 * np.mean(np.abs(A_z) ** 2, axis=(1, 2)) * 2, 3))


if __name__ == "__main__":
    main()
