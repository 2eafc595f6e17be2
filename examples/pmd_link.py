#!/usr/bin/env python3
"""Polarisation-mode dispersion on the Manakov line: ``FIBER(coupling="manakov", pmd=D_p)``, the coarse-step (waveplate) model with one section per step.

A pair of Gaussian pulses, one in each polarisation, through 100 km of an otherwise ideal fibre (no loss, dispersion or nonlinearity, so that PMD is all
that happens) in 100 steps of 1 km, for 16 seeds at D_p = 0.1 and 1 ps/sqrt(km).  Printed per coefficient:

* the rms width of the pair's power envelope behind the fibre, its mean and its spread over the seeds, beside the input's;
* the rms differential group delay over seeds and frequencies beside ``D_p sqrt(L)``.  The fibre is linear here, so two runs per seed -- the pulse in x
  alone, then in y alone -- give its Jones matrix ``T(w)`` at every frequency the pulse lights, and ``DGD(w) = 2 sqrt|det dT/dw|``.

    python examples/pmd_link.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticomlib_amd import FIBER, gv, optical_signal, workloads  # noqa: E402

N, T0_PS, LENGTH, H, SEEDS = 1 << 12, 10.0, 100.0, 1.0, 16


def pulse():
    """(t [ps], Gaussian field of rms power width T0 / sqrt(2), unit energy)"""
    t = (np.arange(N) - N // 2) * gv.dt * 1e12
    p = np.exp(-t ** 2 / (2 * T0_PS ** 2))
    return t, p / np.sqrt(np.sum(p ** 2))


def rms_width(t, power):
    m = np.sum(t * power) / np.sum(power)
    return float(np.sqrt(np.sum((t - m) ** 2 * power) / np.sum(power)))


def jones(y_x, y_y, p, band):
    """T(w) at the bins ``band`` from the fibre's answers to the pulse in x alone and in y alone: columns Y / X."""
    X = np.fft.fft(p)[band]
    Yx, Yy = np.fft.fft(y_x, axis=-1)[:, band] / X, np.fft.fft(y_y, axis=-1)[:, band] / X
    return np.stack([Yx, Yy], axis=-1).transpose(1, 0, 2)                     # (bins, 2, 2)


def dgd(T, dw):
    """2 sqrt|det dT/dw| by central differences along the (contiguous) bins: T in SU(2) makes dT/dw T^-1 traceless with eigenvalues +- i DGD / 2."""
    dT = (T[2:] - T[:-2]) / (2 * dw)
    return 2 * np.sqrt(np.abs(np.linalg.det(dT)))


def main(fiber=FIBER):
    gv(**workloads.BENCH_GV)
    t, p = pulse()
    zero = np.zeros_like(p)
    w = np.fft.fftfreq(N, gv.dt) * 2 * np.pi * 1e-12                             # rad/ps
    order = np.argsort(w)
    band = order[np.abs(w[order]) < 0.1]                                        # contiguous in frequency: where the pulse has light
    dw = 2 * np.pi / (N * gv.dt * 1e12)
    ideal = dict(length=LENGTH, h=H, alpha=0.0, beta_2=0.0, beta_3=0.0, gamma=0.0, precision="complex128", coupling="manakov")
    print(f"pulse pair of rms width {rms_width(t, p ** 2):.2f} ps, {LENGTH:.0f} km in {int(LENGTH / H)} sections, {SEEDS} seeds")
    for dp in (0.1, 1.0):
        widths, delays, engine = [], [], None
        for seed in range(SEEDS):
            out_x = fiber(optical_signal(np.stack([p, zero])), pmd=dp, pmd_seed=seed, **ideal)
            out_y = fiber(optical_signal(np.stack([zero, p])), pmd=dp, pmd_seed=seed, **ideal)
            engine = out_x.engine
            y_x, y_y = np.asarray(out_x.signal), np.asarray(out_y.signal)
            pair = (y_x + y_y) / np.sqrt(2)                                     # (the fibre is linear: the pair's answer is the sum of the answers)
            widths.append(rms_width(t, np.sum(np.abs(pair) ** 2, axis=0)))
            delays.append(dgd(jones(y_x, y_y, p, band), dw))
        delays = np.array(delays)
        print(f"D_p = {dp:4.1f} ps/sqrt(km) [{engine}]: pair's rms width {np.mean(widths):6.2f} ps mean, {np.std(widths):5.2f} ps spread over seeds "
              f"({np.min(widths):.2f} ... {np.max(widths):.2f});  rms DGD {np.sqrt(np.mean(delays ** 2)):6.3f} ps beside D_p sqrt(L) = {dp * np.sqrt(LENGTH):6.3f} ps")


if __name__ == "__main__":
    main()
