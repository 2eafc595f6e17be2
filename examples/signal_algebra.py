#!/usr/bin/env python3
"""The signal algebra between devices, on the GPU: PD -> (x - sqrt(power)) * g -> x[:n] -> x.filter(h) -> x > thr.

Prints ``_lib.TRANSFERS`` before and after the chain: nothing is copied to the host between the photodetector and the decided bits
(``power()`` reads one scalar inside the library; the taps of ``h`` are the one upload).

    python examples/signal_algebra.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticomlib_amd import DAC, LASER, MZM, PD, PRBS, _lib, gv  # noqa: E402


def main():
    gv(sps=16, R=10e9, N=4096)
    bits = PRBS(order=15, len=4096)
    field = MZM(LASER(P0=3.0), DAC(bits, Vpp=3.0, offset=-1.5), bias=0.0, Vpi=6.0)
    x = PD(field, BW=7.5e9, rng="device")
    print("PD output:", x)
    before = dict(_lib.TRANSFERS)
    y = (x - x.power() ** 0.5) * 20.0            # remove the rms level, apply a gain
    y = y[: 4000 * gv.sps]                       # keep 4000 bit slots
    h = np.hanning(2 * gv.sps + 1)
    y = y.filter(h / h.sum())                    # a matched-filter-like smoothing
    decided = y[gv.sps // 2:: gv.sps] > 0.0      # sample and decide
    after = dict(_lib.TRANSFERS)
    print("transfers before:", before)
    print("transfers after: ", after)
    print(f"device-to-host copies between PD and the bits: {after['d2h'] - before['d2h']}; result on the GPU: {y.on_device}")
    assert after["d2h"] == before["d2h"] and y.on_device
    print("decided bits:", decided, "ones:", decided.ones)


if __name__ == "__main__":
    main()
