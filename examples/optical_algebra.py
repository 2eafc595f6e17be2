#!/usr/bin/env python3
"""The optical_signal algebra between devices, on the GPU: two modulated channels are combined, amplified, cut and indexed.

    (ch1 + ch2) * g  ->  x[:n]  ->  x[0, a:b], np.abs(x), x.power()

Prints ``_lib.TRANSFERS`` before and after the algebra: nothing crosses PCIe between the modulators and the photodetector (``power()``
reads its numbers inside the library).

    python examples/optical_algebra.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticomlib_amd import DAC, LASER, MZM, PD, PRBS, _lib, gv  # noqa: E402


def main():
    gv(sps=16, R=10e9, N=4096)
    drive = lambda seed: DAC(PRBS(order=15, len=4096, seed=seed), Vpp=3.0, offset=-1.5)        # noqa: E731
    ch1 = MZM(LASER(P0=3.0, df=-25e9), drive(1), bias=0.0, Vpi=6.0)
    ch2 = MZM(LASER(P0=0.0, df=25e9), drive(2), bias=0.0, Vpi=6.0)
    print("channels:", ch1, ch2)
    before = dict(_lib.TRANSFERS)
    both = (ch1 + ch2) * 10 ** (6 / 20)          # combine, 6 dB of gain
    both = both - both * 0.01                    # a 1 % tap
    kept = both[: 4000 * gv.sps]                 # keep 4000 bit slots
    head = kept[0, 16:48]                        # the first polarisation's samples 16 ... 47
    envelope = np.abs(kept)                      # |signal + noise|, a field on the GPU
    power = kept.power("dBm")
    after = dict(_lib.TRANSFERS)
    print("transfers before:", before)
    print("transfers after: ", after)
    on_gpu = all(x.on_device for x in (both, kept, head, envelope))
    print(f"transfers during the algebra: h2d +{after['h2d'] - before['h2d']}, d2h +{after['d2h'] - before['d2h']}; results on the GPU: {on_gpu}")
    assert after == before and on_gpu
    print("kept:", kept, "power [dBm]:", power)
    print("photocurrent:", PD(kept, BW=7.5e9, rng="device"))


if __name__ == "__main__":
    main()
