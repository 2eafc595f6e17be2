#!/usr/bin/env python3
"""``GET_EYE(...).plot()`` of a link whose record never leaves the GPU:

    PRBS -> DAC (Gaussian pulses) -> MZM(LASER) -> FIBER (20 km) -> PD -> GET_EYE -> .plot(EyeShowOptions(all_none=True))

The eye's record ``y`` stays in GPU memory: the 350 x 350 density, its blur and the side panel are computed there by the fold entry points of
csrc/eye_density.hip.  ``_lib.TRANSFERS`` counts the array copies between host and device: the plot adds two downloads (the counts and the blurred
grid) and no upload.

    python examples/eye_plot.py [eye.png]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import matplotlib

matplotlib.use("Agg")

from opticomlib_amd import DAC, FIBER, GET_EYE, LASER, MZM, PD, PRBS, EyeShowOptions, _lib, gv  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "eye_plot.png"
    Vpi = 5.0
    gv(sps=32, R=10e9, N=1 << 12)
    tx = PRBS(order=15, len=1 << 12)
    drive = DAC(tx, Vpp=Vpi, offset=-Vpi / 2, pulse_shape="gaussian")
    field = MZM(LASER(P0=5), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=26)
    pd = PD(FIBER(field, length=20, alpha=0.2, beta_2=-20, gamma=2, h=1.0), BW=0.75 * gv.R, r=1.0, include_noise="all")
    e = GET_EYE(pd, nslots=4096)
    before = dict(_lib.TRANSFERS)
    print("transfers before the plot:", before)
    e.plot(EyeShowOptions(all_none=True), savefig=out)
    after = dict(_lib.TRANSFERS)
    print("transfers after the plot: ", after, "| the record is still on the device:", isinstance(e.__dict__["_y"], _lib.DeviceArray))
    assert after["h2d"] == before["h2d"]
    print("wrote", out)


if __name__ == "__main__":
    main()
