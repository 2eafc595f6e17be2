#!/usr/bin/env python3
"""The eye diagram of a record that never leaves the GPU: PRBS -> DAC -> LPF on the device, then ``plot_eye(style='density')``, whose density grid
is computed by the kernels of csrc/eye_density.hip where the record lies.  ``_lib.TRANSFERS`` counts the array copies between host and device:
the plot adds two downloads (the 200 x 200 counts and the blurred grid) and no upload.

    python examples/eye_diagram.py [eye.png]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

from opticomlib_amd import DAC, LPF, PRBS, _lib, gv  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "eye_diagram.png"
    gv(sps=16, R=10e9)
    bits = PRBS(order=15, len=1 << 14)
    x = LPF(DAC(bits, Vpp=1.0), BW=7e9)
    print("on the device:", x.on_device, "| samples:", x.size, "| transfers before the plot:", dict(_lib.TRANSFERS))
    fig, ax = plt.subplots(figsize=(8, 5))
    x.plot_eye(style="density", ax=ax, show=False)
    print("transfers after the plot: ", dict(_lib.TRANSFERS), "| still on the device:", x.on_device)
    fig.savefig(out, dpi=120)
    print("wrote", out)


if __name__ == "__main__":
    main()
