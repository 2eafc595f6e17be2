"""The reference's laser linewidth demo without the GUI, on the MI355X path:

    LASER(P0 = 0 dBm, lw = 20 / 100 MHz, rng = "device") -> get_psd(nperseg = 8192)

gv(sps=32, R=1 GHz, N=100000): 3.2 M samples at 32 GS/s.  The phase noise is drawn and summed on the device and the Welch estimate reads the
field where it lies; only the 8192-bin spectrum comes back.  The -3 dB (full) width of a Wiener-phase laser's Lorentzian line is its
linewidth: the script prints it next to `lw`, with the frequency resolution fs / nperseg.

    python examples/laser_psd.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import LASER, get_psd, gv  # noqa: E402

gv(sps=32, R=1e9, N=100000)
nperseg = 4 * 2048
print(f"{gv.t.size} samples at {gv.fs * 1e-9:.0f} GS/s, nperseg = {nperseg}, resolution {gv.fs / nperseg * 1e-6:.2f} MHz")
for lw in (20e6, 100e6):
    laser = LASER(P0=0, lw=lw, rng="device")
    get_psd(laser, fs=gv.fs, nperseg=nperseg)                           # first call: code objects and tables
    t = time.perf_counter()
    f, psd = get_psd(laser, fs=gv.fs, nperseg=nperseg)
    t = time.perf_counter() - t
    above = f[psd >= psd.max() / 2]
    width = above.max() - above.min() + gv.fs / nperseg
    print(f"lw = {lw * 1e-6:6.1f} MHz   -3 dB width = {width * 1e-6:6.1f} MHz   peak {10 * np.log10(psd.max()) + 30:6.2f} dBm   "
          f"get_psd {t * 1e3:.2f} ms   field on the device: {laser.on_device}")
