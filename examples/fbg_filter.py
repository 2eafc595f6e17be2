"""A fibre Bragg grating with the four built-in apodizations, on the MI355X path:

    CW carrier -> FBG(apodization = uniform | rcos | gaussian | parabolic)

The grating (centre at the carrier, v·δneff = 1e-4, kL = 8) is solved on the device for every frequency bin of a 2^14-sample grid at
200 GHz; the script prints the peak reflectivity, the full width at half maximum of |H|² and the RK45 steps of each solve.

    python examples/fbg_filter.py [kL]
"""
import os
import sys
import time

import numpy as np
from scipy.signal import peak_widths

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import FBG, gv, optical_signal  # noqa: E402

kL = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
gv(fs=200e9)
carrier = optical_signal(np.full(1 << 14, 1e-3 ** 0.5, complex))          # 1 mW
df = gv.fs / carrier.size
print(f"grid: {carrier.size} bins of {df / 1e6:.1f} MHz")
for apo in ("uniform", "rcos", "gaussian", "parabolic"):
    t = time.time()
    _, H = FBG(carrier, fc=gv.f0, vdneff=1e-4, kL=kL, apodization=apo, print_params=False, retH=True)
    t = time.time() - t
    R = np.abs(H) ** 2
    top = int(np.argmax(R))
    fwhm = peak_widths(R, [top], rel_height=0.5)[0][0] * df
    print(f"{apo:>9}: peak reflectivity {R[top]:.4f}, FWHM {fwhm / 1e9:6.2f} GHz, {FBG.last_steps} RK45 steps, {t * 1e3:6.1f} ms")
