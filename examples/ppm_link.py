"""A 16-PPM optical link on the MI355X path, end to end:

    PRBS -> ppm.PPM_ENCODER -> DAC (Gaussian pulses) -> MZM(LASER) -> FIBER (20 km SMF, adaptive split step) -> PD -> ppm.DSP -> ppm.BER_analizer

examples/ook_link.py with pulse-position modulation: every device is taken from opticomlib_amd, and everything from the bits to the
received bits stays in GPU memory.  ppm.DSP runs twice, with the soft decision and with the hard one (threshold from the eye).

    python examples/ppm_link.py [bits] [length_km]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import DAC, FIBER, LASER, MZM, PD, PRBS, gv, ppm  # noqa: E402

M = 16
bits = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 12
length = float(sys.argv[2]) if len(sys.argv) > 2 else 20.0
Vpi = 5.0
gv(sps=32, R=10e9, N=bits // 4 * M)


def link():
    t0 = time.perf_counter()
    tx = PRBS(order=15, len=bits)
    slots = ppm.PPM_ENCODER(tx, M)
    drive = DAC(slots, Vpp=Vpi, offset=-Vpi / 2, pulse_shape="gaussian")
    field = MZM(LASER(P0=5), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=26)
    t1 = time.perf_counter()
    out = FIBER(field, length=length, alpha=0.2, beta_2=-20, gamma=2)          # adaptive step, phi_max = 0.01
    pd = PD(out, BW=0.75 * gv.R, r=1.0, include_noise="all")
    soft = ppm.DSP(pd, M, decision="soft")
    hard = ppm.DSP(pd, M, decision="hard")                                     # eye, threshold, decisions and HDD on the device
    ber = [ppm.BER_analizer("counter", Tx=tx, Rx=rx) for rx in (soft, hard)]
    return tx, out, soft, hard, ber, t1 - t0, time.perf_counter() - t1


link()                                  # first call: plans, tables and code objects are created
tx, out, soft, hard, ber, t_tx, t_rx = link()
power_dbm = 10 * np.log10(np.mean(np.abs(out.signal) ** 2) / 1e-3)
e = hard.eye_obj
print(f"{bits} bits, {M}-PPM, {tx.size // 4 * M * gv.sps} samples, {length:g} km: transmitter {1e3 * t_tx:.1f} ms, fibre + detector + DSP {1e3 * t_rx:.1f} ms "
      f"(second call)")
print(f"received power {power_dbm:.2f} dBm, eye: mu0 {e.mu0 * 1e3:.3f} mV, mu1 {e.mu1 * 1e3:.3f} mV, threshold {hard.rth * 1e3:.3f} mV; "
      f"BER soft {ber[0]:.3g} ({round(ber[0] * soft.size)} errors), hard {ber[1]:.3g} ({round(ber[1] * hard.size)} errors) in {soft.size} bits")
