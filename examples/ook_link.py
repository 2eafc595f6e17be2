"""A 10 Gb/s on-off-keyed link on the MI355X path, end to end:

    PRBS -> DAC (Gaussian pulses) -> MZM(LASER) -> FIBER (50 km SMF, adaptive split step) -> PD -> ook.DSP -> BER_analizer

the chain of the reference's own example (opticomlib: examples/ook_transmission_fiber_simulation.py) with every
device taken from opticomlib_amd.  Everything from the modulator to the received bits stays in GPU memory.

    python examples/ook_link.py [bits] [length_km]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import DAC, FIBER, LASER, MZM, PD, PRBS, gv, ook  # noqa: E402

bits = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 12
length = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
Vpi = 5.0
gv(sps=64, R=10e9, N=bits)

def link():
    t0 = time.perf_counter()
    tx = PRBS(order=15, len=bits)
    drive = DAC(tx, Vpp=Vpi, offset=-Vpi / 2, pulse_shape="gaussian")
    field = MZM(LASER(P0=5), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=26)
    t1 = time.perf_counter()
    out = FIBER(field, length=length, alpha=0.2, beta_2=-20, gamma=2)          # adaptive step, phi_max = 0.01
    pd = PD(out, BW=0.75 * gv.R, r=1.0, include_noise="all")
    rx, eye, rth = ook.DSP(pd)                                                  # eye, threshold and decisions on the device
    ber = ook.BER_analizer("counter", Tx=tx, Rx=rx)
    return tx, out, rx, eye, rth, ber, t1 - t0, time.perf_counter() - t1


link()                                  # first call: plans, tables and code objects are created
tx, out, rx, eye, threshold, ber, t_tx, t_rx = link()
errors = int(round(ber * rx.size))
power_dbm = 10 * np.log10(np.mean(np.abs(out.signal) ** 2) / 1e-3)
print(f"{bits} bits, {bits * gv.sps} samples, {length:g} km: transmitter {1e3 * t_tx:.1f} ms, fibre + detector + DSP {1e3 * t_rx:.1f} ms (second call)")
print(f"received power {power_dbm:.2f} dBm, eye: t_opt {eye.t_opt:g}, mu0 {eye.mu0 * 1e3:.3f} mV, mu1 {eye.mu1 * 1e3:.3f} mV, "
      f"threshold {threshold * 1e3:.3f} mV (ook.DSP), {errors} errors in {rx.size} bits (BER_analizer)")
