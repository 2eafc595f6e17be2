"""The data-aided receiver on the MI355X path: a link whose record starts somewhere inside the transmitted word is found, cut and decided
without leaving GPU memory:

    PRBS -> DAC -> MZM(LASER) -> FIBER -> PD, with a known extra delay in front
         -> lab.SYNC -> lab.GET_EYE_v2 -> SAMPLER at eye.i -> ook.BER_analizer('counter')

``_lib.TRANSFERS`` (the host <-> device array copies) is printed before and after the receiver part: it does not move until a result is read.

    python examples/lab_sync.py [delay_samples] [length_km]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import DAC, FIBER, LASER, MZM, PD, PRBS, SAMPLER, _lib, gv, lab, ook  # noqa: E402
from opticomlib_amd.typing import binary_sequence  # noqa: E402

delay = int(sys.argv[1]) if len(sys.argv) > 1 else 1234
length = float(sys.argv[2]) if len(sys.argv) > 2 else 20.0
order, periods, Vpi = 9, 4, 5.0
word_len = 2 ** order - 1
gv(sps=16, R=10e9, N=periods * word_len)

word = PRBS(order=order)                                        # the transmitted word: what the receiver knows
tx = PRBS(order=order, len=periods * word_len)                  # what is sent: the word, over and over
drive = DAC(tx, Vpp=Vpi, offset=-Vpi / 2, pulse_shape="gaussian")
field = MZM(LASER(P0=5), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=26)
out = FIBER(field, length=length, alpha=0.2, beta_2=-20, gamma=2, h=1.0)
pd = PD(out, BW=0.75 * gv.R, r=1.0, include_noise="all")
l = word_len * gv.sps
record = pd[l - delay % l:]                                     # a device-side slice: the record starts `delay` samples before a word

before = dict(_lib.TRANSFERS)
synced, i = lab.SYNC(record, word)
eye = lab.GET_EYE_v2(synced, tx)
samples = SAMPLER(synced, eye.i)
rx = samples > eye.threshold                                    # a device-resident binary_sequence
ber = ook.BER_analizer("counter", Tx=tx, Rx=rx)
after = dict(_lib.TRANSFERS)

print(f"{periods} x PRBS-{order} at {gv.sps} samples per slot, {length:g} km; the record starts {delay % l} samples before a word")
print(f"lab.SYNC: i = {i}; the synchronised record holds {synced.size} samples ({synced.size // gv.sps} slots)")
print(f"lab.GET_EYE_v2: mu0 {eye.mu0 * 1e3:.3f} mV, mu1 {eye.mu1 * 1e3:.3f} mV, s0 {eye.s0 * 1e3:.3f} mV, s1 {eye.s1 * 1e3:.3f} mV, "
      f"threshold {eye.threshold * 1e3:.3f} mV, sampling instant {eye.i}")
print(f"{int(round(ber * rx.size))} errors in {rx.size} bits (ook.BER_analizer)")
print(f"host <-> device array copies before the receiver {before}, after it {after}")
assert isinstance(rx, binary_sequence) and after == before
