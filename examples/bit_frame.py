"""A frame assembled where its bits lie: a preamble and a repeated word from two ``PRBS`` calls become ``frame = pre + word * k`` on the GPU,
a shifted copy of it is sent, and the receiver aligns, samples and decides it without leaving GPU memory:

    frame = pre + word * k;  sent = (frame * 3)[shift:]
    DAC(sent) -> lab.SYNC(., frame) -> SAMPLER -> > thr -> [:len(frame)].hamming_distance(frame)

``_lib.TRANSFERS`` (the host <-> device array copies) is printed before and after: nothing is copied, the counts and the distance come back as
single integers.

    python examples/bit_frame.py [shift_slots] [k]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticomlib_amd import DAC, PRBS, SAMPLER, _lib, gv, lab  # noqa: E402
from opticomlib_amd.typing import binary_sequence  # noqa: E402

shift = int(sys.argv[1]) if len(sys.argv) > 1 else 200
k = int(sys.argv[2]) if len(sys.argv) > 2 else 6
pre, word = PRBS(order=7), PRBS(order=9, seed=0x155)            # 127 and 511 bits, device-resident
gv(sps=16, R=10e9)

before = dict(_lib.TRANSFERS)
frame = pre + word * k                                          # what the receiver knows
sent = (frame * 3)[shift:]                                      # three frames on the line; the record starts `shift` slots into the first
signal = DAC(sent, pulse_shape="gaussian")
synced, i = lab.SYNC(signal, frame)
samples = SAMPLER(synced, gv.sps // 2)
rx = samples > 0.5                                              # a device-resident binary_sequence
ones, errors = frame.ones, rx[:frame.size].hamming_distance(frame)
after = dict(_lib.TRANSFERS)

print(f"frame = PRBS-7 + PRBS-9 x {k}: {frame.size} bits, {ones} ones; sent from slot {shift} on at {gv.sps} samples per slot")
print(f"lab.SYNC: i = {i} samples ({i / gv.sps:g} slots); {rx.size} bits decided, hamming distance to the frame {errors}")
print(f"host <-> device array copies before {before}, after {after}")
assert all(isinstance(x, binary_sequence) and x.on_device for x in (frame, sent, rx)) and after == before
assert errors == 0 and i == (frame.size - shift % frame.size) % frame.size * gv.sps
