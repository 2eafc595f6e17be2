#!/usr/bin/env python3
"""A polarisation-multiplexed 16-QAM link from bits to bits, in GPU memory all the way:

    PRBS -> QAM_ENCODER -> SHAPE -> x LASER(lw) -> FIBER(coupling="manakov") -> [DBP] -> coherent.DSP(ref=...) -> BER, EVM

Prints the counts of host <-> device copies before and after the chain (none is made until a result is read), and the bit error rate and the error
vector magnitude of both polarisations with and without digital back-propagation.  An illustration: no value is claimed.

    python examples/coherent_link.py [symbols] [launch power, dBm]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticomlib_amd import DBP, FIBER, LASER, PRBS, _lib, coherent, device_rng_seed, gv, optical_signal, workloads  # noqa: E402
from opticomlib_amd.devices import _stack_rows  # noqa: E402

M = 16


def main():
    nsym = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    dbm = float(sys.argv[2]) if len(sys.argv) > 2 else 9.0
    gv(sps=16, R=32e9, N=nsym)
    device_rng_seed(1)
    print("transfers before:", dict(_lib.TRANSFERS))
    bits = [PRBS(15, len=4 * nsym, seed=7 + p) for p in range(2)]
    symbols = [coherent.QAM_ENCODER(b, M) for b in bits]
    rows = [(LASER(dbm, lw=100e3, rng="device") * coherent.SHAPE(s, "rcos", beta=0.2))._raw("signal") for s in symbols]
    tx = optical_signal.from_device(_stack_rows(rows, np.complex128, rows[0].device, (2, nsym * gv.sps)))
    fibre = dict(length=80.0, h=0.5, coupling="manakov", **workloads.SMF)
    after = FIBER(tx, **fibre)
    # without back-propagation the dispersion alone closes the constellation: the comparison is between a linear and a nonlinear equaliser
    linear = DBP(after, **{**fibre, "gamma": 0.0})
    full = DBP(after, **fibre)
    results = {"dispersion compensated": coherent.DSP(linear, M, ref=symbols), "back-propagated": coherent.DSP(full, M, ref=symbols)}
    print("transfers after: ", dict(_lib.TRANSFERS))
    for name, rx in results.items():
        for p in range(2):
            print(f"{name:>24}, polarisation {p}: BER {coherent.BER(bits[p], rx.bits[p]):.2e}  EVM {100 * rx.evm[p]:5.2f} %  quarter turns {rx.quarter_turns[p]}")


if __name__ == "__main__":
    main()
