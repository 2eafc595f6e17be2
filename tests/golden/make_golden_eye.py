#!/usr/bin/env python3
"""Generate the eye / OOK receiver fixtures ``eye_*.npz`` by importing the reference (a development host only).

    python tests/golden/make_golden_eye.py [--reference PATH]

Each case calls the reference's ``GET_EYE`` or ``ook.DSP`` + ``BER_analizer`` with ``np.random.seed(k)`` set just before the call:
sklearn's unseeded KMeans draws from NumPy's global state, so the seed makes the fixtures reproducible.  The input signal is stored
with the outputs (and, for ``DSP(BW=...)``, the reference's filtered signal, so that a CPU check can start after the filter).
Recorded alongside every output: the NumPy / SciPy / sklearn versions.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402

EYE_KEYS = ("t_left", "t_right", "t_opt", "y_left", "y_right", "t_dist", "t_span0", "t_span1", "i", "mu0", "mu1", "s0", "s1", "threshold",
            "er", "eye_h")

# name -> (what, pulse, sps, bits, noise sigma, nslots, sps_resamp, BW / R)
CASES = {
    "eye_nrz_sps16": ("eye", "nrz", 16, 512, 0.05, 4096, None, None),
    "eye_gauss_sps64_r128": ("eye", "gaussian", 64, 256, 0.05, 4096, 128, None),
    "eye_gauss_sps16_r128_odd": ("eye", "gaussian", 16, 300, 0.04, 4096, 128, None),    # 4800 samples: not a power of two
    "eye_nrz_sps64_short": ("eye", "nrz", 64, 100, 0.05, 4096, None, None),            # a word shorter than nslots
    "eye_gauss_sps16_nslots256": ("eye", "gaussian", 16, 1024, 0.06, 256, 128, None),
    "eye_nrz_degenerate": ("eye", "nrz", 16, 256, 0.0, 4096, None, None),              # no noise: the band is empty (fallback branch)
    "eye_dsp_gauss_sps32": ("dsp", "gaussian", 32, 500, 0.08, None, None, None),
    "eye_dsp_nrz_sps32_bw": ("dsp", "nrz", 32, 600, 0.05, None, None, 0.75),
    "eye_dsp_pd_link": ("link", "gaussian", 32, 511, None, None, None, None),            # a PD output (currents ~1e-3 A)
}


def make_input(name, case, devices, typing, k):
    what, pulse, sps, nbits, sigma, *_ = case
    typing.gv(sps=sps, R=1e9 if what != "link" else 10e9, N=nbits)
    tx = devices.PRBS(order=9 if nbits > 127 else 7, len=nbits)
    if what == "link":
        np.random.seed(1000 + k)
        Vpi = 5.0
        drive = devices.DAC(tx, Vpp=Vpi, offset=-Vpi / 2, pulse_shape=pulse)
        field = devices.MZM(devices.LASER(P0=1), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=20)
        out = devices.FIBER(field, length=5, alpha=0.2, beta_2=-20, gamma=2, h=0.5)
        pd = devices.PD(out, BW=0.75 * typing.gv.R, r=1.0, include_noise="all")
        x = np.asarray((pd.signal + pd.noise).real, dtype=np.float64)
    else:
        x = np.asarray(devices.DAC(tx, pulse_shape=pulse, Vpp=1.0).signal, dtype=np.float64)
        if sigma:
            x = x + np.random.default_rng(k).normal(0, sigma, x.size)
    return np.asarray(tx.data, dtype=np.uint8), x


def eye_record(e):
    rec = {}
    for key in EYE_KEYS:
        v = getattr(e, key, None)
        rec[key] = np.array(np.nan if v is None else v, dtype=np.float64)
    rec["top_int"] = np.asarray(e.top_int, dtype=np.float64).ravel()
    rec["bot_int"] = np.asarray(e.bot_int, dtype=np.float64).ravel()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    devices, typing = import_reference(args.reference)
    from opticomlib import ook
    import scipy
    import sklearn
    for k, (name, case) in enumerate(CASES.items()):
        what, pulse, sps, nbits, sigma, nslots, sps_resamp, bw = case
        tx, x = make_input(name, case, devices, typing, k)
        out = {"x": x, "tx": tx, "what": np.array(what), "sps": np.array(sps), "R": np.array(typing.gv.R),
               "nslots": np.array(-1 if nslots is None else nslots), "sps_resamp": np.array(-1 if sps_resamp is None else sps_resamp),
               "BW": np.array(np.nan if bw is None else bw * typing.gv.R),
               "versions": np.array(f"numpy {np.__version__}; scipy {scipy.__version__}; sklearn {sklearn.__version__}")}
        sig = typing.electrical_signal(x)
        np.random.seed(k)
        if what == "eye":
            e = devices.GET_EYE(sig, nslots=nslots, sps_resamp=sps_resamp)
        else:
            if bw is not None:
                out["x_filt"] = np.asarray(devices.LPF(typing.electrical_signal(x), bw * typing.gv.R).signal, dtype=np.float64)
                np.random.seed(k)
            rx, e, rth = ook.DSP(sig, BW=None if bw is None else bw * typing.gv.R)
            out["rx"] = np.asarray(rx.data, dtype=np.uint8)
            out["rth"] = np.array(rth)
            out["ber_counter"] = np.array(ook.BER_analizer("counter", Tx=typing.binary_sequence(tx), Rx=rx))
            out["ber_estimator"] = np.array(ook.BER_analizer("estimator", eye_obj=e))
        out.update(eye_record(e))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, x.size, {key: float(out[key]) for key in ("t_opt", "i", "mu0", "mu1", "threshold")})


if __name__ == "__main__":
    main()
