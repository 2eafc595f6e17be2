#!/usr/bin/env python3
"""Generate the PPM receiver fixtures ``ppm_*.npz`` by importing the reference (a development host only).

    python tests/golden/make_golden_ppm.py [--reference PATH]

Each case sets ``np.random.seed(k)`` just before the reference call: HDD draws from NumPy's global generator, and so does sklearn's KMeans
inside GET_EYE.  The inputs are stored with the outputs, and with them the NumPy / SciPy / sklearn versions.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402

CODEC_M = (2, 4, 16, 64, 256)
HDD_CASES = ((4, 4000, 0.3), (16, 1500, 0.08), (64, 300, 0.02), (256, 80, 0.005), (2, 4000, 0.5))      # (M, symbols, P(slot ON))
SDD_CASES = ((4, 8, 0.35), (16, 4, 0.3), (64, 4, 0.25))                                                   # (M, sps, noise sigma)
SLOTS = 4096                                                                                             # slots of a signal case


def ppm_signal(devices, typing, ppm, rng, M, nsym, sps, sigma):
    typing.gv(sps=sps, R=1e9)
    bits = rng.integers(0, 2, nsym * int(np.log2(M))).astype(np.uint8)
    x = devices.DAC(ppm.PPM_ENCODER(bits, M), pulse_shape="gaussian")
    # float32 values (stored as float64): the fixtures stay small, and the inputs are exact in either precision
    sig = np.real(np.asarray(x.signal)).astype(np.float32).astype(np.float64)
    noise = rng.normal(0, sigma, sig.size).astype(np.float32).astype(np.float64)
    return bits, sig, noise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    devices, typing = import_reference(args.reference)
    from opticomlib import ppm, ook
    import scipy
    import sklearn
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}; sklearn {sklearn.__version__}")
    save = lambda name, **kw: np.savez_compressed(os.path.join(HERE, name + ".npz"), versions=versions, **kw)
    rng = np.random.default_rng(2024)
    k = 0

    # encoder / decoder; the decoder input has empty and double symbols
    out = {}
    for M in CODEC_M:
        kb = int(np.log2(M))
        bits = rng.integers(0, 2, 257 * kb + kb - 1).astype(np.uint8)           # not a multiple of k: the encoder truncates
        enc = np.asarray(ppm.PPM_ENCODER(bits, M).data, dtype=np.uint8)
        dec_in = enc.reshape(-1, M).copy()
        dec_in[rng.random(dec_in.shape[0]) < 0.1] = 0
        dbl = np.nonzero(rng.random(dec_in.shape[0]) < 0.1)[0]
        dec_in[dbl, rng.integers(0, M, dbl.size)] = 1
        dec_in = dec_in.ravel()
        out.update({f"bits_{M}": bits, f"enc_{M}": enc, f"dec_in_{M}": dec_in,
                    f"dec_out_{M}": np.asarray(ppm.PPM_DECODER(dec_in, M).data, dtype=np.uint8)})
    save("ppm_codec", **out)

    # HDD
    out = {}
    for M, nsym, p in HDD_CASES:
        k += 1
        inp = (rng.random(nsym * M) < p).astype(np.uint8)
        np.random.seed(k)
        res = np.asarray(ppm.HDD(inp.copy(), M).data, dtype=np.uint8)
        out.update({f"in_{M}": inp, f"out_{M}": res, f"seed_{M}": np.array(k)})
    save("ppm_hdd", **out)

    # SDD on noisy Gaussian pulses, and a hand case with ties and NaN
    out = {}
    for M, sps, sigma in SDD_CASES:
        bits, sig, noise = ppm_signal(devices, typing, ppm, rng, M, SLOTS // M, sps, sigma)
        out.update({f"sig_{M}": sig, f"noise_{M}": noise, f"sps_{M}": np.array(sps),
                    f"out_{M}": np.asarray(ppm.SDD(typing.electrical_signal(sig, noise), M).data, dtype=np.uint8)})
    typing.gv(sps=4, R=1e9)
    ties = np.kron([0.5, 1.0, 1.0, 0.2, np.nan, 1.0, np.nan, 3.0, -0.0, 0.0, -1.0, -2.0, 2.0, 2.0, 2.0, 2.0], np.ones(4))
    out.update({"ties_x": ties, "ties_out": np.asarray(ppm.SDD(ties, 4).data, dtype=np.uint8)})
    save("ppm_sdd", **out)

    # DSP: soft, hard with a given threshold, hard with an estimated one
    for name, M, sps, sigma, decision, thr in (("ppm_dsp_soft", 16, 8, 0.3, "soft", None), ("ppm_dsp_hard_thr", 4, 8, 0.25, "hard", 0.55),
                                               ("ppm_dsp_hard_thr_m64", 64, 8, 0.2, "hard", 0.6), ("ppm_dsp_hard_est", 8, 16, 0.17, "hard", None)):
        k += 1
        nsym = SLOTS // M
        # the estimated-threshold case has an input of its own: an eye whose two-means the reference's KMeans reaches
        bits, sig, noise = ppm_signal(devices, typing, ppm, rng if thr is not None or decision == "soft" else np.random.default_rng(5), M, nsym, sps, sigma)
        x = typing.electrical_signal(sig, noise)
        rec = {"bits": bits, "sig": sig, "noise": noise, "M": np.array(M), "sps": np.array(sps), "seed": np.array(k)}
        np.random.seed(k)
        rec["rx"] = np.asarray(ppm.DSP(x, M, decision=decision, threshold=thr).data, dtype=np.uint8)
        if thr is not None:
            rec["rth"] = np.array(thr)
        elif decision == "hard":
            np.random.seed(k)
            e = devices.GET_EYE(x, nslots=8192)
            rth = e.threshold if e.threshold is not None else ppm.THRESHOLD_EST(e, M)
            rec.update({"rth": np.array(rth), "mu0": np.array(e.mu0), "mu1": np.array(e.mu1), "s0": np.array(e.s0), "s1": np.array(e.s1),
                        "threshold": np.array(np.nan if e.threshold is None else e.threshold),
                        "decisions": np.asarray((sig + noise)[sps // 2:: sps] > rth, dtype=np.uint8)})
        save(name, **rec)
        print(name, "bit errors", int(np.sum(rec["rx"][: bits.size] != bits[: rec["rx"].size])), "of", bits.size)

    # estimator and theory
    eyes = np.array([[0.0, 1.0, 0.1, 0.1], [0.1, 0.9, 0.12, 0.15], [0.05, 1.2, 0.2, 0.25], [0.2, 0.8, 0.1, 0.08]])
    Ms = np.array([2, 4, 8, 16, 64, 256])
    est = np.zeros((2, eyes.shape[0], Ms.size))
    for a, decision in enumerate(("hard", "soft")):
        for i, (mu0, mu1, s0, s1) in enumerate(eyes):
            for j, M in enumerate(Ms):
                est[a, i, j] = ppm.BER_analizer("estimator", eye_obj=typing.eye(mu0=mu0, mu1=mu1, s0=s0, s1=s1), M=int(M), decision=decision)
    mu1 = np.array([0.5, 1.0, 1.5, 2.0])
    s = np.array([0.1, 0.12, 0.2, 0.3])
    theory = np.array([[ppm.theory_BER(mu1, s, 1.3 * s, int(M), d) for M in Ms] for d in ("hard", "soft")])
    save("ppm_ber", eyes=eyes, Ms=Ms, estimator=est, mu1=mu1, s=s, theory=theory, theory_ook=ook.theory_BER(mu1, s, 1.3 * s))


if __name__ == "__main__":
    main()
