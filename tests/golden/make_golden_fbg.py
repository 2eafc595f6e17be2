#!/usr/bin/env python3
"""Generate the FBG / PM / ADC fixtures ``fbg_*.npz``, ``pm_*.npz`` and ``adc_*.npz`` by importing the reference (a development host only).

    python tests/golden/make_golden_fbg.py [--reference PATH]

FBG fixtures hold the inputs, the keyword arguments (JSON), H (after the filtfilt correction, as ``retH`` returns it), the filtered signal and
noise, the printed parameter block, and the step counts of the reference's ``solve_ivp`` (``len(sol.t) - 1`` and ``nfev``; the attempted
steps are ``(nfev - 2) / 6``).  Every file also stores the NumPy / SciPy versions.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402

# (name, fs, n, kwargs, with noise)
FBG_CASES = (
    ("fbg_uniform_kl2", 100e9, 2048, dict(fc="f0", vdneff=1e-4, kL=2), True),
    ("fbg_uniform_kl16", 100e9, 4096, dict(fc="f0", vdneff=1e-4, kL=16), False),
    ("fbg_rcos", 100e9, 2048, dict(fc="f0", vdneff=1e-4, kL=8, apodization="rcos"), True),
    ("fbg_gaussian", 100e9, 2048, dict(fc="f0", vdneff=1e-4, kL=8, apodization="gaussian"), False),
    ("fbg_parabolic", 100e9, 2048, dict(fc="f0", vdneff=1e-4, kL=8, apodization="parabolic"), False),
    ("fbg_chirped_rcos", 400e9, 4096, dict(fc="f0", vdneff=1e-4, kL=16, F=20, apodization="rcos"), True),
    ("fbg_fc_dneff_n", 200e9, 2048, dict(fc="f0", dneff=1e-4, v=0.8, N=20000), False),
    ("fbg_landa_kl_n", 100e9, 2048, dict(landa_D=1550.2e-9, kL=3, N=30000), False),
    ("fbg_landa_vdneff_l", 100e9, 2048, dict(landa_D=1550e-9, vdneff=5e-5, L=0.02), False),
    ("fbg_nofiltfilt", 100e9, 2048, dict(fc="f0", vdneff=1e-4, kL=4, filtfilt=False), True),
    ("fbg_npow2_3000", 100e9, 3000, dict(fc="f0", vdneff=1e-4, kL=4, apodization="gaussian"), True),
)


class Counter:
    def __init__(self, solve_ivp):
        self.solve_ivp, self.last = solve_ivp, None

    def __call__(self, *a, **k):
        sol = self.solve_ivp(*a, **k)
        self.last = (len(sol.t) - 1, sol.nfev)
        return sol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    devices, typing = import_reference(args.reference)
    import scipy
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}")
    save = lambda name, **kw: np.savez_compressed(os.path.join(HERE, name + ".npz"), versions=versions, **kw)
    counter = Counter(devices.solve_ivp)
    devices.solve_ivp = counter
    rng = np.random.default_rng(1894)

    for name, fs, n, kw, noisy in FBG_CASES:
        typing.gv(fs=fs)
        sig = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.1
        noi = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.01 if noisy else None
        x = typing.optical_signal(sig, noi) if noisy else typing.optical_signal(sig)
        call = {k: (typing.gv.f0 if v == "f0" else v) for k, v in kw.items()}
        text = io.StringIO()
        with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(text):
            warnings.simplefilter("always")
            out, H = devices.FBG(x, print_params=True, retH=True, **call)
        steps, nfev = counter.last
        save(name, fs=fs, kwargs=json.dumps(call), signal=sig, noise=noi if noisy else np.zeros(0), H=H,
             out_signal=np.asarray(out.signal), out_noise=np.asarray(out.noise) if noisy else np.zeros(0), steps=steps, nfev=nfev,
             printed=np.array(text.getvalue()), warned=np.array([str(w.message) for w in caught]))
        print(f"{name}: n={n} steps={steps} attempts={(nfev - 2) // 6} max|H|={np.abs(H).max():.3f}")

    # PM: array drive with its own noise (the optical signal with noise), a scalar drive, a dual-polarisation input
    typing.gv(sps=16, R=10e9)
    n = 4096
    sig = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.1
    noi = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.01
    v = rng.uniform(-3, 3, n)
    vn = rng.normal(0, 0.05, n)
    out = devices.PM(typing.optical_signal(sig, noi), typing.electrical_signal(v, vn), Vpi=3.3)
    out_s = devices.PM(typing.optical_signal(sig), 2.5, Vpi=5)
    sig2 = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.1
    out2 = devices.PM(typing.optical_signal(sig2), v, Vpi=4.0)
    save("pm_cases", signal=sig, noise=noi, v=v, vn=vn, out_signal=np.asarray(out.signal), out_noise=np.asarray(out.noise),
         out_scalar=np.asarray(out_s.signal), signal2=sig2, out2=np.asarray(out2.signal))

    # ADC: a 4-level signal with a noise array (which the reference does not quantise), n = 2, 4, 8, at the grid rate and resampled
    typing.gv(sps=16, R=10e9)
    n = 4096
    levels = rng.integers(0, 4, n // 16).repeat(16).astype(float)
    x = levels + rng.normal(0, 0.1, n)
    xn = rng.normal(0, 0.02, n)
    res = {}
    for bits in (2, 4, 8):
        for tag, fs in (("nofs", None), ("fs", typing.gv.fs / 2)):
            for otype in ("n", "v"):
                o = devices.ADC(typing.electrical_signal(x, xn), fs=fs, n=bits, otype=otype)
                res[f"n{bits}_{tag}_{otype}"] = np.asarray(o.signal)
    save("adc_cases", signal=x, noise=xn, fs=typing.gv.fs, **res)


if __name__ == "__main__":
    main()
