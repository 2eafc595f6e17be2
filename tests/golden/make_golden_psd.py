#!/usr/bin/env python3
"""Generate the PSD fixtures ``psd_*.npz`` by importing the reference and calling its ``opticomlib.utils.get_psd`` (a development host only).

    python tests/golden/make_golden_psd.py [--reference ../reference]

Every file holds the input (``x``; or ``phase``, float32, for the 2^16-sample complex128 field, built as ``exp(1j * phase)`` in float64 on
both sides, which keeps the file under 512 KiB), ``fs``, ``nperseg`` (-1: the default), the reference's ``f`` and ``psd``, and the text of the
warning it raised ("" for none).
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402


def field_from_phase(phase):
    return np.exp(1j * np.asarray(phase, dtype=np.float64))


def cases():
    rng = np.random.default_rng(2048)
    fs = 10e9
    t = np.arange(0, 1000e-9, 1 / fs)
    yield "psd_sine_1ghz", {"x": np.sin(2 * np.pi * 1e9 * t)}, fs, None             # the reference test (utils_test.py:12)
    yield "psd_real_f32", {"x": rng.standard_normal(6000).astype(np.float32) + np.float32(0.3)}, 1.0, 512
    # a laser field with 1 MHz linewidth at 64 GS/s: a Wiener phase (LASER's model), nperseg of the reference's linewidth demo
    fs_l, lw = 64e9, 1e6
    phase = np.cumsum(rng.normal(0, np.sqrt(2 * np.pi * lw / fs_l), 1 << 16)).astype(np.float32)
    yield "psd_phase_noise_c128", {"phase": phase}, fs_l * 1e-9, 8192
    dual = ((rng.standard_normal((2, 8192)) + 1j * rng.standard_normal((2, 8192))) * 0.1).astype(np.complex64)
    yield "psd_dualpol_c64_default", {"x": dual}, 128.0, None                        # len(sig) = 2: nperseg = 2, psd of shape (2, 2)
    yield "psd_dualpol_c64_1024", {"x": dual}, 128.0, 1024
    yield "psd_real_nperseg3000", {"x": np.cos(np.arange(12000) * 0.37) + 0.1 * rng.standard_normal(12000)}, 1.0, 3000
    yield "psd_c128_nperseg17", {"x": rng.standard_normal(4000) + 1j * rng.standard_normal(4000)}, 1.0, 17
    yield "psd_short_input", {"x": rng.standard_normal(1000)}, 1.0, 2048              # nperseg > 1000 samples: SciPy's warning


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    import_reference(args.reference)
    import scipy
    from opticomlib.utils import get_psd
    for name, inp, fs, nperseg in cases():
        x = field_from_phase(inp["phase"]) if "phase" in inp else inp["x"]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            f, psd = get_psd(x, fs, nperseg)
        msgs = [str(m.message) for m in w if issubclass(m.category, UserWarning)]
        out = dict(inp)
        out.update({"fs": np.array(fs), "nperseg": np.array(-1 if nperseg is None else nperseg), "f": f, "psd": psd,
                    "warning": np.array(msgs[0] if msgs else ""), "versions": np.array(f"numpy {np.__version__}; scipy {scipy.__version__}")})
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, x.shape, x.dtype, psd.shape, psd.dtype, os.path.getsize(path), repr(msgs[0]) if msgs else "")


if __name__ == "__main__":
    main()
