#!/usr/bin/env python3
"""Generate the data-aided receiver fixtures ``sync_*.npz`` / ``eyev2_*.npz`` by importing the reference (a development host only).

    python tests/golden/make_golden_sync.py [--reference PATH]

The reference's ``lab.py`` imports the instrument libraries ``pyvisa``, ``h5py`` (and, inside one function, ``serial``) at module level; none
of them is needed by ``SYNC`` and ``GET_EYE_v2``, so empty stand-in modules take their names in ``sys.modules`` before the import.  Each
case stores its inputs with the reference's outputs -- or, where the reference raises, the exception's type and text -- and nothing else.

``lab.py`` also calls ``sps()``, ``dt()`` and ``len()`` on its signal as methods, while the reference's ``electrical_signal`` has ``sps`` and
``dt`` as properties and no ``len``: ``GET_EYE_v2`` (and ``SYNC`` on an ``electrical_signal``) raise ``TypeError`` as they stand.  The eye cases
therefore hand over a subclass of the reference's signal that answers those three calls; ``SYNC`` is called with arrays, the form that works.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402

# name -> (sps, what the record is, delay, noise sigma); PRBS-7 words of 127 slots
SYNC_CASES = {
    "sync_sps8_inside": (8, "periodic", 300, 0.05),
    "sync_sps16_inside": (16, "periodic", 1001, 0.05),
    "sync_sps8_first_lag": (8, "tail", 0, 0.05),              # the word, then a floor: lag 0 is a peak of its own
    "sync_sps16_last_lag": (16, "floor_then_word", None, 0.05),   # i == l: the slice [l:-(0)] is empty
    "sync_sps8_inverted": (8, "inverted", 0, 0.0),            # raises: no correlation maximum
    "sync_sps8_exact_length": (8, "exact", 0, 0.05),          # len(rx) == l: the slice [0:-l] is empty
}
# name -> (pulse, sps, slots, noise sigma (as the signal's noise), nslots)
EYE_CASES = {
    "eyev2_gauss_sps8": ("gaussian", 8, 127, 0.05, 4096),
    "eyev2_gauss_sps16_clean": ("gaussian", 16, 127, 0.0, 4096),
    "eyev2_nrz_sps32_nslots64": ("nrz", 32, 127, 0.04, 64),
}


def import_lab(path):
    devices, typing = import_reference(path)
    for name in ("pyvisa", "h5py", "serial"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from opticomlib import lab
    return devices, typing, lab


def callable_grid(typing):
    """The reference's electrical_signal with ``sps()``, ``dt()`` and ``len()`` as the methods ``lab.py`` calls (slices keep the class)."""
    class signal_with_methods(typing.electrical_signal):
        sps = lambda self: typing.gv.sps                        # noqa: E731
        dt = lambda self: typing.gv.dt                          # noqa: E731
        len = lambda self: self.size                            # noqa: E731
    return signal_with_methods


def record(sps, kind, delay, sigma, word, rng):
    tx = np.kron(word.astype(float), np.ones(sps))
    l = tx.size
    if kind == "periodic":
        rx = np.roll(np.tile(tx, 3), delay)
    elif kind == "tail":
        rx = np.concatenate([tx, np.zeros(l + 5 * sps)])
    elif kind == "floor_then_word":
        rx = np.concatenate([np.zeros(l), tx, np.zeros(3 * sps)])
    elif kind == "inverted":
        rx = -np.tile(tx, 3)
    else:
        rx = tx.copy()
    return rx + (rng.normal(0, sigma, rx.size) if sigma else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    devices, typing, lab = import_lab(args.reference)
    import scipy
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}")
    for k, (name, (sps, kind, delay, sigma)) in enumerate(SYNC_CASES.items()):
        typing.gv(sps=sps, R=1e9)
        word = np.asarray(devices.PRBS(order=7).data, dtype=np.uint8)
        rx = record(sps, kind, delay, sigma, word, np.random.default_rng(100 + k))
        out = {"rx": rx, "tx": word, "sps": np.array(sps), "R": np.array(typing.gv.R), "versions": versions}
        try:
            sig, i = lab.SYNC(rx, word, sps)
            out.update(i=np.array(int(i)), signal=np.asarray(sig.signal, dtype=np.float64), raises=np.array(""), message=np.array(""),
                       noise_is_null=np.array(sig.noise is None or not isinstance(sig.noise, np.ndarray)))
        except Exception as e:                                  # noqa: BLE001 -- the case records whatever the reference raises
            out.update(raises=np.array(type(e).__name__), message=np.array(str(e)))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, rx.size, str(out["raises"]) or int(out["i"]))
    for k, (name, (pulse, sps, nbits, sigma, nslots)) in enumerate(EYE_CASES.items()):
        typing.gv(sps=sps, R=1e9, N=nbits)
        tx = devices.PRBS(order=7, len=nbits)
        x = np.asarray(np.real(devices.DAC(tx, pulse_shape=pulse, Vpp=1.0).signal), dtype=np.float64)
        noise = np.random.default_rng(200 + k).normal(0, sigma, x.size) if sigma else None
        cls = callable_grid(typing)
        sig = cls(x) if noise is None else cls(x, noise)
        e = lab.GET_EYE_v2(sig, tx, nslots=nslots)
        out = {"x": x, "noise": np.zeros(0) if noise is None else noise, "tx": np.asarray(tx.data, dtype=np.uint8), "sps": np.array(sps), "R": np.array(typing.gv.R),
               "nslots": np.array(nslots), "versions": versions}
        for key in ("i", "t_left", "t_right", "t_dist", "t_opt", "t_span0", "t_span1", "mu0", "mu1", "s0", "s1", "threshold", "er", "eye_h"):
            out[key] = np.array(getattr(e, key), dtype=np.float64)
        for key in ("y", "ones", "zeros"):
            out[key] = np.asarray(getattr(e, key), dtype=np.float64)
        out["t0_size"], out["t1_size"] = np.array(np.asarray(e.t0).size), np.array(np.asarray(e.t1).size)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, x.size, {key: float(out[key]) for key in ("mu0", "mu1", "s0", "s1", "threshold")})


if __name__ == "__main__":
    main()
