"""On-off keying receiver, reference ``opticomlib/ook.py``: ``THRESHOLD_EST``, ``DSP`` and ``BER_analizer``.

``DSP`` runs on the GPU end to end (optional ``LPF``, ``GET_EYE``, the decision at ``gv.sps // 2``) and returns its bits in GPU
memory; ``BER_analizer('counter')`` compares two device-resident sequences there.  ``THRESHOLD_EST`` and the estimator are a few
host scalars, as in the reference, and so is ``theory_BER``.
"""
from __future__ import annotations

import time
from typing import Literal

import numpy as np
from scipy.special import erfc

from . import _lib
from .devices import GET_EYE, LPF, _adopt, _dev_array, _real_sum_device, _sample_device, default_device
from .typing import NULL, binary_sequence, electrical_signal

__all__ = ["THRESHOLD_EST", "DSP", "BER_analizer", "theory_BER"]


def _Q(x):
    return 0.5 * erfc(x / np.sqrt(2))


def THRESHOLD_EST(eye_obj) -> float:
    """Decision threshold minimising ``Q((mu1 - r) / s1) / 2 + Q((r - mu0) / s0) / 2`` over ``linspace(mu0, mu1, 1000)``
    (reference ``ook.py:22-61``)."""
    mu0, mu1, s0, s1 = eye_obj.mu0, eye_obj.mu1, eye_obj.s0, eye_obj.s1
    r = np.linspace(mu0, mu1, 1000)
    return r[np.argmin(0.5 * (_Q((mu1 - r) / s1) + _Q((r - mu0) / s0)))]


def DSP(input, BW: float = None, *, device=None):
    """OOK decisions (reference ``ook.py:63-133``): ``LPF`` when ``BW`` is given, ``GET_EYE(nslots=8192, sps_resamp=128)``, the threshold
    of :func:`THRESHOLD_EST`, then ``x[gv.sps // 2 :: gv.sps] > rth``.  Returns ``(bits, eye, rth)``; the bits stay in GPU memory."""
    t0 = time.time()
    input, grid, _ = _adopt(input, "electrical_signal")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    x = LPF(input, BW, device=device) if BW is not None else input
    eye_obj = GET_EYE(x, nslots=8192, sps_resamp=128, device=device, _grid=grid)
    rth = THRESHOLD_EST(eye_obj)
    dev = default_device() if device is None else int(device)
    sps = int(grid.sps)
    sig, noi = x._raw("signal"), x._raw("noise")
    real = lambda a: not np.iscomplexobj(np.empty(0, a.dtype))
    if real(sig) and (noi is NULL or real(noi)):             # signal + noise > rth, read where they lie (the reference's `x > rth`)
        bits = _sample_device(sig, sps // 2, sps, dev, thr=rth, noise=None if noi is NULL else noi)
    else:                                                   # complex: Re(signal + noise) first
        bits = _sample_device(_real_sum_device(x, x.size, 0, dev), sps // 2, sps, dev, thr=rth)
    output = binary_sequence.from_device(bits) if isinstance(bits, _lib.DeviceArray) else binary_sequence(bits)
    output.execution_time = time.time() - t0
    return output, eye_obj, rth


def _bits_device(seq, dev: int) -> "_lib.DeviceArray":
    raw = seq._raw() if isinstance(seq, binary_sequence) else getattr(seq, "data", seq)
    if isinstance(raw, _lib.DeviceArray):
        return _dev_array(raw, np.uint8, dev) if raw.device != dev else raw
    a = np.asarray(raw)
    if isinstance(raw, str) or a.dtype.kind in "US":
        a = np.asarray(binary_sequence(raw).data)
    return _lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.uint8).ravel(), np.uint8, dev)


def BER_analizer(mode: Literal["counter", "estimator"], *, device=None, **kargs):
    """Bit error rate (reference ``ook.py:135-220``): ``'counter'`` compares ``Rx`` with ``Tx[:Rx.size]`` on the GPU;
    ``'estimator'`` evaluates the Q-function expression at the threshold of :func:`THRESHOLD_EST` from ``eye_obj``."""
    if mode == "counter":
        assert "Rx" in kargs.keys() and "Tx" in kargs.keys(), "`Tx` and `Rx` are required arguments for `mode='counter'`."
        dev = default_device() if device is None else int(device)
        rx, tx = _bits_device(kargs["Rx"], dev), _bits_device(kargs["Tx"], dev)
        n = rx.size
        assert tx.size >= n, "Error: `Tx` and `Rx` must have the same length."
        errs = _lib._I64(0)
        _lib.api.ssfm_device_count_diff(dev, tx, rx, n, _lib.C.byref(errs))
        return errs.value / n
    elif mode == "estimator":
        assert "eye_obj" in kargs.keys(), "`eye_obj` is a required argument for `mode='estimator'`."
        e = kargs["eye_obj"]
        um = THRESHOLD_EST(e)
        return 0.5 * (_Q((e.mu1 - um) / e.s1) + _Q((um - e.mu0) / e.s0))
    else:
        raise TypeError("Invalid mode. Use `counter` or `estimator`.")


def theory_BER(mu1, s0, s1):
    """Theoretical bit error probability of OOK (reference ``ook.py:222-256``): ``0.5 min(Q((mu1 - r)/s1) + Q(r/s0))`` over
    ``linspace(0, mu1, 1000)``, vectorised over ``mu1``, ``s0`` and ``s1`` as the reference does."""
    @np.vectorize
    def fun(mu1_, s0_, s1_):
        r = np.linspace(0, mu1_, 1000)
        return 0.5 * np.min(_Q((mu1_ - r) / s1_) + _Q(r / s0_))

    return fun(mu1, s0, s1)
