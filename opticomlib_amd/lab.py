"""The data-aided receiver, reference ``opticomlib/lab.py``: ``SYNC`` and ``GET_EYE_v2``.

``SYNC`` finds where the transmitted slot sequence starts inside a received record (one FFT correlation on a power-of-two complex128
plan, its peak statistics reduced on the GPU) and cuts the record there; ``GET_EYE_v2`` estimates the eye's levels from the slots known
to have been sent.  Both run on the GPU end to end (csrc/sync.hip) and leave their results in GPU memory: a device-resident record and
device-resident bits (what ``PD``, ``LPF``, ``ADC``, ``DAC`` and ``PRBS`` return) are used where they lie, host inputs are uploaded once.
There is no CPU fallback: a case the device path does not take raises.

The instrument drivers, ``save_h5`` and ``load_h5`` of the reference's module are not part of this one; it imports no instrument library.
"""
from __future__ import annotations

import operator
import time

import numpy as np

from . import _lib
from .devices import _adopt, _dev_array, _on_device, _real_sum_device, _wrap_out, default_device, get_plan
from .devices import _S as _EYE_STATE
from .typing import NULL, binary_sequence, electrical_signal, eye

__all__ = ["SYNC", "GET_EYE_v2"]

_EYE_MAX_N = 1 << 21


def _slots(slots_tx, strict: bool):
    """The slots as ``(host uint8 array or uint8 DeviceArray, count)``.  ``strict`` (SYNC): only a ``binary_sequence`` or an ``ndarray``."""
    if isinstance(slots_tx, binary_sequence):
        raw = slots_tx._raw()
        if _on_device(raw):
            return raw, int(raw.size)
    elif type(slots_tx).__name__ == "binary_sequence" and hasattr(slots_tx, "data"):          # the caller's library's own class
        raw = np.asarray(slots_tx.data)
    elif strict and not isinstance(slots_tx, np.ndarray):
        raise TypeError('The "slots_tx" must be of type `binary_sequence` or `np.ndarray`.')
    else:
        raw = binary_sequence(slots_tx).data if not isinstance(slots_tx, np.ndarray) else slots_tx
    raw = np.asarray(raw)
    if raw.ndim != 1:
        raise ValueError(f"Binary sequence must be 1D, invalid shape {raw.shape}")
    if not np.all((raw == 0) | (raw == 1)):
        raise ValueError("Binary sequence must contain only 0 and 1 values.")
    return raw.astype(np.uint8), int(raw.size)


def _bits_on(dev: int, bits):
    if _on_device(bits):
        return _dev_array(bits, np.uint8, dev)
    return _lib.DeviceArray.from_host(np.ascontiguousarray(bits, dtype=np.uint8), np.uint8, dev)


def _correlate(plan, x, b, sps: int, W: int):
    """The plan's field <- ``corr[k] = sum_m x[k + m] tx[m]`` at index k (real parts), for the first ``W`` samples of the float64 device array
    ``x`` and the device-resident slots ``b`` held ``sps`` samples each; the lags ``k <= W - len(b) sps`` do not wrap.  Complete on return."""
    plan.load_template(b, sps)                                  # field <- the held slots, time-reversed modulo the plan length
    plan.table_from_field(0)                                    # slot 0 <- conj(fft(tx))
    plan.load_padded(x, W)                                      # field <- the first W samples of the record
    plan.apply_table(0)                                         # field[k] <- corr[k]
    plan.synchronize()


def SYNC(signal_rx, slots_tx, sps: int = None, *, device=None):
    """Signal synchroniser, reference ``lab.py:92-155``: the position ``i`` of the largest correlation between the record and the transmitted
    slots (held ``sps`` samples each, ``l`` samples in all) within a window of ``2 l`` samples, and the record cut there,
    ``signal_rx[i : -(l - i)]``.  Returns ``(electrical_signal, i)``; the signal carries no noise, as in the reference.

    ``signal_rx``: an ``electrical_signal`` (``sps`` is then the grid's) or an ``ndarray`` (``sps`` is required, else ``ValueError``); anything
    else is a ``TypeError``, as is a ``slots_tx`` that is neither a ``binary_sequence`` nor an ``ndarray``.  A record shorter than the
    transmitted sequence raises ``BufferError``; a largest correlation below three standard deviations of the correlation raises
    ``ValueError('No correlation maximum found!!')``.  The slice keeps Python's reading of ``-(l - i)``: ``i == l`` and a record of exactly
    ``l`` samples select nothing, and an empty ``electrical_signal`` is the constructor's ``ValueError``, here as in the reference.

    Only real records are correlated on the device: a complex ``signal_rx`` raises ``TypeError``.  Slot values other than 0 and 1 raise
    ``ValueError``; a window beyond the largest direct complex128 plan raises ``ValueError``.

    On the GPU: the template is generated from the uint8 slots, time-reversed, in the field of a plan of ``M = max(256, next_pow2(W))`` points
    (``W = min(len, 2 l)``), turned into its transfer table, applied to the first ``W`` samples of the record, and one reduction leaves the
    maximum, its first index, the mean and the two-pass population standard deviation of the ``W - l + 1`` lags for the host to read: eight
    launches and one blocking read; the cut is one more launch.  A NaN in the correlation is the maximum (``np.max`` / ``np.argmax``)."""
    t0 = time.time()
    rx, grid, back = _adopt(signal_rx, "electrical_signal")
    if isinstance(rx, electrical_signal):
        sps, raw = int(grid.sps), rx._raw("signal")
    elif isinstance(rx, np.ndarray):
        if sps is None:
            raise ValueError('"sps" must be provided to perform synchronization.')
        sps, raw = operator.index(sps), rx
    else:
        raise TypeError('The "signal_rx" must be of type `electrical_signal` or `np.ndarray`.')
    bits, nbits = _slots(slots_tx, strict=True)
    if raw.ndim != 1:
        raise ValueError(f"Signal must be scalar or 1D array for electrical_signal, invalid shape {tuple(raw.shape)}")
    if np.dtype(raw.dtype).kind == "c":
        raise TypeError("SYNC correlates real records on the device; a complex `signal_rx` is not taken (there is no CPU fallback)")
    if sps < 1:
        raise ValueError(f'"sps" must be a positive integer, got {sps}')
    n, l = int(raw.size), nbits * sps
    if n < l:
        raise BufferError('The length of the received vector must be greater than the transmitted vector!!')
    W = min(n, 2 * l)
    nc = W - l + 1
    M = 1 << max(8, (W - 1).bit_length())
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if M > (1 << hi):
        raise ValueError(f"SYNC: a correlation window of {W} samples exceeds the device path (2^{hi} points; there is no CPU fallback)")
    dev = default_device() if device is None else int(device)
    x = _dev_array(raw, np.float64, dev)
    b = _bits_on(dev, bits)
    st = np.zeros(4)
    plan = get_plan(M, 1, _lib.C128, dev)
    with plan.lock:
        _correlate(plan, x, b, sps, W)
        _lib.api.ssfm_sync_peak(plan.field_device_ptr, 2, nc, _lib._ptr(st), st.size)
    peak, i, std = float(st[0]), int(st[1]), float(st[3])
    if peak < 3 * std:
        raise ValueError('No correlation maximum found!!')
    start, stop, _ = slice(i, -(l - i)).indices(n)
    count = max(stop - start, 0)
    if count < 1:
        raise ValueError(f"Signal must be scalar or 1D array for electrical_signal, invalid shape {(0,)}")
    out = _lib.DeviceArray((count,), np.float64, dev)
    _lib.api.ssfm_signal_slice(1, n, x, None, 0, start, 1, count, out, None)
    output = _wrap_out(electrical_signal, out, NULL)
    output.execution_time = time.time() - t0
    return back((output, i))


def GET_EYE_v2(sync_signal, slots_tx, nslots: int = 4096, *, device=None):
    """Eye parameters from the slots known to have been sent, reference ``lab.py:158-273``: the signal is truncated to a multiple of
    ``2 sps`` and to ``nslots`` slots, ``ones`` / ``zeros`` are the samples of ``Re(signal + noise)`` whose slot was sent as 1 / as 0, and
    ``mu0``, ``mu1``, ``s0``, ``s1`` are the moments of those whose time within the slot lies strictly inside ``(-0.05, 0.05)``;
    ``threshold`` is the argmin over ``linspace(mu0, mu1, 500)`` of the Gaussian KDE (Scott's factor) of those samples.  Returns
    :class:`~opticomlib_amd.typing.eye`: ``y`` (the rolled signal), ``ones`` and ``zeros`` stay in GPU memory until they are read; ``t``, ``t0``
    and ``t1`` are formed on the host on first access.

    A ``slots_tx`` shorter than the slots in use raises ``IndexError`` (the reference's boolean index); span samples that are all equal raise
    ``numpy.linalg.LinAlgError`` (the reference's singular ``gaussian_kde``).  Up to 2^21 samples; there is no CPU fallback.

    The KDE adds its kernels in sample order, the reference over the zeros first and the ones after them: the sums differ by rounding only."""
    t0 = time.time()
    input, grid, _ = _adopt(sync_signal, "electrical_signal")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    bits, nbits = _slots(slots_tx, strict=False)
    if input.ndim != 1:
        raise ValueError("`sync_signal` must be a 1D-array.")
    sps, dt = int(grid.sps), grid.dt
    size = input.size - input.size % (2 * sps)
    nslots = min(size // sps, int(nslots))
    if nslots < 1:
        raise ValueError(f"GET_EYE_v2 needs at least one slot, got {nslots} (signal of {input.size} samples at sps={sps})")
    n = nslots * sps
    if nbits < nslots:
        raise IndexError(f"boolean index did not match indexed array along axis 0; size of axis is {n} but size of corresponding boolean axis is {nbits * sps}")
    if n > _EYE_MAX_N:
        raise ValueError(f"GET_EYE_v2 on the device takes up to 2^21 samples, got {n} (there is no CPU fallback)")
    dev = default_device() if device is None else int(device)
    b = _bits_on(dev, bits)
    x = _real_sum_device(input, n, 0, dev)
    y = _real_sum_device(input, n, -sps // 2 + 1, dev)
    t_span0, t_span1 = 0 - 0.05 * 1, 0 + 0.05 * 1
    tg = np.linspace(-0.5, 0.5, sps, endpoint=False)
    ks = np.nonzero((tg > t_span0) & (tg < t_span1))[0]
    k_lo, k_hi = (int(ks[0]), int(ks[-1]) + 1) if ks.size else (0, 0)
    lv = np.zeros(64)
    _lib.api.ssfm_eye_levels_known(x, n, sps, k_lo, k_hi, b, 500, _lib._ptr(lv), lv.size)
    L = lambda name: float(lv[_EYE_STATE[name]])             # noqa: E731
    mu0, mu1, s0, s1 = L("MU0"), L("MU1"), L("SD0"), L("SD1")
    if L("SINGULAR"):
        if L("NC") < 2:
            raise ValueError("`dataset` input should have multiple elements.")
        if not L("CVAR") > 0:
            raise np.linalg.LinAlgError("GET_EYE_v2: the samples at the centre of the eye are all equal: the covariance of the Gaussian KDE is singular")
        threshold = float("nan")                                # a level without a sample: the grid's ends are NaN
    else:
        threshold = float(np.linspace(mu0, mu1, 500)[int(L("KDE"))])
    cnt = np.zeros(64)
    _lib.api.ssfm_eye_split_known(None, nslots, sps, b, None, None, _lib._ptr(cnt), cnt.size)
    n0, n1 = int(cnt[_EYE_STATE["N0"]]), int(cnt[_EYE_STATE["N1"]])
    ones = _lib.DeviceArray((max(n1, 1) * sps,), np.float64, dev)
    zeros = _lib.DeviceArray((max(n0, 1) * sps,), np.float64, dev)
    _lib.api.ssfm_eye_split_known(x, nslots, sps, b, ones, zeros, _lib._ptr(cnt), cnt.size)
    d = {"sps": sps, "dt": dt, "y": y, "ones": ones if n1 else np.empty(0), "zeros": zeros if n0 else np.empty(0), "_nslots": nslots, "_n0": n0, "_n1": n1,
         "i": sps // 2, "t_left": -0.5, "t_right": 0.5, "y_left": None, "y_right": None, "t_dist": 1, "t_opt": 0, "t_span0": t_span0, "t_span1": t_span1,
         "mu0": mu0, "mu1": mu1, "s0": s0, "s1": s1, "threshold": threshold}
    with np.errstate(divide="ignore", invalid="ignore"):
        d["er"] = 10 * np.log10(mu1 / mu0) if mu0 > 0 else np.inf if mu0 == 0 else np.nan
    d["eye_h"] = mu1 - 3 * s1 - mu0 - 3 * s0
    d["execution_time"] = time.time() - t0
    return eye(**d)
