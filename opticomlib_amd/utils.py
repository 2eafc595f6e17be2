"""Spectral estimation on the device: :func:`get_psd` (reference ``utils.py:2048-2079``) and the spectrum behind the signals'
``.psd()`` plots (``typing.py:1850-1970``).

The reference wraps ``scipy.signal.welch``; here the same estimate -- periodic Hann window, ``noverlap = nperseg // 2``,
``nfft = nperseg``, no detrend, ``scaling='spectrum'``, two-sided, mean over the segments -- runs in the HIP kernels of
``csrc/psd.hip`` on the field where it lies (a device-resident signal is read in place, only the result comes back).
All arithmetic is float64.  There is no host fallback.
"""
from __future__ import annotations

import warnings
from collections.abc import Iterable

import numpy as np

from . import _lib
from .typing import _is_device

DIRECT_MAX = 15               # route 2: nperseg < 16, a direct DFT per segment
POW2_MIN, POW2_MAX = 16, 8192  # route 1: one workgroup line transform per segment
CHUNK_BYTES = 256 << 20       # route 3: chunk_rows x M x 16 B of the chirp-z plan stays at or below this
_MAX_GRID_ROWS = 65535        # ssfm_welch, ssfm_welch_finish: rows per call (grid.y)
_MAX_PLAN_BATCH = 65535       # route 3: rows of a plan (ssfm_plan_create)


def _welch_layout(n: int, nperseg: int) -> dict:
    """SciPy's segmenting of ``n`` samples (``nperseg`` already validated and clamped to ``n``): ``noverlap = nperseg // 2``,
    ``step = nperseg - noverlap``, ``nseg = (n - noverlap) // step`` (the trailing samples are dropped), and the route:
    1 = power of two of 16 ... 8192 (line kernel), 2 = nperseg < 16 (direct DFT), 3 = anything else (chirp-z transform)."""
    n, nperseg = int(n), int(nperseg)
    noverlap = nperseg // 2
    step = nperseg - noverlap
    nseg = (n - noverlap) // step
    if nperseg <= DIRECT_MAX:
        route = 2
    elif POW2_MIN <= nperseg <= POW2_MAX and nperseg & (nperseg - 1) == 0:
        route = 1
    else:
        route = 3
    return {"nseg": nseg, "noverlap": noverlap, "step": step, "route": route}


def _hann_scale(nperseg: int) -> float:
    """``1 / sum(w)^2`` of ``scipy.signal.get_window('hann', nperseg)`` (periodic), computed the way SciPy builds the window."""
    if nperseg == 1:
        return 1.0
    fac = np.linspace(-np.pi, np.pi, nperseg + 1)
    w = np.zeros(nperseg + 1)
    w += 0.5 * np.cos(0 * fac)
    w += 0.5 * np.cos(1 * fac)
    return float(1.0 / w[:-1].sum() ** 2)


def _validate_nperseg(nperseg, n: int) -> int:
    """SciPy 1.15's ``_triage_segments`` for a string window: cast to int, reject < 1, clamp to the input length with its warning."""
    nperseg = int(nperseg)
    if nperseg < 1:
        raise ValueError("nperseg must be a positive integer")
    if nperseg > n:
        warnings.warn(f"nperseg = {nperseg:d} is greater than input length  = {n:d}, using nperseg = {n:d}", UserWarning, stacklevel=3)
        nperseg = n
    return nperseg


def _out_f32(dtype) -> bool:
    """SciPy computes in ``result_type(x, complex64)``: single precision for float32 / complex64 (and for the small integer, bool and float16 types)."""
    return np.result_type(np.dtype(dtype), np.complex64) == np.dtype(np.complex64)


_CODES = {np.dtype(np.complex64): _lib.C64, np.dtype(np.complex128): _lib.C128, np.dtype(np.float64): _lib.F64_REAL}


def _on_device(x, dev: int):
    """``x`` (host array or DeviceArray) as a DeviceArray the kernels read: complex64, complex128 or float64 (other real types widen to
    float64, other complex types to complex128).  A device array of one of those types is used where it lies."""
    if _is_device(x):
        if np.dtype(x.dtype) in _CODES:
            return x
        x = x.to_host()
    x = np.asarray(x)
    if x.dtype not in _CODES:
        x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    return _lib.DeviceArray.from_host(np.ascontiguousarray(x), device=dev)


def _check_chirp_length(nperseg: int) -> None:
    """Route 3 runs on the chirp-z engine, whose line of M >= 2 nperseg - 1 points has a largest size: refuse a longer segment."""
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if 2 * nperseg - 1 > (1 << hi):
        raise ValueError(f"the device transform takes 2 ... 2^{hi - 1} samples per row, got {nperseg} (there is no CPU fallback)")


def _welch_device(d, rows: int, n: int, ld: int, nperseg: int, out_f32: bool, dev: int) -> np.ndarray:
    """(rows, nperseg) fftshifted Welch estimate of the first ``n`` elements of every row of the device array ``d`` (rows ``ld`` apart)."""
    lay = _welch_layout(n, nperseg)
    code = _CODES[np.dtype(d.dtype)]
    itemsize = np.dtype(d.dtype).itemsize
    scale = _hann_scale(nperseg)
    odt = np.float32 if out_f32 else np.float64
    out = _lib.host_empty((rows, nperseg), odt)
    if lay["route"] in (1, 2):
        for r0 in range(0, rows, _MAX_GRID_ROWS):
            r1 = min(rows, r0 + _MAX_GRID_ROWS)
            _lib.api.ssfm_welch(dev, d.ptr + r0 * ld * itemsize, code, r1 - r0, n, ld, nperseg, scale, int(out_f32), out.ctypes.data + r0 * nperseg * out.itemsize)
        return out
    from .devices import _ChirpZ
    _check_chirp_length(nperseg)
    nseg = lay["nseg"]
    total = rows * nseg
    M = 1 << max(8, (2 * nperseg - 2).bit_length())             # the chirp-z plan's line (devices._ChirpZ)
    chunk = max(1, min(total, CHUNK_BYTES // (M * 16), _MAX_PLAN_BATCH))
    frames = _lib.DeviceArray((chunk, nperseg), np.complex128, dev)
    acc = _lib.zeros_device((rows, nperseg), np.float64, dev)
    with _ChirpZ(nperseg, chunk, dev) as eng:
        for first in range(0, total, chunk):
            count = min(chunk, total - first)
            _lib.api.ssfm_welch_frames(dev, d, code, rows, n, ld, nperseg, first, count, chunk, frames)
            eng.fourier(frames, False)
            _lib.api.ssfm_welch_accumulate(dev, frames, nperseg, rows, nseg, first, count, acc)
    for r0 in range(0, rows, _MAX_GRID_ROWS):                      # ssfm_welch_finish takes at most 65535 rows, as ssfm_welch does
        r1 = min(rows, r0 + _MAX_GRID_ROWS)
        _lib.api.ssfm_welch_finish(dev, acc.ptr + r0 * nperseg * 8, r1 - r0, nperseg, scale / nseg, int(out_f32), out.ctypes.data + r0 * nperseg * out.itemsize)
    return out


def _welch(x, fs, nperseg, n=None, device=None):
    """``fftshift`` of ``scipy.signal.welch(x[..., :n], fs, nperseg, scaling='spectrum', return_onesided=False, detrend=False)`` along the last
    axis, on the device.  ``x``: NumPy array or DeviceArray; ``n``: use only the first ``n`` samples of every row (no copy)."""
    shape = tuple(int(s) for s in x.shape)
    if len(shape) == 0:
        raise ValueError("the input must have at least one dimension")
    ld = shape[-1]
    n = ld if n is None else int(n)
    lead = shape[:-1]
    out_f32 = _out_f32(x.dtype)
    if n == 0 or int(np.prod(lead)) == 0:                          # SciPy: empty in, empty out (before any check of nperseg)
        e = np.empty(lead + (n,))
        return np.fft.fftshift(e), np.fft.fftshift(e, axes=-1)
    nperseg = _validate_nperseg(nperseg, n)
    f = np.fft.fftshift(np.fft.fftfreq(nperseg, 1 / fs))
    rows = int(np.prod(lead)) if lead else 1
    if device is None:
        from .devices import default_device
        device = x.device if _is_device(x) else default_device()
    dev = int(device)
    if _is_device(x) and x.device != dev:
        x = x.to_host()
    if not _is_device(x) and n != ld:
        x = np.asarray(x)[..., :n]
        ld = n
    if _welch_layout(n, nperseg)["route"] == 3:
        _check_chirp_length(nperseg)                              # before anything is uploaded or allocated
    d = _on_device(x, dev)
    psd = _welch_device(d, rows, n, ld, nperseg, out_f32, dev)
    return f, psd.reshape(lead + (nperseg,))


def _is_array_like(obj) -> bool:
    """The reference's ``_is_iterable_and_numpy_compatible``: iterable, convertible by ``np.array``, numeric throughout."""
    if isinstance(obj, np.ndarray):
        return obj.dtype.kind in "biufc"
    if not isinstance(obj, Iterable):
        return False
    try:
        a = np.array(obj)
    except Exception:
        return False
    return a.dtype.kind in "biufc"


def get_psd(signal, fs, nperseg=None, *, device=None):
    """Power spectral density by Welch's method (reference ``opticomlib.utils.get_psd``), computed on the GPU.

    Parameters
    ----------
    signal : array_like, or an object with a ``.signal`` attribute
        Input.  Only the signal is used, never the noise (as in the reference).  This package's own signal classes are read where
        they lie: a device-resident field is not copied to the host.  1-D or 2-D (any leading shape is taken as rows); the
        transform runs along the last axis.
    fs : float
        Sampling frequency.  ``f`` comes out in the same unit.
    nperseg : int, optional
        Segment length.  Default: ``min(2048, len(sig))``, exactly the reference's rule -- note that ``len`` of a 2-D
        (dual-polarisation) array is its number of rows, so such an input gets ``nperseg = 2`` and a ``(2, 2)`` result; this
        quirk is kept on purpose (the function is a drop-in).  As in SciPy 1.15: cast to ``int``, ``ValueError`` below 1,
        a ``UserWarning`` and the input length when it is longer than the input.
    device : int, optional
        GPU index.  Default: the device a device-resident input lies on, else this process's device.

    Returns
    -------
    f : np.ndarray
        ``fftshift(fftfreq(nperseg, 1 / fs))``, float64.
    psd : np.ndarray
        The two-sided spectrum (``scaling='spectrum'``), fftshifted along the last axis; float32 where SciPy computes in single
        precision (float32 / complex64 input), float64 otherwise.
    """
    from .typing import electrical_signal, optical_signal
    if isinstance(signal, (electrical_signal, optical_signal)):
        sig = signal._raw("signal")
    elif hasattr(signal, "signal"):
        sig = signal.signal
    elif _is_array_like(signal):
        sig = np.array(signal)
    else:
        raise TypeError("signal must be array_like or have a .signal attribute")
    if not _is_device(sig):
        sig = np.asarray(sig)
    nperseg = nperseg if nperseg is not None else _default_nperseg(sig)
    return _welch(sig, fs, nperseg, device=device)


def _default_nperseg(sig) -> int:
    """The reference's default, ``min(2048, len(sig))``: ``len`` of a 2-D array is its number of rows (2 for a dual-polarisation field)."""
    return min(2048, len(sig))


def _dbm(x):
    """The reference's ``dbm`` (``utils.py:388-417``): ``10 log10(x) + 30``; no warning at zero."""
    x = np.asarray(x)
    if (x < 0).any():
        raise ValueError("Some values of input array are negative.")
    with np.errstate(divide="ignore"):
        return 10 * np.log10(x) + 30


def plot_psd(obj, fmt='-', mode='x', n=None, xlabel=None, ylabel=None, yscale='dbm', grid=False, hold=True, show=False, **kwargs):
    """The body of ``electrical_signal.psd()`` / ``optical_signal.psd()`` (reference ``typing.py:1850-1970``) with the spectrum from the device."""
    import matplotlib.pyplot as plt
    from .typing import gv

    size = obj.size
    n = min(size, gv.t.size) if n is None else n
    m = len(range(size)[slice(None, n)])                          # the length of self[:n]
    raw = obj._raw("signal")
    nperseg = 2048 if m > 2048 else m
    f, psd = _welch(raw, gv.fs * 1e-9, nperseg, n=m)

    if yscale == 'linear':
        psd = psd * 1e3
        ylabel = ylabel if ylabel else 'Power [mW]'
        ylim = (-0.1,)
    elif yscale == 'dbm':
        psd = _dbm(psd)
        ylabel = ylabel if ylabel else 'Power [dBm]'
        ylim = (-100,)
    else:
        raise TypeError('`yscale` must be one of the following values ("linear", "dbm")')

    n_pol = getattr(obj, 'n_pol', 1)
    if n_pol == 1:
        if not isinstance(fmt, str):
            warnings.warn('`fmt` must be a string for single polarization signals, using default value.')
            fmt = '-'
        args = (f, psd, fmt)
    else:
        if mode == 'x':
            if not isinstance(fmt, str):
                warnings.warn('`fmt` must be a string for single polarization signals, using default value.')
                fmt = '-'
            args = (f, psd[0], fmt)
        elif mode == 'y':
            if not isinstance(fmt, str):
                warnings.warn('`fmt` must be a string for single polarization signals, using default value.')
                fmt = '-'
            args = (f, psd[1], fmt)
        elif mode == 'both':
            if isinstance(fmt, (list, tuple)):
                args = (f, psd[0], fmt[0], f, psd[1], fmt[1])
            elif isinstance(fmt, str):
                args = (f, psd[0], fmt, f, psd[1], fmt)
            else:
                warnings.warn('`fmt` must be a string or a list of strings for both polarizations signals, using default value.')
                args = (f, psd[0], '-', f, psd[1], '-')
        else:
            raise TypeError('argument `mode` should be ("x", "y" or "both")')

    label = kwargs.pop('label', None) if mode == 'both' and n_pol > 1 else None

    if not hold:
        plt.figure()

    ls = plt.plot(*args, **kwargs)
    plt.ylabel(ylabel)
    plt.xlabel(xlabel if xlabel else 'Frequency [GHz]')
    plt.xlim(-3.5 * gv.R * 1e-9, 3.5 * gv.R * 1e-9)
    plt.ylim(*ylim)
    if grid:
        plt.grid(alpha=0.3)

    if label is not None:
        if isinstance(label, str):
            ls[0].set_label(label + ' X')
            ls[1].set_label(label + ' Y')
        elif isinstance(label, (list, tuple)):
            ls[0].set_label(label[0])
            ls[1].set_label(label[1])
        else:
            raise ValueError('`label` must be a string or a list of strings.')
        plt.legend()
    if show:
        plt.show()
    return obj


__all__ = ["get_psd"]
