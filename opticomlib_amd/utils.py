"""Spectral estimation on the device: :func:`get_psd` (reference ``utils.py:2048-2079``) and the spectrum behind the signals'
``.psd()`` plots (``typing.py:1850-1970``).

The reference wraps ``scipy.signal.welch``; here the same estimate -- periodic Hann window, ``noverlap = nperseg // 2``,
``nfft = nperseg``, no detrend, ``scaling='spectrum'``, two-sided, mean over the segments -- runs in the HIP kernels of
``csrc/psd.hip`` on the field where it lies (a device-resident signal is read in place, only the result comes back).
All arithmetic is float64.  There is no host fallback.

Also the eye diagram (reference ``utils.py:1593-1787``): :func:`eye_density` computes the picture's data -- ``np.histogram2d`` of the traces'
points, ``scipy.ndimage.gaussian_filter`` of the counts, the plotted points' colours -- where the record lies (``csrc/eye_density.hip`` for a
record in GPU memory, NumPy / SciPy for a host record), and :func:`eyediagram` draws it.
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


# ----------------------------------------------------------------------------- the eye diagram's density (csrc/eye_density.hip)
EYE_CHUNK_POINTS = 32768      # csrc/eye_density.hip kChunkPoints: a workgroup of the counting kernel takes max(1, 32768 // (2 sps)) traces
EYE_MAX_BINS = 4096           # csrc/eye_density.hip kMaxBins (the device path; the host path is NumPy's and has no limit)
_EYE_STYLES = ("line", "dot", "density")


class EyeDensity:
    """What :func:`eye_density` returns (host arrays): ``grid`` the blurred density, (B, B) float64, ``grid[ix, iy]``; ``counts`` the integer
    counts before the blur; ``xedges``, ``yedges``; ``extent = (min_x, max_x, min_y, max_y)``; ``n_traces``; with ``colors=True`` also ``x``,
    ``y``, ``colors`` of the ``n_traces * 2 sps`` plotted points and their grid indices ``ix``, ``iy`` (else None)."""
    __slots__ = ("grid", "counts", "xedges", "yedges", "extent", "n_traces", "x", "y", "colors", "ix", "iy")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _eye_geometry(n: int, sps: int, n_traces):
    """``(start, P, T)`` of the reference's truncation (``utils.py:1651-1670``), with its errors and their texts."""
    start, end = sps // 2, n - sps // 2
    if start >= end:
        raise ValueError(f"Signal too short for truncation. Need at least {sps} samples, got {n}.")
    P = 2 * sps
    if end - start < P:
        raise ValueError(f"Need at least {P} points for eye diagram, got {end - start} after truncation.")
    available = (end - start) // P
    T = min(available, n_traces) if n_traces is not None else available
    if T == 0:
        raise ValueError(f"Not enough points to form even one trace of {P} points after truncation.")
    if T < 0:
        raise ValueError(f"n_traces must not be negative, got {n_traces}")
    return start, P, int(T)


def _hist_edges(lo, hi, bins: int) -> np.ndarray:
    """The edges ``np.histogramdd`` forms for an integer ``bins``: its ``_get_outer_edges`` (the error for a range that is not finite, +- 0.5
    around a single value), then ``np.linspace``."""
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    with np.errstate(all="ignore"):
        return np.linspace(lo, hi, bins + 1)


def _hist_bins(edges: np.ndarray, v: np.ndarray) -> np.ndarray:
    """``np.histogramdd``'s bin of every value: ``searchsorted(side='right') - 1``, a value equal to the last edge in the last bin."""
    b = np.searchsorted(edges, v, side="right")
    b[v == edges[-1]] -= 1
    return b - 1


def _grid_index(v, lo, hi, bins: int) -> np.ndarray:
    """The reference's grid index of plotted values (``utils.py:1705-1715``)."""
    with np.errstate(all="ignore"):
        vn = np.zeros_like(v) if hi == lo else (v - lo) / (hi - lo)
        return np.clip((vn * (bins - 1)).astype(int), 0, bins - 1)


def _gauss_weights(sigma: float):
    """``scipy.ndimage``'s Gaussian kernel of ``gaussian_filter(sigma, truncate=4)``: ``(radius, weights[radius:])`` -- the centre's weight first --
    or ``(0, None)`` where SciPy skips the axis (``sigma <= 1e-15``)."""
    sigma = float(sigma)
    if not sigma > 1e-15:
        if sigma < 0 or sigma != sigma:
            raise ValueError("grid_sigma must not be negative")
        return 0, None
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return r, np.ascontiguousarray(phi[r:])


def _eye_record(y, device):
    """``(signal, noise or None, on_device)`` of the record behind ``y``: DeviceArrays where it lies in GPU memory, one float64 host array else."""
    from .typing import NULL, electrical_signal
    complex_error = TypeError("the eye diagram takes a real record: pass `.real` or `.abs()` of a complex signal")
    if isinstance(y, electrical_signal) and y.on_device:
        s, n = y._device_arrays()
        if s.dtype.kind == "c":
            raise complex_error
        return s, n, True
    if _is_device(y):
        if np.dtype(y.dtype) != np.dtype(np.float64):
            if np.dtype(y.dtype).kind == "c":
                raise complex_error
            raise TypeError(f"the eye diagram takes a float64 device array, not {y.dtype}")
        if y.ndim != 1:
            raise ValueError(f"the eye diagram takes a 1-D record, got shape {y.shape}")
        return y, None, True
    if isinstance(y, electrical_signal):
        a = np.asarray(y.signal + y.noise)
    else:
        a = np.asarray(y)
    if a.dtype.kind == "c":
        raise complex_error
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"the eye diagram takes a 1-D record, got shape {a.shape}")
    if device is not None:                                         # an explicit device: the host record is uploaded and computed there
        return _lib.DeviceArray.from_host(a, device=int(device)), None, True
    return a, None, False


def _eye_density_host(a, start, P, T, B, sigma, X1, colors):
    from scipy.ndimage import gaussian_filter
    Y = a[start:start + T * P]
    X = np.tile(X1, T)
    min_y, max_y = Y.min(), Y.max()
    with np.errstate(all="ignore"):
        counts, xe, ye = np.histogram2d(X, Y, bins=B)
    grid = gaussian_filter(counts, sigma=sigma)
    out = dict(grid=grid, counts=counts.astype(np.uint32), xedges=xe, yedges=ye, extent=(X1.min(), X1.max(), min_y, max_y), n_traces=T)
    if colors:
        ix, iy = _grid_index(X, X1.min(), X1.max(), B), _grid_index(Y, min_y, max_y, B)
        c = grid[ix, iy]
        span = c.max() - c.min()
        out.update(x=X, y=Y, ix=ix, iy=iy, colors=np.zeros_like(c) if span == 0 else (c - c.min()) / span)
    return EyeDensity(**out)


def _eye_density_device(s, nz, start, P, T, B, sigma, X1, colors, n_traces):
    import ctypes as C
    if nz is not None and (nz.device != s.device or nz.shape != s.shape):
        raise ValueError("signal and noise differ in shape or device")
    if B > EYE_MAX_BINS:
        raise ValueError(f"the device path takes N_grid_bins up to {EYE_MAX_BINS}, got {B}")
    n, sps, nt = s.size, P // 2, -1 if n_traces is None else int(n_traces)
    rng = (C.c_double * 3)()
    _lib.api.ssfm_eye_density_range(s, nz, n, sps, nt, rng)
    flags = int(rng[2])
    min_y, max_y = (np.float64(np.nan),) * 2 if flags & 1 else (np.float64(rng[0]), np.float64(rng[1]))
    ye = _hist_edges(min_y, max_y, B)                             # (raises NumPy's error for a range that is not finite: nothing further is launched)
    if not np.isfinite(ye).all() and B > 1:
        # max - min overflows: linspace gives [nan, inf, ..., inf, max], the maximum's searchsorted index is 0, its shift makes it -1 and
        # np.ravel_multi_index refuses it -- the maximum is always among the points, so NumPy always raises here
        raise ValueError("invalid entry in coordinates array")
    min_x, max_x = X1.min(), X1.max()
    xe = _hist_edges(min_x, max_x, B)
    xbin = np.ascontiguousarray(_hist_bins(xe, X1), dtype=np.int32)
    r, w = _gauss_weights(sigma)
    counts = _lib.host_empty((B, B), np.uint32)
    grid = _lib.host_empty((B, B), np.float64)
    out = dict(xedges=xe, yedges=ye, extent=(min_x, max_x, min_y, max_y), n_traces=T)
    points = (None, 0.0, 0.0, None, None, None)                   # no colours: the plotted points stay on the device
    if colors:
        xidx = np.ascontiguousarray(_grid_index(X1, min_x, max_x, B), dtype=np.int32)
        pts, iy, col = (_lib.host_empty((T * P,), dt) for dt in (np.float64, np.int32, np.float64))
        points = (_lib._ptr(xidx), float(min_y), float(max_y), _lib._ptr(pts), _lib._ptr(iy), _lib._ptr(col))
    _lib.api.ssfm_eye_density(s, nz, n, sps, nt, B, _lib._ptr(ye), _lib._ptr(xbin), None if w is None else _lib._ptr(w), r, _lib._ptr(counts),
                              _lib._ptr(grid), *points)
    _lib.TRANSFERS["d2h"] += 2                                     # counts and grid
    if colors:
        _lib.TRANSFERS["d2h"] += 3                                 # the points' values, indices and colours
        out.update(x=np.tile(X1, T), y=pts, colors=col, ix=np.tile(xidx.astype(np.intp), T), iy=iy.astype(np.intp))
    return EyeDensity(grid=grid, counts=counts, **out)


def eye_density(y, sps, n_traces=None, N_grid_bins=200, grid_sigma=5, *, colors=False, device=None):
    """The density behind an eye diagram (the computed part of the reference's ``opticomlib.utils.eyediagram``): the record is cut by ``sps // 2``
    samples at both ends and folded into traces of ``2 sps`` points over the abscissa ``linspace(-1, 1 - 1/sps, 2 sps)``; the result holds
    ``np.histogram2d(X, Y, bins=N_grid_bins)``, its ``scipy.ndimage.gaussian_filter(sigma=grid_sigma)`` and, with ``colors=True``, each plotted
    point's normalised grid value.

    ``y``: an ``electrical_signal`` (signal + noise), a float64 ``DeviceArray`` or array_like.  A record in GPU memory is computed there by the
    kernels of ``csrc/eye_density.hip`` -- only the grid (and with ``colors=True`` the plotted points) comes back; host data is NumPy / SciPy on
    the host and needs no GPU, unless ``device`` names one.  A complex record raises ``TypeError`` (take ``.real`` or ``.abs()``).
    ``n_traces``: the most traces to take (default: all).  Returns an :class:`EyeDensity`.

    Raises the reference's ``ValueError`` s for a record too short for the truncation, with fewer than ``2 sps`` points after it, or with no trace
    to draw, and NumPy's ("autodetected range of [...] is not finite") for a NaN or an infinity among the plotted points.  On the device
    ``N_grid_bins <= 4096`` and the record holds at most 2^31 samples."""
    sps, B = int(sps), int(N_grid_bins)
    if sps < 1:
        raise ValueError(f"sps must be a positive integer, got {sps}")
    if B < 1:
        raise ValueError("`bins[0]` must be positive, when an integer")
    s, nz, on_device = _eye_record(y, device)
    start, P, T = _eye_geometry(int(s.size), sps, n_traces)
    X1 = np.linspace(-1, 1 - 1 / sps, P)
    if on_device:
        if device is not None and int(device) != s.device:
            raise ValueError(f"the record lies on GPU {s.device}, not on GPU {int(device)}")
        return _eye_density_device(s, nz, start, P, T, B, grid_sigma, X1, colors, n_traces)
    return _eye_density_host(s, start, P, T, B, grid_sigma, X1, colors)


def eyediagram(y, sps, n_traces=None, cmap='viridis', N_grid_bins=200, grid_sigma=5, style='dot', ax=None, **plot_kw):
    """Plot a coloured eye diagram (reference ``opticomlib.utils.eyediagram``) from :func:`eye_density`, which computes where the record lies.

    ``style``: ``'dot'`` one scatter of the points coloured by density (``s`` 0.1, ``alpha`` 0.9), ``'line'`` one ``LineCollection`` per trace
    (``linewidth`` 1, ``alpha`` 0.05, ``capstyle`` / ``joinstyle`` 'round'), ``'density'`` the blurred grid alone (``imshow``).  ``plot_kw``:
    ``figsize``, ``dpi`` (100) for a new figure; ``xlabel``, ``ylabel``, ``title`` (``"Eye Diagram ({num_traces} traces)"``), ``grid`` (True),
    ``grid_alpha`` (0.3), ``xlim`` ((-1, 1)), ``ylim`` ((min_y, max_y)), ``tight_layout`` (True), ``show`` (False) -- the defaults the reference's
    code uses.  Everything is drawn on ``ax`` (a new figure's axes when None).  Returns the axes."""
    from .typing import electrical_signal
    sps = int(sps)
    size = y.size if isinstance(y, electrical_signal) or _is_device(y) else len(y)
    _eye_geometry(int(size), sps, n_traces)                        # the reference's errors, in its order, before anything is computed
    if style not in _EYE_STYLES:
        raise ValueError(f"Invalid style '{style}'. Choose from 'line', 'dot', or 'density'.")
    import matplotlib.pyplot as plt
    try:
        cmap_obj = getattr(plt.cm, cmap)
    except AttributeError:
        warnings.warn(f"Colormap '{cmap}' not found. Using 'viridis' by default.")
        cmap_obj = plt.cm.viridis
    d = eye_density(y, sps, n_traces, N_grid_bins, grid_sigma, colors=style != 'density')
    min_x, max_x, min_y, max_y = d.extent
    created = ax is None
    if created:
        _, ax = plt.subplots(figsize=plot_kw.get('figsize', None), dpi=plot_kw.get('dpi', 100))
    if style == 'dot':
        ax.scatter(d.x, d.y, c=d.colors, cmap=cmap_obj, s=plot_kw.get('s', 0.1), alpha=plot_kw.get('alpha', 0.9))
    elif style == 'density':
        ax.imshow(d.grid.T, extent=[min_x, max_x, min_y, max_y], origin='lower', aspect='auto', cmap=cmap_obj)
    else:
        from matplotlib.collections import LineCollection
        P = 2 * sps
        Y, col = d.y.reshape(d.n_traces, P), d.colors.reshape(d.n_traces, P)
        for i in range(d.n_traces):
            points = np.array([d.x[:P], Y[i]]).T.reshape(-1, 1, 2)
            segments = np.concatenate([points[:-1], points[1:]], axis=1)
            if len(segments) > 0:
                ax.add_collection(LineCollection(segments, colors=cmap_obj(col[i][:len(segments)]), linewidth=plot_kw.get('linewidth', 1),
                                                 alpha=plot_kw.get('alpha', 0.05), capstyle=plot_kw.get('capstyle', 'round'),
                                                 joinstyle=plot_kw.get('joinstyle', 'round')))
    xlim, ylim = plot_kw.get('xlim', None), plot_kw.get('ylim', None)
    ax.set_xlim(xlim if xlim is not None else (-1, 1))
    ax.set_ylim(ylim if ylim is not None else (min_y, max_y))
    ax.set_xlabel(plot_kw.get('xlabel', "Time (2-symbol segment)"))
    ax.set_ylabel(plot_kw.get('ylabel', "Amplitude"))
    ax.set_title(plot_kw.get('title', "Eye Diagram ({num_traces} traces)").format(num_traces=d.n_traces))
    if plot_kw.get('grid', True):
        ax.grid(True, alpha=plot_kw.get('grid_alpha', 0.3))
    if created and plot_kw.get('tight_layout', True):
        plt.tight_layout()
    if created and plot_kw.get('show', False):
        plt.show()
    return ax


# ----------------------------------------------------------------------------- eye.plot's fold of the record (csrc/eye_density.hip, the fold entry points)
EYE_PLOT_BINS = 350           # reference typing.py:2721: the grid of eye.plot
EYE_PLOT_SIGMA = 3            # typing.py:2723
EYE_PLOT_HIST_BINS = 200      # typing.py:2782: the bins of the side histogram


class EyeFoldDensity(EyeDensity):
    """What :func:`eye_fold_density` returns (host arrays): the fields of :class:`EyeDensity` -- ``x``, ``y``, ``colors``, ``ix``, ``iy`` of the
    ``n_traces * 2 sps`` drawn points -- and with ``hist=(lo, hi)`` also ``hist_counts`` (200 integers), ``hist_edges`` (201) and ``n_masked``,
    the number of points whose abscissa lies strictly between ``lo`` and ``hi``."""
    __slots__ = ("hist_counts", "hist_edges", "n_masked")

    def __init__(self, **kw):
        for k in EyeDensity.__slots__ + self.__slots__:
            setattr(self, k, kw.get(k))


def _eye_plot_fold(eye_obj):
    """``(record, start, count, P, L, n_draw, tg)`` of the points ``eye.plot`` draws (reference ``typing.py:2718-2719`` and ``:2759-2764``):
    ``np.roll(y, -sps // 2)[sps // 2 : -sps // 2]`` is ``y[sps:]`` and ``t[:-sps]`` has the period ``P = 2 (sps_resamp or sps)``, so point
    ``j < count = n - sps`` is sample ``sps + j`` at phase ``j mod P``; the ``n_draw = count // (2 sps)`` drawn traces have ``L = 2 sps`` points.
    The record is read from ``eye_obj.__dict__`` so that one in GPU memory is not downloaded."""
    d = getattr(eye_obj, "__dict__", {})
    y = d.get("_y")
    if y is None or "t_opt" not in d or "sps" not in d:
        raise ValueError('Empty eye diagram object.')
    sps = int(d["sps"])
    tg = eye_obj._tgrid()
    if not _is_device(y):
        y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError(f"the eye diagram takes a 1-D record, got shape {y.shape}")
    n = int(y.size)
    if sps < 1 or n - sps < 1:
        raise ValueError(f"the eye's record of {n} samples at sps={sps} leaves no point to plot")
    count, L = n - sps, 2 * sps
    return y, sps, count, int(tg.size), L, count // L, tg


def _fold_tables(tg, count, lo_hi):
    """The abscissa's share of the fold, all on the host: ``(m, xedges, xbin, xidx, mask)`` -- ``m`` phases occur among the points, the
    histogram's x-edges span their abscissae, and every phase has its column, its colour index and (with ``lo_hi``) its pass through the window."""
    P, B = tg.size, EYE_PLOT_BINS
    m = min(count, P)
    min_x, max_x = tg[:m].min(), tg[:m].max()
    xe = _hist_edges(min_x, max_x, B)
    xbin = np.full(P, B - 1, dtype=np.int32)                       # (phases beyond the m-th never occur: any valid column)
    xbin[:m] = _hist_bins(xe, tg[:m])
    xidx = np.zeros(P, dtype=np.int32)
    xidx[:m] = _grid_index(tg[:m], min_x, max_x, B)
    mask = None
    if lo_hi is not None:
        mask = np.ascontiguousarray((tg > lo_hi[0]) & (tg < lo_hi[1]), dtype=np.uint8)
    return m, xe, xbin, xidx, mask


def _fold_hist_edges(n_masked, lo, hi):
    """The edges ``np.histogram(v, bins=200)`` forms for the masked points: over their range, or over (0, 1) when there is none."""
    return _hist_edges(lo, hi, EYE_PLOT_HIST_BINS) if n_masked else np.linspace(0.0, 1.0, EYE_PLOT_HIST_BINS + 1)


def _eye_fold_density_host(a, start, count, L, n_draw, tg, colors, hist):
    from scipy.ndimage import gaussian_filter
    B, P = EYE_PLOT_BINS, tg.size
    Y = a[start:start + count]
    X = np.tile(tg, -(-count // P))[:count]
    with np.errstate(all="ignore"):
        counts, xe, ye = np.histogram2d(X, Y, bins=B)
    grid = gaussian_filter(counts, sigma=EYE_PLOT_SIGMA)
    min_y, max_y = Y.min(), Y.max()
    out = dict(grid=grid, counts=counts.astype(np.uint32), xedges=xe, yedges=ye, extent=(X.min(), X.max(), min_y, max_y), n_traces=n_draw)
    if colors:
        ix, iy = _grid_index(X, X.min(), X.max(), B), _grid_index(Y, min_y, max_y, B)
        c = grid[ix, iy]
        with np.errstate(all="ignore"):
            c = (c - c.min()) / (c.max() - c.min())               # (unguarded, as the reference: NaN when every point has one colour)
        k = n_draw * L
        out.update(x=X[:k], y=Y[:k], ix=ix[:k], iy=iy[:k], colors=c[:k])
    if hist is not None:
        v = Y[(X > hist[0]) & (X < hist[1])]
        hc, he = np.histogram(v, bins=EYE_PLOT_HIST_BINS)
        out.update(hist_counts=hc.astype(np.uint32), hist_edges=he, n_masked=int(v.size))
    return EyeFoldDensity(**out)


def _eye_fold_density_device(s, start, count, L, n_draw, tg, colors, hist):
    import ctypes as C
    B, H, P, n = EYE_PLOT_BINS, EYE_PLOT_HIST_BINS, int(tg.size), int(s.size)
    m, xe, xbin, xidx, mask = _fold_tables(tg, count, hist)
    rng = (C.c_double * 7)()
    _lib.api.ssfm_eye_fold_range(s, n, start, count, P, None if mask is None else _lib._ptr(mask), rng)
    min_y, max_y = (np.float64(np.nan),) * 2 if int(rng[2]) & 1 else (np.float64(rng[0]), np.float64(rng[1]))
    ye = _hist_edges(min_y, max_y, B)                             # (raises NumPy's error for a range that is not finite: nothing further is launched)
    if not np.isfinite(ye).all():
        raise ValueError("invalid entry in coordinates array")    # max - min overflows: what np.histogram2d raises (see _eye_density_device)
    r, w = _gauss_weights(EYE_PLOT_SIGMA)
    counts = _lib.host_empty((B, B), np.uint32)
    grid = _lib.host_empty((B, B), np.float64)
    out = dict(xedges=xe, yedges=ye, extent=(tg[:m].min(), tg[:m].max(), min_y, max_y), n_traces=n_draw)
    k = n_draw * L
    points = (None, 0.0, 0.0, None, None, None)
    if colors:
        pts, iy, col = (_lib.host_empty((k,), dt) for dt in (np.float64, np.int32, np.float64))
        points = (_lib._ptr(xidx), float(min_y), float(max_y), _lib._ptr(pts), _lib._ptr(iy), _lib._ptr(col))
    side = (None, 0, None, None)
    if hist is not None:
        n_masked = int(rng[6])
        he = _fold_hist_edges(n_masked, np.float64(rng[3]), np.float64(rng[4]))
        hc = np.zeros(H, dtype=np.uint32)
        out.update(hist_counts=hc, hist_edges=he, n_masked=n_masked)
        if n_masked:
            side = (_lib._ptr(mask), H, _lib._ptr(he), _lib._ptr(hc))
    _lib.api.ssfm_eye_fold_density(s, n, start, count, P, L, n_draw, B, _lib._ptr(ye), _lib._ptr(xbin), _lib._ptr(w), r, _lib._ptr(counts),
                                   _lib._ptr(grid), *points, *side)
    _lib.TRANSFERS["d2h"] += 2 + (1 if side[3] is not None else 0)  # counts and grid; the side histogram's counts
    if colors:
        _lib.TRANSFERS["d2h"] += 3                                 # the drawn points' values, indices and colours
        reps = -(-k // P) if k else 0
        out.update(x=np.tile(tg, reps)[:k], y=pts, colors=col, ix=np.tile(xidx.astype(np.intp), reps)[:k], iy=iy.astype(np.intp))
    return EyeFoldDensity(grid=grid, counts=counts, **out)


def eye_fold_density(eye_obj, *, colors=False, hist=None):
    """The computed part of ``eye.plot`` (reference ``typing.py:2718-2788``), like :func:`eye_density` is of ``eyediagram``: the eye's record
    ``y`` without its first ``sps`` samples, folded over the eye's time grid of period ``2 (sps_resamp or sps)``; the result holds
    ``np.histogram2d(t_, y_, bins=350)``, its ``gaussian_filter(sigma=3)``, with ``colors=True`` the drawn points (``n_traces = len(y_) // (2 sps)``
    traces of ``2 sps`` points) with their grid indices and their grid values, normalised over all points, and with ``hist=(lo, hi)``
    ``np.histogram(bins=200)`` of the points whose abscissa lies strictly between ``lo`` and ``hi``.  Returns an :class:`EyeFoldDensity`.

    A record that ``GET_EYE`` left in GPU memory is computed there (``ssfm_eye_fold_range``, ``ssfm_eye_fold_density``) and stays there: only the
    results come back.  A record on the host (after ``eye.y`` was read) is NumPy / SciPy on the host and loads no device.

    Raises ``ValueError('Empty eye diagram object.')`` for an eye without record or ``t_opt``, and NumPy's ("autodetected range of [...] is not
    finite") for a NaN or an infinity among the plotted points."""
    y, sps, count, P, L, n_draw, tg = _eye_plot_fold(eye_obj)
    if hist is not None:
        hist = (float(hist[0]), float(hist[1]))
    if _is_device(y):
        if np.dtype(y.dtype) != np.dtype(np.float64):
            raise TypeError(f"the eye diagram takes a float64 device array, not {y.dtype}")
        return _eye_fold_density_device(y, sps, count, L, n_draw, tg, colors, hist)
    return _eye_fold_density_host(y, sps, count, L, n_draw, tg, colors, hist)


__all__ = ["get_psd", "eye_density", "eyediagram", "EyeDensity", "eye_fold_density", "EyeFoldDensity"]
