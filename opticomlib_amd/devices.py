"""``FIBER`` / ``DBP`` / ``DM`` with the reference's call signatures, running on MI355X.

Host-side mirror of reference ``opticomlib/devices.py:1038-1206`` (FIBER), ``:1209-1283``
(DBP) and ``:945-1035`` (DM): same argument names, defaults, units, return types and the
same ``TypeError``.  All field arithmetic happens in the HIP library behind the C ABI
(``include/ssfm_amd.h``); this module only prepares the O(N) operator coefficients and the
float32 step schedule exactly the way the reference's prologue does, and wraps the result.

There is deliberately NO CPU fallback: sizes the HIP path does not cover raise
``ValueError``; a missing library or device raises ``SsfmError``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import functools
import time
import warnings
from collections import OrderedDict, namedtuple

import numpy as np

from . import _lib, accuracy
from .typing import _C_LIGHT, NULL, binary_sequence, electrical_signal, eye, gv, optical_signal

_F32 = np.float32
_CACHE_LOCK = threading.RLock()       # guards the module's small caches (plans, operators, grid powers, chirps) against concurrent callers
_PLANS: "OrderedDict[tuple, _lib.Plan]" = OrderedDict()
_MAX_PLANS = 12           # a 2^20 x 2 plan holds ~0.1 GB of the 288 GB; a link script cycles through a handful of shapes


def default_device() -> int:
    """Device index of this process: ``LOCAL_RANK`` under torchrun, else 0."""
    return int(os.environ.get("LOCAL_RANK", "0")) % max(_lib.device_count(), 1)


def get_plan(n: int, batch: int, precision: int, device=None) -> _lib.Plan:
    """Plans own all device buffers; keep the few most recent ones alive.

    Eviction only DROPS the cache's reference: the plan's buffers are freed when its last user lets go of it
    (``Plan.__del__``), never under a thread that was handed the plan a moment ago and has not taken its lock yet."""
    device = default_device() if device is None else int(device)
    key = (device, int(n), int(batch), int(precision))
    with _CACHE_LOCK:
        plan = _PLANS.pop(key, None)
        if plan is None or plan.closed:
            plan = _lib.Plan(n, batch, precision, device)
        _PLANS[key] = plan
        while len(_PLANS) > _MAX_PLANS:
            _PLANS.popitem(last=False)
    return plan


def release_plans():
    with _CACHE_LOCK:
        plans = list(_PLANS.values())
        _PLANS.clear()
    for p in plans:
        with p.lock:
            p.close()


def _tag(*key) -> int:
    """Non-zero 64-bit label of what a caller stages in a plan (``Plan.set_tag`` / ``Plan.tag``): the plan itself
    clears the label whenever the buffer is overwritten, so a matching label means the content is still there.

    A digest of the exact values, NOT Python's ``hash``: ``hash(-1.0) == hash(-2.0)`` in CPython, so a hash-labelled
    plan took ``FIBER(beta_2=-2)`` for the ``FIBER(beta_2=-1)`` it had staged.  Floats enter by their bit patterns
    (``-0.0`` and ``0.0``, ``1`` and ``1.0`` are different keys: a spurious miss only re-stages)."""
    import hashlib
    import struct
    h = hashlib.blake2b(digest_size=8)
    for k in key:
        if isinstance(k, float):
            h.update(b"f" + struct.pack("<d", k))
        elif isinstance(k, (int, np.integer)):
            h.update(b"i" + int(k).to_bytes(16, "little", signed=True))
        elif isinstance(k, str):
            h.update(b"s" + k.encode() + b"\0")
        else:
            raise TypeError(f"_tag: unsupported key component {type(k).__name__}")
    return int.from_bytes(h.digest(), "little") | 1


def _is_fast_size(n: int, precision: int) -> bool:
    """Power of two within the fused two-kernel engine's range."""
    lo, hi = _lib.supported_log2n(precision)
    return (1 << lo) <= n <= (1 << hi) and n & (n - 1) == 0


def _check_size(n: int, precision: int):
    """Any length from 2 up to 2^21 samples per polarisation runs on the GPU, and powers of two up to 2^24: powers of two in [2^8, 2^22] through
    the fused engine, 2^23 and 2^24 as split plans (round 6), every other length through the chirp-z path on a power-of-two plan of >= 2n - 1 <= 2^22 points."""
    if _is_fast_size(n, precision):
        return
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    _, top = _lib.supported_log2n(_lib.C128)
    if n < 2 or 2 * n - 1 > (1 << hi):
        raise ValueError(
            f"the MI355X fibre path takes 2 ... 2^{hi - 1} samples per polarisation (powers of two up to 2^{top}), "
            f"got {n} (there is no CPU fallback)")


def _precision_code(precision) -> int:
    p = np.dtype(precision)
    if p == np.complex64:
        return _lib.C64
    if p == np.complex128:
        return _lib.C128
    raise ValueError("precision must be complex64 or complex128")


# ------------------------------------------------------------------ device residency
# Results of FIBER / DBP / DM / BPF / LPF stay in GPU memory (``signal`` / ``noise`` backed by a
# ``_lib.DeviceArray``) until somebody reads them on the host; the next device call of a chain takes them
# from there.  ``KEEP_ON_DEVICE = False`` restores eager host arrays.
KEEP_ON_DEVICE = True


def _on_device(a) -> bool:
    return isinstance(a, _lib.DeviceArray)


def _dev_array(x, dtype, dev: int) -> "_lib.DeviceArray":
    """``x`` (host array or DeviceArray) as a DeviceArray of ``dtype`` on GPU ``dev``; no transfer and no
    copy when it already is one."""
    dtype = np.dtype(dtype)
    if _on_device(x):
        if x.device != dev:                                 # other GPU: through the host
            return _lib.DeviceArray.from_host(x.to_host(), dtype, dev)
        return x if x.dtype == dtype else x.astype(dtype)
    return _lib.DeviceArray.from_host(np.asarray(x), dtype, dev)


def _stack_rows(arrays, dtype, dev: int, shape=None) -> "_lib.DeviceArray":
    """``arrays`` (host arrays or DeviceArrays of one shape, ``(rows, n)`` or ``(n,)``) one after the other in ONE new device buffer of
    ``dtype`` on GPU ``dev``: ``(k rows, n)`` for k arrays, or ``shape`` when given (blocks beyond the arrays are left unset)."""
    if shape is None:
        shape = (len(arrays) * int(np.prod(arrays[0].shape[:-1], dtype=np.int64)), arrays[0].shape[-1])
    buf = _lib.DeviceArray(shape, dtype, dev)
    for k, a in enumerate(arrays):
        d = _dev_array(a, dtype, dev)
        if (k + 1) * d.nbytes > buf.nbytes:
            raise ValueError(f"{len(arrays)} arrays of {d.shape} do not fit a buffer of {buf.shape}")
        _lib.api.ssfm_device_copy(dev, buf.ptr + k * d.nbytes, d, d.nbytes, _lib.COPY_D2D)
    return buf


def _row_block(buf: "_lib.DeviceArray", k: int, shape) -> "_lib.DeviceArray":
    """Block ``k`` of a :func:`_stack_rows` buffer of arrays of ``shape``, as a new DeviceArray of that shape."""
    out = _lib.DeviceArray(shape, buf.dtype, buf.device)
    if (k + 1) * out.nbytes > buf.nbytes:
        raise ValueError(f"block {k} of {shape} lies beyond a buffer of {buf.shape}")
    _lib.api.ssfm_device_copy(buf.device, out, buf.ptr + k * out.nbytes, out.nbytes, _lib.COPY_D2D)
    return out


def _wrap_out(cls, sig, noi, **kw):
    """Signal object around device results; materialised at once when KEEP_ON_DEVICE is off."""
    out = cls.from_device(sig, noi, **kw)
    if not KEEP_ON_DEVICE:
        out.signal, out.noise                               # noqa: B018 -- the attribute reads download
    return out


# ------------------------------------------------------------------ signals of the reference library itself
# A script written against opticomlib can swap single devices: `from opticomlib_amd import FIBER` and keep
# opticomlib's own PRBS / DAC / MZM / DSP around it.  Its signal objects are recognised by layout (class name,
# `.signal`, `.noise`), the sampling grid is read from THAT library's `gv` (the one the script configured), and
# the result is handed back as an object of the caller's class, so the next opticomlib device accepts it.
def _adopt(input, kind: str):
    """-> (our signal object, sampling grid, back) ; ``back(result)`` converts to the caller's class.

    ``kind``: 'optical_signal' or 'electrical_signal'.  Our own objects pass through with the global ``gv``."""
    ours = optical_signal if kind == "optical_signal" else electrical_signal
    if isinstance(input, ours):
        return input, gv, lambda out: out
    if type(input).__name__ != kind or not hasattr(input, "signal") or not hasattr(input, "noise"):
        return input, gv, lambda out: out                  # not a signal: the device raises its TypeError
    import sys
    mod = sys.modules.get(type(input).__module__)
    grid = getattr(mod, "gv", None)
    if grid is None or not all(hasattr(grid, a) for a in ("fs", "dt")):
        raise TypeError(f"cannot find the sampling grid (`gv`) of {type(input).__module__}")
    noise = input.noise if isinstance(input.noise, np.ndarray) else NULL
    mine = ours(np.asarray(input.signal), noise)
    if kind == "optical_signal" and mine.n_pol != getattr(input, "n_pol", mine.n_pol):
        mine = ours(np.asarray(input.signal), noise, n_pol=input.n_pol)

    def back(out):
        if isinstance(out, tuple):                          # (signal, H) or (z, A_z)
            return (back(out[0]),) + tuple(out[1:]) if isinstance(out[0], (optical_signal, electrical_signal)) else out
        cls = getattr(mod, type(out).__name__, None)
        if cls is None:
            return out
        res = cls(out.signal) if out.noise is NULL else cls(out.signal, out.noise)
        res.execution_time = out.execution_time
        return res
    return mine, grid, back


# ------------------------------------------------------------------ operator coefficients
_OPERATORS: "OrderedDict[tuple, np.ndarray]" = OrderedDict()
_MAX_OPERATORS = 4            # 8-16 MiB each at 2^20


def linear_operator(n, dt, alpha, beta_2, beta_3, precision=_lib.C64):
    """D~(w) = -alpha/2 + j beta_2/2 w^2 + j beta_3/6 w^3 in FFT order.

    complex64: every factor is rounded to float32 in the reference's own order
    (``devices.py:1137-1145``) so both sides start from identical coefficients.
    complex128: the float64 form of ``devices.py:2440-2442``.

    The last few operators are kept (read-only): NumPy's ``w**3`` costs ~0.1 s at 2^20 points, and a link
    simulation calls FIBER / DBP with the same fibre again and again.
    """
    key = (int(n), float(dt), float(alpha), float(beta_2), float(beta_3), int(precision))
    with _CACHE_LOCK:
        hit = _OPERATORS.get(key)
        if hit is not None:
            _OPERATORS.move_to_end(key)
            return hit
    d = _linear_operator(n, dt, alpha, beta_2, beta_3, precision)
    d.flags.writeable = False
    with _CACHE_LOCK:
        _OPERATORS[key] = d
        while len(_OPERATORS) > _MAX_OPERATORS:
            _OPERATORS.popitem(last=False)
    return d


_GRID_POWERS: "OrderedDict[tuple, tuple]" = OrderedDict()


def _grid_powers(n, dt, precision):
    """``(w**2, w**3)`` of the angular-frequency grid [rad/ps] in the plan's real type, kept for the last two grids:
    NumPy's ``w**3`` (``pow``) costs 38 ms at 2^20 points -- 12x a whole 100-step propagation -- and depends only on
    the sampling grid, so a sweep over fibre parameters pays it once."""
    key = (int(n), float(dt), int(precision))
    with _CACHE_LOCK:
        hit = _GRID_POWERS.get(key)
        if hit is not None:
            _GRID_POWERS.move_to_end(key)
            return hit
    w = np.fft.fftfreq(n, dt) * 2 * np.pi * 1e-12        # rad/ps
    if precision == _lib.C64:
        w = np.asarray(w, dtype=_F32)
    hit = (w**2, w**3)
    for a in hit:
        a.flags.writeable = False
    with _CACHE_LOCK:
        _GRID_POWERS[key] = hit
        while len(_GRID_POWERS) > 2:
            _GRID_POWERS.popitem(last=False)
    return hit


def _linear_operator(n, dt, alpha, beta_2, beta_3, precision):
    w2, w3 = _grid_powers(n, dt, precision)
    if precision == _lib.C64:
        a = np.array(alpha / 4.343, dtype=_F32)
        b2 = np.array(beta_2, dtype=_F32)
        b3 = np.array(beta_3, dtype=_F32)
        return -a / 2 + 1j / 2 * b2 * w2 + 1j / 6 * b3 * w3
    a = alpha / 4.343
    return -a / 2 + 1j / 2 * beta_2 * w2 + 1j / 6 * beta_3 * w3


def step_schedule(length, h, precision=_lib.C64):
    """Step sizes and positions of a fixed-``h`` run.

    The reference accumulates ``z`` and clamps ``h`` in float32 (``devices.py:1158-1161,
    1173,1196``), which decides the step COUNT (100 km / 0.1 km is 1001 steps); the same
    arithmetic is replayed here.  Returns ``(h[S], z[S+1])`` in the plan's real type.
    """
    rt = _F32 if precision == _lib.C64 else np.float64
    L = rt(length)
    hs = rt(h)
    if not np.isfinite(hs) or hs <= 0:
        raise ValueError(f"h must be a positive step size in km, got {h!r} (the reference never terminates for h <= 0)")
    hcur = min(hs, L)
    z = rt(0)
    hlist, zlist = [], [z]
    while z < L:
        z = rt(z + hcur)
        hlist.append(hcur)
        zlist.append(z)
        hcur = rt(min(hcur, rt(L - z)))
    return np.array(hlist, dtype=rt), np.array(zlist, dtype=rt)


# ------------------------------------------------------------------ chirp-z engine (any length)
_CHIRPS: "OrderedDict[tuple, tuple]" = OrderedDict()      # (device, n) -> (c, conj c) on the device; content-addressed, never stale
_CHIRPS32: "OrderedDict[tuple, object]" = OrderedDict()   # (device, n) -> c in complex64, for the one-launch lines


def _cached(cache: OrderedDict, key, make):
    """``cache[key]``, made by ``make()`` when it is not there; a cache keeps its four newest entries."""
    with _CACHE_LOCK:
        if key not in cache:
            cache[key] = make()
            while len(cache) > 4:
                cache.pop(next(iter(cache)))
        return cache[key]


def _chirp32(dev: int, n: int) -> "_lib.DeviceArray":
    return _cached(_CHIRPS32, (dev, n), lambda: _lib.chirp_device(n, False, dev).astype(np.complex64))


def _rows(shape):
    """``(n, batch)`` of a field of ``shape`` ``(n,)`` or ``(batch, n)``."""
    return shape[-1], (1 if len(shape) == 1 else shape[0])


class _ChirpZ:
    """Split-step / single-transfer engine for fields of ANY length n on a power-of-two complex128 plan of
    M >= 2n - 1 points (Bluestein; algebra in csrc/chirpz.hip).  The field lives in a device array in natural
    order; all arithmetic of THIS engine is complex128 whatever the caller's precision (complex64 callers of up to 2048 samples take
    ``_fiber_chirpz_small_c64`` instead)."""

    def __init__(self, n: int, batch: int, dev: int):
        self.n, self.batch, self.dev = int(n), int(batch), int(dev)
        M = 1 << max(8, (2 * n - 2).bit_length())
        self.plan = get_plan(M, batch, _lib.C128, dev)
        with self.plan.lock:
            self._ensure_tables()
        self.chirp, self.chirp_conj = _cached(_CHIRPS, (dev, n), lambda: (_lib.chirp_device(n, False, dev), _lib.chirp_device(n, True, dev)))

    def _ensure_tables(self):
        want = _tag("chirp", self.n)
        if self.plan.tag(1) != want or self.plan.tag(2) != want:
            # both convolution kernels are generated AND transformed on the device (ssfm_chirp_setup): no host FFT, no upload
            self.plan.chirp_setup(self.n)
            for slot in (0, 1):
                self.plan.set_tag(1 + slot, want)

    # the engine works in the plan's field buffer and table slots: its users hold the plan's lock for their whole sequence
    def __enter__(self):
        self.plan.lock.acquire()
        self._ensure_tables()
        return self

    def __exit__(self, *exc):
        self.plan.lock.release()
        return False

    def transfer(self, A, H, exponent=False):
        """``A <- ifft(fft(A) * H)`` (or ``* exp(H)`` with ``exponent``) for a device table ``H`` of n entries, in place."""
        self.plan.chirp_transfer(A, self.chirp, H, exponent)

    def fourier(self, A, inverse: bool):
        """``fft`` (or ``ifft``) of every row of the device array ``A`` (batch, n), in place; returns ``A``."""
        self.plan.chirp_fourier(A, self.chirp, self.chirp_conj, inverse)
        self.plan.synchronize()
        return A


def _chirpz_transfer(raws, H, exponent: bool, dev: int):
    """``ifft(fft(x) H)`` (or ``* exp(H)`` with ``exponent``) of every row of the arrays ``raws`` (signal, then noise: one shape) on the
    chirp-z engine (any length): the rows stacked in one buffer, transformed in place, split back into new device arrays of that shape."""
    shape = tuple(raws[0].shape)
    buf = _stack_rows(raws, np.complex128, dev)
    with _ChirpZ(shape[-1], buf.shape[0], dev) as eng:
        eng.transfer(buf, H, exponent=exponent)
        eng.plan.synchronize()
    return [_row_block(buf, k, shape) for k in range(len(raws))]


def _fourier(obj, domain, shift=False):
    """``signal('w')`` / ``signal('t')`` of the reference's signal classes (``typing.py:1421-1462``): fft or ifft of
    signal and noise along the last axis -- on the device, for any length from 2 to 2^21 (complex128 chirp-z
    transform), the result stays in GPU memory.  ``shift`` applies fftshift / ifftshift (two device copies per row)."""
    if domain not in ("t", "w", "f"):
        raise ValueError("`domain` must be one of the following values ('t', 'w', 'f')")
    inverse = domain == "t"
    dev = default_device()
    raws = [obj._raw("signal")] + ([] if obj._raw("noise") is NULL else [obj._raw("noise")])
    shape = tuple(raws[0].shape)
    n, rows = _rows(shape)
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if n < 2 or 2 * n - 1 > (1 << hi):
        raise ValueError(f"the device transform takes 2 ... 2^{hi - 1} samples per row, got {n} (there is no CPU fallback)")
    single = all(np.dtype(a.dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) for a in raws)   # NumPy >= 2 keeps single precision
    buf = _stack_rows(raws, np.complex128, dev)
    with _ChirpZ(n, buf.shape[0], dev) as eng:
        res = eng.fourier(buf, inverse)
    cp = lambda dst, src, nbytes: _lib.api.ssfm_device_copy(dev, dst, src, nbytes, _lib.COPY_D2D)
    outs = []
    s_ = n // 2
    for k in range(len(raws)):
        if not shift:
            o = _row_block(res, k, shape)
        else:
            o = _lib.DeviceArray(shape, np.complex128, dev)
            for r in range(rows):
                src, dst = res.ptr + (k * rows + r) * n * 16, o.ptr + r * n * 16
                if not inverse:                                 # fftshift: out[(i + n//2) % n] = in[i]
                    cp(dst + s_ * 16, src, (n - s_) * 16)
                    cp(dst, src + (n - s_) * 16, s_ * 16)
                else:                                           # ifftshift: out[i] = in[(i + n//2) % n]
                    cp(dst, src + s_ * 16, (n - s_) * 16)
                    cp(dst + (n - s_) * 16, src, s_ * 16)
        outs.append(o.astype(np.complex64) if single else o)
    kw = {"n_pol": obj.n_pol} if isinstance(obj, optical_signal) else {}
    return _wrap_out(type(obj), outs[0], outs[1] if len(outs) > 1 else NULL, **kw)


class _Fibre(namedtuple("_Fibre", "length alpha beta_2 beta_3 gamma phi_max h dt prec rt L g single")):
    """The fibre of one ``FIBER`` call as the caller gave it (``prec``: the plan's precision code) and, worked out once by :meth:`of`, what every engine
    derives from it in the caller's arithmetic ``rt`` (float32 in complex64 mode: reference devices.py:1137-1161): ``L`` and ``g`` are length and gamma
    in it, ``single`` says that the adaptive rule (``h`` is None) has nothing to adapt to -- one step of the whole length (reference devices.py:1163-1170)."""
    __slots__ = ()

    @classmethod
    def of(cls, length, alpha, beta_2, beta_3, gamma, phi_max, h, dt, prec):
        rt = _F32 if prec == _lib.C64 else np.float64
        single = False
        if h is None:
            b2, b3 = rt(beta_2), rt(beta_3)
            single = bool((b2 == 0 and b3 == 0) or rt(gamma) == 0)
        return cls(length, alpha, beta_2, beta_3, gamma, phi_max, h, dt, prec, rt, rt(length), float(rt(gamma)), single)

    def schedule(self):
        return step_schedule(self.length, self.h, self.prec)

    def known_run(self):
        """``(hs float64, zs)`` of a run whose steps are known beforehand -- a fixed ``h``, or one step of the whole length -- and None for one
        that the adaptive rule steps through."""
        if self.h is None:
            return (np.array([float(self.L)]), [self.rt(0), self.L]) if self.single else None
        hs, z = step_schedule(self.length, self.h, self.prec)
        return np.asarray(hs, dtype=np.float64), list(z)

    def operator(self, n: int):
        return linear_operator(n, self.dt, self.alpha, self.beta_2, self.beta_3, self.prec)


def _fiber_chirpz(fibre, A_dev, n, batch, return_steps, dev, bar):
    """FIBER for a length that is not a power of two (same semantics as the fused engine: float32 coefficients
    and step arithmetic in complex64 mode, reference devices.py:1137-1161, 1172-1196)."""
    if fibre.prec == _lib.C64 and n <= 2048 and not return_steps and bar is None and os.environ.get("SSFM_CHIRP_LOOP", "c") != "python" \
            and os.environ.get("SSFM_CHIRP_SMALL", "1") != "0" and batch <= 16:
        got = _fiber_chirpz_small_c64(fibre, A_dev, n, batch, dev)
        if got is not None:
            return got + ("chirp_small_c64",)
    if fibre.prec == _lib.C64 and 2048 < n <= 65536 and not return_steps and bar is None and os.environ.get("SSFM_CHIRP_LOOP", "c") != "python" \
            and os.environ.get("SSFM_MEDIUM", "1") != "0":
        got = _fiber_chirpz_medium_c64(fibre, A_dev, n, batch, dev)
        if got is not None:
            return got + ("chirp_medium_c64",)
    with _ChirpZ(n, batch, dev) as eng:
        return _fiber_chirpz_locked(eng, fibre, A_dev, n, batch, return_steps, dev, bar) + ("chirp_line_c128",)


# Accuracy margin of the one-launch complex64 chirp-z line (2048 < n <= 65536; profiles/r05_chirp_margin.txt).  A step of that line is four
# padded complex64 transforms of 2-4 x the field's length where the reference's pocketfft makes two of the length itself: measured over 242 random
# fibres, max|A - A_float64|/peak <= 7.5e-7 x steps^0.75.  The reference's own complex64 run sits up to the tolerance itself from the float64
# solution for such lengths, so the line may use HALF of the stated bound -- `accuracy.tol(steps)`, ONE bound continuous in the number of steps
# (2e-5 up to 100 steps, the log-log line to 3e-4 at 1000, proportional beyond).  Where the law exceeds half the bound the run takes the complex128
# line (four launches per step, 1e-13 from float64): 27 ... 1031 steps, DERIVED from the law and the bound (`accuracy.c64_line_window`).  Round 5's
# window, 32 ... 100, was fitted to the step at 101 steps of the tolerance the tests then used (2e-5 up to 100 steps, 3e-4 from 101): a 101-step
# run is 2.4e-5 from the float64 solution by the line's own law.  `precision="complex128"` always takes the complex128 line.
_c64_line_has_margin = accuracy.c64_line_has_margin
_C64_LINE_NO_MARGIN = accuracy.c64_line_window()          # (first, last) step count without margin: (27, 1031)


def _prepare_c64(fibre, A_dev, n, batch, dev):
    """What a one-launch complex64 line works on: ``(A, chirp, Dt, g)`` -- the field as a new (batch, n) complex64 array, the line's chirp, the
    operator on the device, gamma in the caller's arithmetic."""
    chirp = _chirp32(dev, n)
    A = A_dev.astype(np.complex64)                          # (a copy when it has the type already: the caller's array is never modified)
    A.shape = (batch, n)
    Dt = _lib.DeviceArray.from_host(np.asarray(fibre.operator(n), dtype=np.complex64), np.complex64, dev)
    return A, chirp, Dt, fibre.g


def _prepare_c128(fibre, A_dev, n, batch, dev):
    """The same for the complex128 line: ``(A, P, Dt, g)``, ``P`` its (batch, n) buffer of powers."""
    A = A_dev.astype(np.complex128)                         # (a copy when it has the type already: the caller's array is never modified)
    A.shape = (batch, n)
    P = _lib.DeviceArray((batch, n), np.float64, dev)
    Dt = _lib.DeviceArray.from_host(np.asarray(fibre.operator(n), dtype=np.complex128), np.complex128, dev)
    return A, P, Dt, fibre.g


def _raise_chirp_midway():
    raise _lib.SsfmError("the one-launch chirp-z engine lost its workgroups in the middle of a run of more than 131072 steps")


def _adaptive_run(run, L, rt, max_steps=1 << 17, after=None):
    """An adaptive run over the length ``L`` in the arithmetic ``rt``, at most ``max_steps`` steps per call: ``run(length=left, max_steps=k)`` advances the
    field and returns ``(steps, z)``, ``z`` counted from where it started (``after(z)`` follows it), or None when its engine could not run.  One call
    unless a run needs more than 131072 steps: then it goes on from where it is.  Returns the positions from 0 on; None when the first call gave up."""
    zs, z0 = [rt(0)], rt(0)
    while True:
        got = run(length=float(rt(L - z0)), max_steps=max_steps)
        if got is None:
            return None if z0 == 0 else _raise_chirp_midway()
        steps, z = got
        zs += [rt(z0 + rt(v)) for v in z[1:]]
        if after is not None:
            after(z)
        if steps < max_steps or not (zs[-1] < L):
            return zs
        z0 = zs[-1]


def _fiber_chirpz_small_c64(fibre, A_dev, n, batch, dev):
    """``precision="complex64"`` at up to 2048 samples that are not a power of two: the whole run in ONE launch on a complex64 line of M >= 2n - 1 <= 4096 points
    (k_small_chirp / k_small_chirp_adapt instantiated for float; round 4).  The reference itself transforms such a length in single precision (pocketfft's Bluestein,
    devices.py:1178-1180), so this is its arithmetic class: 2e-6 ... 7e-6 from the float64 solution after 100 steps (profiles/r04_chirpz_c64_error.txt) where the
    complex128 line of the general path sits at 1e-13 -- and a step takes half the time (one CU does the four line transforms of a step; float64 was its bound).
    ``precision="complex128"`` keeps the complex128 line.  None: the plan has no such engine, or its rows' workgroups did not meet: the general path runs."""
    M = 1 << max(8, (2 * n - 2).bit_length())
    plan = get_plan(M, batch, _lib.C64, dev)
    L = _F32(fibre.length)
    if not float(L) > 0:
        return A_dev.astype(np.complex64), [_F32(0)], None       # (a copy when it has the type already)
    with plan.lock:
        A, chirp, Dt, g = _prepare_c64(fibre, A_dev, n, batch, dev)
        known = fibre.known_run()
        if known is not None:
            hs, zs = known
            if not plan.chirp_propagate_c64(A, chirp, Dt, g, hs):
                return None
        else:
            phi = float(_F32(fibre.phi_max))
            zs = _adaptive_run(functools.partial(plan.chirp_propagate_c64, A, chirp, Dt, g, None, phi_max=phi), L, _F32)
            if zs is None:
                return None
        plan.synchronize()
        return A, zs, None


def _fiber_chirpz_medium_c64(fibre, A_dev, n, batch, dev):
    """``precision="complex64"``, 2048 < n <= 65536 samples that are not a power of two: the whole run in one launch on one XCD on a complex64 line of
    M >= 2n - 1 points, 2^13 ... 2^17 (k_medium_chirp / k_medium_chirp_adapt: four passes per step instead of five / seven launches; round 4).  The arithmetic
    class of ``_fiber_chirpz_small_c64``.  None: a plan whose rows do not fit the one-XCD engine (2^17 points in all), more than four step sizes, or a launch
    whose workgroups did not meet: the general path runs."""
    M = 1 << (2 * n - 2).bit_length()
    L = _F32(fibre.length)
    if M * batch > (1 << 17) or not float(L) > 0:
        return None
    known = fibre.known_run()
    if known is None and os.environ.get("SSFM_MEDIUM_ADAPT", "1") == "0":
        return None
    hs, zs = known if known is not None else (np.array([float(L)]), None)    # (an adaptive run counts as one step here; its own count is judged below)
    if len(set(hs.tolist())) > 4 or not _c64_line_has_margin(len(hs)):
        return None
    plan = get_plan(M, batch, _lib.C64, dev)
    with plan.lock:
        A, chirp, Dt, g = _prepare_c64(fibre, A_dev, n, batch, dev)
        if known is not None:
            if not plan.chirp_propagate_c64(A, chirp, Dt, g, hs):
                return None
            return A, zs, None
        # adaptive: the step count is the run's own.  One step on a copy gives the first step size; the run's length in steps follows from it
        # (h grows as the power falls: steps ~ L_eff / h0) -- a run that will end inside the window without margin goes to the complex128 line at once
        phi = float(_F32(fibre.phi_max))
        probe = A.copy()
        got = plan.chirp_propagate_c64(probe, chirp, Dt, g, None, length=float(L), phi_max=phi, max_steps=1)
        if got is None:
            return None
        h0 = float(got[1][1]) if got[0] >= 1 else float(L)
        a_lin = float(_F32(fibre.alpha / 4.343))
        x = a_lin * float(L)
        l_eff = float(L) if abs(x) < 1e-6 else float(L) * (1.0 - np.exp(-x)) / x
        est = l_eff / h0 if h0 > 0 else 1.0
        if 0.85 * _C64_LINE_NO_MARGIN[0] <= est <= 1.15 * _C64_LINE_NO_MARGIN[1]:
            return None
        zs = _adaptive_run(functools.partial(plan.chirp_propagate_c64, A, chirp, Dt, g, None, phi_max=phi), L, _F32)
        if zs is None or not _c64_line_has_margin(len(zs) - 1):              # (the estimate was off: the run is repeated on the complex128 line)
            return None
        return A, zs, None


def _fiber_chirpz_locked(eng, fibre, A_dev, n, batch, return_steps, dev, bar):
    """The complex128 line (the caller holds the engine's plan): the whole run from C (ssfm_chirp_propagate: no host call per kernel, the adaptive step
    rule on the device).  A caller that wants the field after every step (return_steps), a progress bar, or SSFM_CHIRP_LOOP=python gets the same entry
    point a step at a time (one step size, or -- adaptive -- max_steps = 1 over what is left of the length: the step rule is evaluated on the device in
    the caller's arithmetic either way, so the schedule is the whole run's bit for bit)."""
    rt, L = fibre.rt, fibre.L
    f32 = fibre.prec == _lib.C64
    A, P, Dt, g = _prepare_c128(fibre, A_dev, n, batch, dev)
    zs = [rt(0)]
    snaps = [A.copy()] if return_steps else None

    def fixed(hs):
        eng.plan.chirp_propagate(A, P, eng.chirp, Dt, g, hs, f32=f32)

    # over what is left of the length, at most max_steps steps: adaptive(length=..., max_steps=...) -> (steps, z)
    adaptive = functools.partial(eng.plan.chirp_propagate, A, P, eng.chirp, Dt, g, None, phi_max=float(rt(fibre.phi_max)), f32=f32)

    known = fibre.known_run()
    if not return_steps and bar is None and os.environ.get("SSFM_CHIRP_LOOP", "c") != "python":
        if known is not None:
            fixed(known[0])
            zs = known[1]
        elif float(L) > 0:
            zs = _adaptive_run(adaptive, L, rt)           # (this line always runs: never None)
        return A, zs, snaps

    steps = 0

    def after_step(hk):
        nonlocal steps
        steps += 1
        if return_steps:
            snaps.append(A.copy())
        if bar is not None:
            bar.update(min(100.0 * float(hk) / float(L), max(0.0, 100.0 - bar.n)))
            bar.set_postfix(FFTs=2 * steps)

    if fibre.h is not None:
        for hk in known[0]:
            fixed(np.array([float(hk)]))
            after_step(hk)
        zs = known[1]
    elif float(L) > 0:                                      # (the reference's loop, `while z < length`, takes no step of a length <= 0)
        if known is not None:
            fixed(known[0])
            after_step(L)
            zs = known[1]
        else:
            zs = _adaptive_run(adaptive, L, rt, 1, lambda z: after_step(rt(z[1])))
    eng.plan.synchronize()
    return A, zs, snaps


def _progress_bar(show_progress):
    """The reference's tqdm bar, or None: not asked for, or tqdm is not installed."""
    if not show_progress:
        return None
    try:
        from tqdm.auto import tqdm
    except ImportError:
        return None
    return tqdm(total=100, desc="Propagating", bar_format="{l_bar}{bar}|[{elapsed}{postfix}]", postfix={"FFTs": 0})


# ------------------------------------------------------------------ FIBER / DBP
def FIBER(input: optical_signal,
          length: float,
          alpha: float = 0.0,
          beta_2: float = 0.0,
          beta_3: float = 0.0,
          gamma: float = 0.0,
          phi_max: float = 0.01,
          h: float = None,
          show_progress: bool = False,
          return_steps: bool = False,
          *,
          precision="complex64",
          device=None,
          every: int = None,
          z_list=None,
          coupling: str = None,
          kappa: float = None,
          pmd: float = None,
          pmd_seed: int = None,
          pmd_scatter: bool = True):
    """Optical fibre: symmetric split-step Fourier solution of the scalar NLSE per polarisation.

    Parameters as the reference (``devices.py:1038-1083``): ``length`` [km], ``alpha`` [dB/km],
    ``beta_2`` [ps^2/km], ``beta_3`` [ps^3/km], ``gamma`` [1/(W km)], ``phi_max`` [rad] bound of
    the nonlinear phase per adaptive step, ``h`` fixed step [km] or ``None`` for adaptive.
    Returns an :class:`optical_signal` (``noise`` folded into ``signal``, ``noise = NULL``) or,
    with ``return_steps``, ``(z float64 (S+1,), A_z (S+1, [2,] N))``.

    Extensions (keyword-only, defaults keep the reference's behaviour): ``precision``
    ``"complex64"`` (the reference's arithmetic) or ``"complex128"``; ``device`` index; ``every``
    (with ``return_steps`` and a fixed ``h`` on a power-of-two length): keep the field after every
    ``every``-th step only (plus the input and the last step) -- the run stays on the fused engine and the
    snapshots travel to page-locked host memory beside it (``ssfm_propagate_fixed_capture``); the reference
    keeps every step, 16 GiB for the 1000-step run of a 2^20-sample dual-polarisation field.  With the adaptive step
    (``h=None``, the reference's default and what its own consumer of ``return_steps`` uses, ``devices.py:2342``) ``every`` and
    ``z_list`` (round 6) keep the run's own engine as well (``ssfm_adaptive_set_capture``): ``z_list`` = positions [km] -- for each
    the field after the first step that reaches it (the input for z <= 0, the end field beyond the length).  The run is
    made twice: once for its z log (an adaptive run repeats bit for bit), once with the capture at the steps that follow from it.

    ``coupling`` (keyword-only): ``None`` -- the reference's behaviour: the two polarisations of a ``(2, N)`` field are two scalar fibres that share
    only the adaptive step size -- or ``"manakov"``: the nonlinear phase of BOTH polarisations follows the power in both,
    ``exp(1j * gamma * kappa * (|A_x|^2 + |A_y|^2) * h / 2)`` per half step, the Manakov equation of a fibre whose birefringence scrambles the
    polarisation state (``kappa`` defaults to 8/9; ``kappa=1`` is the coupled equation without the averaging).  Everything else -- the stale power
    over a step, the coefficient rounding, the step rule ``h = phi_max / max(|gamma kappa| P)`` -- is the reference's loop.  For ``(2, N)`` fields
    of a power-of-two length up to 2^22 (:func:`_fiber_manakov`).

    ``pmd`` (keyword-only, with ``coupling="manakov"``): the PMD coefficient ``D_p`` [ps/sqrt(km)], finite and >= 0 -- the Manakov-PMD equation in the
    coarse-step (waveplate) model with ONE SECTION PER STEP: behind its opening half rotation step ``k`` of size ``h`` turns the axes by the random
    unitary ``U_k`` of :func:`pmd_sections` ``(pmd_seed, count)`` (Haar on SU(2); not with ``pmd_scatter=False``: the axes stay and the run is a pure
    differential delay), and its linear operator delays row 0 by ``tau / 2`` and advances row 1 by ``tau / 2``, ``tau = D_p sqrt(h)`` [ps].  A fixed-step
    run draws one unitary per step, and with an equal step ``h`` the rms differential group delay of ``L`` km is ``D_p sqrt(L)``; the adaptive run draws
    its ``max_steps`` unitaries once and its section lengths FOLLOW THE STEPS, so its delay statistics depend on the power through the step rule.
    ``pmd_seed=None`` picks a seed; the result reports the seed it ran with as ``output.pmd_seed`` and the engine as ``"manakov_pmd_line"``.
    ``pmd=None`` is the ideal fibre above.  Not for ``DBP``: back-propagation cannot know the fibre's random axes.
    """
    t0 = time.time()
    if coupling is not None and coupling != "manakov":
        raise ValueError(f"coupling must be None (per polarisation) or 'manakov', got {coupling!r}")
    if coupling is None and kappa is not None:
        raise ValueError("kappa belongs to coupling='manakov'")
    pmd = _check_pmd(coupling, pmd, pmd_seed, pmd_scatter)
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    prec = _precision_code(precision)
    plan_dtype = np.complex64 if prec == _lib.C64 else np.complex128

    raw_s, raw_n = input._raw("signal"), input._raw("noise")
    dev = default_device() if device is None else int(device)
    A = A_dev = None
    if _on_device(raw_s) or _on_device(raw_n):
        # signal + noise in their common type, then the cast -- NumPy's own order (devices.py:1147)
        if raw_n is NULL:
            A_dev = _dev_array(raw_s, plan_dtype, dev)
        else:
            common = np.result_type(raw_s.dtype, raw_n.dtype, np.complex64)
            total = _dev_array(raw_s, common, dev) + _dev_array(raw_n, common, dev)
            A_dev = total if total.dtype == plan_dtype else total.astype(plan_dtype)
        shape = tuple(A_dev.shape)
    else:
        A = np.asarray(input.to_numpy())
        shape = A.shape
    n, batch = _rows(shape)
    if coupling is not None:
        kappa = _check_manakov(shape, prec, kappa)
    fast = _is_fast_size(n, prec)
    if not fast:
        _check_size(n, prec)
    fibre = _Fibre.of(length, alpha, beta_2, beta_3, gamma, phi_max, h, float(grid.dt), prec)
    if A is not None and fast:
        if A.dtype == np.complex128 and plan_dtype == np.complex64 and A.flags.c_contiguous:
            # the usual case (NumPy signals are complex128): upload as it lies and round to complex64 on the
            # device -- the same round-to-nearest cast, without a 32 -> 16 MiB conversion pass on the host
            A_dev = _lib.DeviceArray.from_host(A, np.complex128, dev).astype(np.complex64)
        else:
            A = np.ascontiguousarray(A, dtype=plan_dtype)

    if not fast:
        # any other length: chirp-z path on a power-of-two plan of >= 2n - 1 points (complex128 arithmetic; complex64 for complex64 callers of up to 2048 samples)
        bar = _progress_bar(show_progress)
        if A_dev is None:
            A_dev = _lib.DeviceArray.from_host(np.ascontiguousarray(A, dtype=np.complex128), np.complex128, dev)
        out, zs, snaps, engine = _fiber_chirpz(fibre, A_dev, n, batch, return_steps, dev, bar)
        if bar is not None:
            bar.close()
        if return_steps:
            if every is not None:
                _lib.check_every(every)                  # (rejected on this path even where `z_list` decides)
            keep = _keep_indices(zs, len(snaps), every, z_list)
            A_z = np.stack([snaps[k].to_host() for k in keep]).astype(plan_dtype).reshape((len(keep),) + tuple(shape))
            return np.asarray(zs, dtype=np.float64)[keep], A_z
        res = out if out.dtype == plan_dtype else out.astype(plan_dtype)
        res.shape = tuple(shape)
        output = _wrap_out(optical_signal, res, NULL)
        output.execution_time = time.time() - t0
        output.engine = engine                                # which chirp-z line ran: "chirp_small_c64", "chirp_medium_c64" (one launch, complex64) or "chirp_line_c128"
        return back(output)

    plan = get_plan(n, batch, prec, dev)
    with plan.lock:
        if coupling is not None:
            output = _fiber_manakov(plan, fibre, kappa, A if A_dev is None else A_dev, shape, show_progress, return_steps, every, z_list, pmd)
        else:
            output = _fiber_on_plan(plan, fibre, A if A_dev is None else A_dev, shape, show_progress, return_steps, every, z_list)
        if not return_steps:
            output.execution_time = time.time() - t0
        return back(output)


MANAKOV_KAPPA = 8.0 / 9.0
_MANAKOV_LOG2_MAX = _lib.DIRECT_LOG2_MAX          # no split plans


def _check_manakov(shape, prec: int, kappa) -> float:
    """What ``coupling="manakov"`` takes, checked before anything touches the GPU; returns kappa (8/9 when None)."""
    n = int(shape[-1])
    if len(shape) != 2 or shape[0] != 2:
        raise ValueError(f"coupling='manakov' is not supported for a field of shape {tuple(shape)}: it couples the two polarisations of a (2, N) field "
                         f"(batches of coupled fields are not supported either)")
    if not _is_fast_size(n, prec) or n > (1 << _MANAKOV_LOG2_MAX):
        raise ValueError(f"coupling='manakov' is not supported for {n} samples per polarisation: a power of two from 2^8 to 2^{_MANAKOV_LOG2_MAX} is needed")
    kappa = MANAKOV_KAPPA if kappa is None else float(kappa)
    if not np.isfinite(kappa) or kappa <= 0:
        raise ValueError(f"coupling='manakov' is not supported for kappa = {kappa!r}: a finite positive factor is needed")
    return kappa


def _check_pmd(coupling, pmd, pmd_seed, pmd_scatter):
    """What ``pmd=`` takes, checked before anything touches the GPU; returns None (no PMD) or ``(D_p, seed, scatter)`` with the seed chosen."""
    if pmd is None:
        if pmd_seed is not None or pmd_scatter is not True:
            raise ValueError("pmd_seed and pmd_scatter belong to pmd=")
        return None
    if coupling != "manakov":
        raise ValueError("pmd needs coupling='manakov': PMD is an impairment of the coupled polarisations")
    try:
        dp = float(pmd)
    except (TypeError, ValueError):
        raise ValueError(f"pmd must be a finite coefficient >= 0 in ps/sqrt(km), got {pmd!r}") from None
    if not np.isfinite(dp) or dp < 0:
        raise ValueError(f"pmd must be a finite coefficient >= 0 in ps/sqrt(km), got {pmd!r}")
    if pmd_seed is None:
        pmd_seed = int(np.random.SeedSequence().generate_state(1)[0])
    return dp, int(pmd_seed), bool(pmd_scatter)


def pmd_sections(seed, count):
    """The ``count`` random waveplates of a PMD run, ``(count, 2, 2)`` complex128: a point of the unit 3-sphere per section --
    ``q = default_rng(seed).standard_normal((count, 4))``, every row scaled to unit length -- read as ``a = q0 + 1j q1``, ``b = q2 + 1j q3``,
    ``U = [[a, b], [-conj(b), conj(a)]]``: Haar-distributed on SU(2).  The first sections of a longer draw are the shorter draw's."""
    q = np.random.default_rng(seed).standard_normal((int(count), 4))
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    a, b = q[:, 0] + 1j * q[:, 1], q[:, 2] + 1j * q[:, 3]
    U = np.empty((int(count), 2, 2), dtype=np.complex128)
    U[:, 0, 0], U[:, 0, 1], U[:, 1, 0], U[:, 1, 1] = a, b, -np.conj(b), np.conj(a)
    return U


def _grid_w(n, dt, precision):
    """The angular-frequency grid [rad/ps] of :func:`_grid_powers`, FFT order, in the plan's real type."""
    w = np.fft.fftfreq(n, dt) * 2 * np.pi * 1e-12
    return np.asarray(w, dtype=_F32) if precision == _lib.C64 else w


def _fiber_manakov(plan, fibre, kappa: float, field, shape, show_progress, return_steps, every=None, z_list=None, pmd=None):
    """``FIBER(coupling="manakov")`` on a power-of-two plan of two rows (the caller holds its lock): the Manakov line of csrc/manakov.hip -- a pointwise
    launch over both rows and the plan's table transform per step, the adaptive step rule on the device.  ``field``: the input, a host array or a
    device array of the plan's type.  Snapshots (``return_steps``) are taken on the device beside the run: every ``every``-th step, or every step
    when ``z_list`` picks among them.  ``pmd``: None or ``(D_p, seed, scatter)`` of :func:`_check_pmd` -- the same run through
    ``Plan.manakov_pmd_propagate``, one unitary of :func:`pmd_sections` per step (drawn once for the ``max_steps`` of an adaptive run)."""
    n, batch, rt, L = plan.n, plan.batch, fibre.rt, fibre.L
    if pmd is None:
        run = plan.manakov_propagate
    else:
        dp, seed, scatter = pmd
        w = _grid_w(n, fibre.dt, fibre.prec)

        def run(g, hs, max_steps=1 << 17, **kw):
            count = len(hs) if hs is not None else max_steps
            sections = pmd_sections(seed, count) if scatter else None
            return plan.manakov_pmd_propagate(g, hs, dp=dp, w=w, sections=sections, max_steps=max_steps, **kw)
    g = float(rt(rt(fibre.gamma) * rt(kappa)))
    op_tag = _tag("fibre", fibre.dt, float(fibre.alpha), float(fibre.beta_2), float(fibre.beta_3))
    if plan.tag(0) != op_tag:
        plan.set_linear_operator(fibre.operator(n))
        plan.set_tag(0, op_tag)
    if _on_device(field):
        plan.set_field_device(field.ptr)
    else:
        plan.set_field(field)
    bar = _progress_bar(show_progress)
    if every is not None:
        every = _lib.check_every(every)
    stride = every if (every is not None and z_list is None) else 1
    first = plan.get_field().reshape(1, batch, n) if return_steps else None

    def snapshots(steps_at_most):
        return _lib.DeviceArray((max(1, -(-steps_at_most // stride)), batch, n), plan.cdtype, plan.device) if return_steps else None

    known = fibre.known_run()
    if fibre.h is None and not fibre.single and g == 0.0:
        known = (np.array([float(L)]), [rt(0), L])            # (kappa rounds gamma away: nothing to adapt to, one step as for gamma == 0)
    snaps = None
    if not float(L) > 0:                                       # (the reference's loop, `while z < length`, takes no step)
        steps, z = 0, [rt(0)]
    elif known is not None:
        hs, z = known
        steps = len(hs)
        snaps = snapshots(steps)
        run(g, hs, snaps=snaps, every=stride)
    else:
        max_steps = 1 << 17
        if return_steps:
            # (the snapshot buffer follows the steps the run takes: the run once for its count -- an adaptive run repeats bit for bit --, the input restored)
            x0 = _lib.DeviceArray((batch, n), plan.cdtype, plan.device)
            plan.get_field_device(x0.ptr)
            max_steps, _ = run(g, None, length=fibre.length, phi_max=fibre.phi_max, max_steps=max_steps)
            plan.set_field_device(x0.ptr)
            snaps = snapshots(max_steps)
        steps, z = run(g, None, length=fibre.length, phi_max=fibre.phi_max, max_steps=max_steps, snaps=snaps, every=stride)
    if bar is not None:
        bar.update(100)
        bar.set_postfix(FFTs=2 * int(steps))
        bar.close()

    if return_steps:
        plan.synchronize()
        kept = _lib.every_index(steps, stride if stride > 1 else None)
        fields = np.concatenate([first, snaps.to_host()[: len(kept) - 1]]) if steps else first
        z = np.asarray(z, dtype=np.float64)[kept]
        if z_list is not None:
            keep = _keep_indices(z, fields.shape[0], None, z_list)
            fields, z = fields[keep], z[keep]
        return z, fields.reshape((fields.shape[0],) + tuple(shape))
    if KEEP_ON_DEVICE:
        out = _lib.DeviceArray(shape, plan.cdtype, plan.device)
        plan.get_field_device(out.ptr)
        output = optical_signal.from_device(out)
    else:
        output = optical_signal(plan.get_field().reshape(shape))
    output.engine = plan.last_run_info()["engine"]
    if pmd is not None:
        output.pmd_seed = pmd[1]
    return output


def _keep_indices(z, n_snaps: int, every, z_list):
    """Which of the ``n_snaps`` snapshots of a run (the input, then one per step, at the positions ``z``) a caller keeps: with ``z_list``, for each
    position the first step that reaches it (0: the input; the last: the end field); else what ``every`` keeps."""
    if z_list is None:
        return _lib.every_index(n_snaps - 1, every)
    z = np.asarray(z, dtype=np.float64)
    return [int(min(np.searchsorted(z, v, side="left"), n_snaps - 1)) for v in np.asarray(z_list, dtype=np.float64).ravel()]


def _adaptive_capture(plan, fibre, every, z_list):
    """``FIBER(h=None, return_steps=True, every=k | z_list=[...])`` on a power-of-two plan: the run once for its z log, the input restored, the run again
    with the capture at the step numbers that follow (``Plan.propagate_adaptive_capture``).  Returns (z of the kept snapshots, snapshots)."""
    n, batch, run = plan.n, plan.batch, (fibre.gamma, fibre.length, fibre.phi_max)
    x0 = _lib.DeviceArray((batch, n), plan.cdtype, plan.device)
    plan.get_field_device(x0.ptr)
    first = plan.get_field().reshape(1, batch, n)
    # (the first pass on the engine the capture will run on: a capture that never fires -- the one-launch engines of the small plans find their
    # step sizes in another order of operations, and their z log differs from the launch-per-pass engines' in the last bits)
    steps, z, _, _ = plan.propagate_adaptive_capture(*run, steps=np.array([1 << 40], dtype=np.int64))
    keep = _keep_indices(z, steps + 1, every, z_list)
    want = sorted({k for k in keep if 0 < k < steps})
    got = {0: first[0]}
    if want:
        plan.set_field_device(x0.ptr)
        steps2, z2, taken, fields = plan.propagate_adaptive_capture(*run, steps=np.asarray(want, dtype=np.int64))
        if steps2 != steps or not np.array_equal(z2, z) or list(taken) != want:
            raise _lib.SsfmError(f"the adaptive run did not repeat ({steps} / {steps2} steps, {len(taken)} of {len(want)} snapshots)")
        for k, f in zip(want, fields):
            got[k] = f
    got[steps] = plan.get_field().reshape(batch, n) if steps else first[0]
    return np.asarray(z)[keep], np.stack([got[k] for k in keep])


def _fiber_on_plan(plan, fibre, field, shape, show_progress, return_steps, every=None, z_list=None):
    """The fused two-kernel engine behind ``FIBER`` (the caller holds the plan's lock for the whole sequence).  ``field``: the input, a host array
    or a device array of the plan's type."""
    n, batch = plan.n, plan.batch
    gamma, L = fibre.gamma, fibre.L
    op_tag = _tag("fibre", fibre.dt, float(fibre.alpha), float(fibre.beta_2), float(fibre.beta_3))
    if plan.tag(0) != op_tag:                             # D~ is O(N) host work + an upload: reuse it while the plan still holds it
        plan.set_linear_operator(fibre.operator(n))
        plan.set_tag(0, op_tag)
    if _on_device(field):
        plan.set_field_device(field.ptr)
    else:
        plan.set_field(field)

    bar = _progress_bar(show_progress)
    if fibre.h is None:
        if return_steps and (every is not None or z_list is not None) and not fibre.single and n <= (1 << _lib.DIRECT_LOG2_MAX) and float(L) > 0:
            z, snaps = _adaptive_capture(plan, fibre, every, z_list)
            steps, every, z_list = len(z) - 1, None, None                         # (thinned already)
        else:                                                                    # (a single step, a split plan: every snapshot is taken; picked below)
            steps, z, snaps = plan.propagate_adaptive(gamma, fibre.length, fibre.phi_max, fibre.single, snapshots=return_steps)
    else:
        hs, z = fibre.schedule()
        steps = hs.size
        snaps = None
        z_list = None                                     # a fixed step ignores `z_list`: ADVICE.md's second finding, left as it is here
        if return_steps and every is not None and steps and n > (1 << _lib.DIRECT_LOG2_MAX):
            # a split plan (more than 2^22 samples per row) has no capture beside the run: `every` steps per call, the field read back in between
            k = _lib.every_index(steps, every)
            fields = [plan.get_field()]
            for a0, a1 in zip(k[:-1], k[1:]):
                plan.propagate_fixed(gamma, hs[a0:a1])
                fields.append(plan.get_field())
            snaps, z, every = np.stack(fields), np.asarray(z)[k], None
        elif return_steps and every is not None and steps:
            cap = plan.propagate_fixed_capture(gamma, hs, every=every)
            snaps, z, every = cap["fields"], np.asarray(z)[cap["steps"]], None              # (thinned already)
        elif return_steps:
            snaps = plan.propagate_fixed(gamma, hs, snapshots=True) if steps else plan.get_field().reshape(1, batch, n)
        elif bar is not None and steps:
            done = 0
            for chunk in np.array_split(hs, min(20, steps)):      # progress needs sync points
                plan.propagate_fixed(gamma, chunk)
                plan.synchronize()
                done += chunk.size
                bar.update(min(100.0 * float(chunk.sum()) / float(L), max(0.0, 100.0 - bar.n)))
                bar.set_postfix(FFTs=2 * done)
        elif steps:
            plan.propagate_fixed(gamma, hs)
    if bar is not None:
        if fibre.h is None or return_steps:
            bar.update(100)
            bar.set_postfix(FFTs=2 * int(steps))
        bar.close()

    if return_steps:
        if (every is not None or z_list is not None) and snaps.shape[0] == len(z):      # (every snapshot was taken: the adaptive run, a run of no steps; thinned here)
            keep = _keep_indices(z, snaps.shape[0], every, z_list)
            snaps, z = snaps[keep], np.asarray(z)[keep]
        A_z = snaps.reshape((snaps.shape[0],) + shape)
        return np.asarray(z, dtype=np.float64), A_z
    if KEEP_ON_DEVICE:
        out = _lib.DeviceArray(shape, plan.cdtype, plan.device)
        plan.get_field_device(out.ptr)
        output = optical_signal.from_device(out)
    else:
        output = optical_signal(plan.get_field().reshape(shape))
    # beside the reference's execution_time: which engine ran ("two_kernel", "medium", "adaptive_fused" ..., _lib.ENGINES) and whether a one-launch
    # engine had to give way to its fallback -- a shared GPU or a profiler turns the fast engines off without any other sign
    info = plan.last_run_info()
    output.engine = info["engine"] + (" (fell back)" if info["fell_back"] else "")
    return output


def DBP(input: optical_signal,
        length: float,
        alpha: float = 0.0,
        beta_2: float = 0.0,
        beta_3: float = 0.0,
        gamma: float = 0.0,
        phi_max: float = 0.01,
        h: float = None,
        show_progress: bool = False,
        return_steps: bool = False,
        *,
        precision="complex64",
        device=None,
        every: int = None,
        z_list=None,
        coupling: str = None,
        kappa: float = None,
        pmd: float = None,
        pmd_seed: int = None,
        pmd_scatter: bool = True):
    """Digital back-propagation = ``FIBER`` with every operator negated (``devices.py:1280-1283``); ``coupling`` / ``kappa`` as ``FIBER``'s.  ``pmd`` is
    refused: back-propagation cannot know the fibre's random axes."""
    if pmd is not None or pmd_seed is not None or pmd_scatter is not True:
        raise ValueError("DBP takes no pmd: back-propagation cannot know the fibre's random axes")
    return FIBER(input, length=length, alpha=-alpha, beta_2=-beta_2, beta_3=-beta_3, gamma=-gamma,
                 phi_max=phi_max, h=h, show_progress=show_progress, return_steps=return_steps,
                 precision=precision, device=device, every=every, z_list=z_list, coupling=coupling, kappa=kappa)


# ------------------------------------------------------------------ DM
def DM(input: optical_signal, D: float, retH: bool = False, *, device=None):
    """Dispersive medium: one linear step ``H(w) = exp(+j w^2 D/2)``, ``D = beta_2 z`` [ps^2]
    (``devices.py:1019-1035``).  complex128; signal and noise are filtered separately and stay
    separate.  With ``retH`` also returns ``fftshift(H)``."""
    t0 = time.time()
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    D = D * 1e-12**2          # ps^2 -> s^2 (devices.py:1025); H(w) is generated on the device

    raw_s, raw_n = input._raw("signal"), input._raw("noise")
    dev = default_device() if device is None else int(device)
    shape = tuple(raw_s.shape)
    n, rows = _rows(shape)
    _check_size(n, _lib.C128)
    has_noise = raw_n is not NULL
    if not _is_fast_size(n, _lib.C128):
        # any other length: chirp-z path with H = exp(+j w^2 D / 2) formed on the host in the reference's own
        # float64 expression (devices.py:1025-1027)
        w = np.fft.fftfreq(n, float(grid.dt)) * 2 * np.pi           # typing.py:1641
        phase = 1j * w ** 2 * D / 2                                 # the exponential itself is taken on the device
        Hd = _lib.DeviceArray.from_host(phase, np.complex128, dev)
        outs = _chirpz_transfer([raw_s, raw_n] if has_noise else [raw_s], Hd, True, dev)
        output = _wrap_out(optical_signal, outs[0], outs[1] if has_noise else NULL, n_pol=input.n_pol)
        output.execution_time = time.time() - t0
        if retH:
            return back(output), np.fft.fftshift(np.exp(phase))
        return back(output)
    plan = get_plan(n, rows * (2 if has_noise else 1), _lib.C128, dev)
    # signal rows, then noise rows, straight into the plan's field buffer
    row_bytes = rows * n * 16
    with plan.lock:
        for k, a in enumerate([raw_s, raw_n] if has_noise else [raw_s]):
            if _on_device(a):
                d = _dev_array(a, np.complex128, dev)
                plan.copy_into_field(k * row_bytes, d.ptr, row_bytes, on_device=True)
            else:
                h = np.ascontiguousarray(a, dtype=np.complex128)
                plan.copy_into_field(k * row_bytes, h.ctypes.data, row_bytes, on_device=False)
        H = plan.apply_dispersion(float(grid.dt), D, want_H=retH)
        outs = []
        for k in range(2 if has_noise else 1):
            o = _lib.DeviceArray(shape, np.complex128, dev)
            plan.copy_from_field(k * row_bytes, o.ptr, row_bytes)
            outs.append(o)
    output = _wrap_out(optical_signal, outs[0], outs[1] if has_noise else NULL, n_pol=input.n_pol)
    output.execution_time = time.time() - t0
    if retH:
        return back(output), np.fft.fftshift(H)
    return back(output)


# ------------------------------------------------------------------ LPF / BPF
def _warn_narrow(cutoff_hz, fs, what):
    """The time-parallel scan behind the zero-phase filters propagates filter states over thousands of samples with
    powers of the state matrix; for a cutoff far below the sampling rate those powers are ill-conditioned and the
    result drifts away from SciPy's sample-by-sample recursion: about 5e-20 (fs / cutoff)^3 relative -- 6e-14 at
    cutoff = fs / 100, 1e-11 at fs / 500, 5e-8 at fs / 10000 (tests/diag/filter_conditioning.py)."""
    if cutoff_hz < 2e-3 * fs:
        import warnings
        warnings.warn(f"{what}: cutoff {cutoff_hz:.3g} Hz is below fs/500 ({fs / 500:.3g} Hz); the device filter then differs from "
                      f"scipy.signal.sosfiltfilt by about {5e-20 * (fs / cutoff_hz) ** 3:.1e} (relative)", RuntimeWarning, stacklevel=3)


@functools.lru_cache(maxsize=64)
def _bessel_design(n, cutoff_hz, fs):
    from scipy import signal as sg
    sos = sg.bessel(N=n, Wn=cutoff_hz, btype="low", fs=fs, output="sos", norm="mag")
    zi = sg.sosfilt_zi(sos)
    sos.setflags(write=False)
    zi.setflags(write=False)
    return sos, zi


def _bessel_sos(n, cutoff_hz, fs):
    """Filter DESIGN (O(order) host work, identical call to the reference's): Bessel low-pass as
    second-order sections, magnitude-normalised, plus the steady-state initial conditions.  SciPy
    needs a millisecond for it -- 20 to 50 times the filter kernels of a call -- so the (read-only)
    result of the last 64 distinct (order, cutoff, fs) is kept."""
    return _bessel_design(int(n) if isinstance(n, (int, np.integer)) else n, float(cutoff_hz), float(fs))


def LPF(input, BW: float, n: int = 4, fs: float = None, retH: bool = False, *, device=None):
    """Electrical low-pass filter: ``n``-th order Bessel, zero phase (``sosfiltfilt``), cutoff ``BW``
    [Hz]; reference ``devices.py:1286-1375``.  ``input``: 1-D array or :class:`electrical_signal`;
    signal and noise are filtered separately and the real part is kept.  With ``retH`` also returns
    ``fftshift`` of the frequency response over ``input.size`` points."""
    t0 = time.time()
    input, grid, back = _adopt(input, "electrical_signal")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    if input.ndim != 1:
        raise ValueError("`input` must be a 1D-array.")
    if not fs:
        fs = grid.fs
    sos, zi = _bessel_sos(n, BW, fs)
    _warn_narrow(BW, fs, "LPF")
    dev = default_device() if device is None else int(device)
    # real coefficients: Re(filter(x)) == filter(Re(x)), so only the real channel is computed
    # (signal and noise go to the device as they lie: no stacked host copy)
    has_noise = input._raw("noise") is not NULL
    res = []
    for a in ([input._raw("signal"), input._raw("noise")] if has_noise else [input._raw("signal")]):
        if _on_device(a) and a.dtype != np.float64:
            a = _lib.real_device(a if a.dtype == np.complex128 else a.astype(np.complex128))     # complex on the device: its real part, there
        x = a if _on_device(a) else _lib.DeviceArray.from_host(np.real(a), np.float64, dev)
        y = _lib.DeviceArray(x.shape, np.float64, dev)
        _lib.sosfiltfilt_device(sos, zi, x.ptr, y.ptr, x.shape[-1], 1, False, dev)
        res.append(y)
    output = _wrap_out(electrical_signal, res[0], res[1] if has_noise else NULL)
    output.execution_time = time.time() - t0
    if retH:
        from scipy import signal as sg
        _, H = sg.sosfreqz(sos, worN=input.size, fs=fs, whole=True)
        return back(output), np.fft.fftshift(H)
    return back(output)


def _bpf_on_grid(x, BW, grid, device):
    """BPF of one of OUR signals on another library's sampling grid (EDFA of an adopted input)."""
    if grid is gv:
        return BPF(x, BW, device=device)
    saved = (gv.fs, gv.dt)
    gv.fs, gv.dt = grid.fs, grid.dt
    try:
        return BPF(x, BW, device=device)
    finally:
        gv.fs, gv.dt = saved


def BPF(input: optical_signal, BW: float, n: int = 4, *, device=None):
    """Optical band-pass filter: Bessel low-pass of cutoff ``BW/2`` on the complex envelope, zero phase;
    reference ``devices.py:788-826``.  Signal and noise are filtered separately."""
    t0 = time.time()
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type (optical_signal).")
    sos, zi = _bessel_sos(n, BW / 2, grid.fs)
    _warn_narrow(BW / 2, grid.fs, "BPF")
    dev = default_device() if device is None else int(device)
    has_noise = input._raw("noise") is not NULL
    res = []
    for a in ([input._raw("signal"), input._raw("noise")] if has_noise else [input._raw("signal")]):
        cplx = np.dtype(a.dtype).kind == "c"                # a real envelope (a CW laser) stays real, as in SciPy
        x = _dev_array(a, np.complex128 if cplx else np.float64, dev)
        y = _lib.DeviceArray(x.shape, x.dtype, dev)
        _lib.sosfiltfilt_device(sos, zi, x.ptr, y.ptr, x.shape[-1], x.size // x.shape[-1], cplx, dev)
        res.append(y)
    output = _wrap_out(optical_signal, res[0], res[1] if has_noise else NULL, n_pol=input.n_pol)
    output.execution_time = time.time() - t0
    return back(output)


# ----------------------------------------------------------------------------- receiver front-end
# SURVEY.md 8(f) rank 2.  The random currents / fields are drawn on the host from the GLOBAL np.random
# generator with the reference's calls in the reference's order, so a script that seeds np.random gets the
# same realisation from either library, and uploaded; all arithmetic (square law, gain, the sums, the zero-phase
# filters) runs on the GPU and the results stay there.
# rng="device": the library's Philox4x32-10 generator (csrc/device_mem.hip) instead of NumPy's global one -- no
# seed-for-seed parity with the reference then, only its statistics, but nothing leaves the GPU.  Every draw
# takes the next stream of the current seed; `device_rng_seed` restarts the sequence (default: OS entropy).
_DEVICE_RNG = {"seed": int.from_bytes(os.urandom(8), "little"), "stream": 0}


def device_rng_seed(seed: int):
    """Seed the device generator used by ``PD`` / ``EDFA`` / ``LASER`` with ``rng="device"``."""
    _DEVICE_RNG["seed"], _DEVICE_RNG["stream"] = int(seed), 0


def _device_randn(shape, std, dtype, dev):
    _DEVICE_RNG["stream"] += 1
    return _lib.randn_device(shape, std, _DEVICE_RNG["seed"], _DEVICE_RNG["stream"], dtype, dev)


def _check_rng(rng):
    if rng not in ("numpy", "device"):
        raise ValueError("`rng` must be 'numpy' (the reference's draws, on the host) or 'device'")


_PD_MODES = ("ase-only", "thermal-only", "shot-only", "ase-thermal", "ase-shot", "thermal-shot", "all", "none")


def _idb(x):
    """dB -> linear (reference ``utils.py:422-451``)."""
    return 10 ** (x / 10)


def PD(input: optical_signal, BW: float, r: float = 1.0, T: float = 300.0, R_load: float = 50.0,
       include_noise: str = "all", i_dark: float = 10e-9, Fn=0, *, device=None, rng: str = "numpy") -> electrical_signal:
    """P-I-N photodetector (reference ``devices.py:1378-1555``): ``v = R_load * (r * |E|^2 + noise)``
    summed over the polarisations, low-pass filtered to ``BW`` [Hz].

    The input's own noise (ASE) appears as signal-ASE and ASE-ASE beat currents in ``.noise``; thermal
    (``4 kB T Fn fs/2 / R_load``) and shot (``2 e (mean(i_ph) + i_dark) fs/2``) currents are Gaussian.
    ``include_noise`` selects the terms as in the reference ('all', 'none', 'ase-only', 'thermal-only',
    'shot-only', 'ase-thermal', 'ase-shot', 'thermal-shot'; case-insensitive).

    ``rng`` (extension): ``"numpy"`` draws the Gaussian currents from NumPy's global generator with the
    reference's calls in the reference's order (seed-for-seed identical output: the default, because it is the
    reference's result sample for sample); ``"device"`` uses the library's Philox generator on the GPU -- same
    statistics, the whole detector stays on the device: 1.7 ms instead of 22 ms for ``PD('all')`` at 2^20 x 2
    (15x; measured, profiles/r04_final_cfg_times.txt).  Use it wherever the realisation need not be the reference's.
    """
    from numbers import Real
    from scipy.constants import e, k as kB
    t0 = time.time()
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    if not isinstance(r, Real):
        raise TypeError("`r` must be a scalar value.")
    if r <= 0 or r > 1:
        raise ValueError("`r` must be in the range (0,1]")
    if not isinstance(T, Real):
        raise TypeError("`T` must be a scalar value.")
    if T < 0:
        raise ValueError("`T` must be a positive value.")
    if not isinstance(R_load, Real):
        raise TypeError("`R_load` must be a scalar value.")
    if R_load < 0:
        raise ValueError("`R_load` must be a positive value.")
    if not isinstance(include_noise, str):
        raise TypeError("`include_noise` must be a string.")
    mode = include_noise.lower()
    _check_rng(rng)
    if mode not in _PD_MODES:
        raise ValueError("The argument `include_noise` must be one of the following: 'ase-only','thermal-only','shot-only',"
                         "'ase-thermal','ase-shot','thermal-shot','all', 'none'.")
    dev = default_device() if device is None else int(device)
    raw_s, raw_n = input._raw("signal"), input._raw("noise")
    has_ase = raw_n is not NULL
    sig_d = _dev_array(raw_s, np.complex128, dev)
    if mode == "none":
        # nothing random to add: detector and filter back to back
        v, _ = _lib.square_law_device(sig_d, None, r, post=R_load)
        output = LPF(electrical_signal.from_device(v), BW, fs=grid.fs, device=dev)
        output.execution_time = time.time() - t0
        return back(output)
    # photocurrents r |E|^2 (signal) and the signal-ASE / ASE-ASE beat terms, summed over the polarisations
    ds, dn = _lib.square_law_device(sig_d, _dev_array(raw_n, np.complex128, dev) if has_ase else None, r)

    def normal(std):
        """Gaussian current of the given standard deviation: the device generator, or NumPy's global one with the
        reference's call (devices.py:1521-1527) uploaded as it is."""
        if rng == "device":
            return _device_randn(ds.shape, std, np.float64, dev)
        return _lib.DeviceArray.from_host(np.random.normal(0, std, input.size), np.float64, dev)
    d_T = d_N = None
    if "thermal" in mode or mode == "all":
        d_T = normal((4 * kB * T * grid.fs / 2 * _idb(Fn) / R_load) ** 0.5)
    if "shot" in mode or mode == "all":
        mean = _lib.mean_device(ds, dn if has_ase else None)
        d_N = normal((2 * e * (mean + i_dark) * grid.fs / 2) ** 0.5)
    d_ase = dn if (has_ase and ("ase" in mode or mode == "all")) else None
    # (ase + shot) + thermal + dark current, times the load: the reference's order of additions (devices.py:1530-1549)
    v_noise = _lib.sum3_device(d_ase, d_N, d_T, i_dark, R_load, ds)       # all three absent ('ase-only', noiseless input): dark current alone
    v_sig = _lib.sum3_device(ds, None, None, 0.0, R_load, ds)
    output = LPF(electrical_signal.from_device(v_sig, v_noise), BW, fs=grid.fs, device=dev)
    output.execution_time = time.time() - t0
    return back(output)


def EDFA(input: optical_signal, G: float, NF: float, BW: float = None, *, device=None, rng: str = "numpy") -> optical_signal:
    """Erbium-doped fibre amplifier, simplest model (reference ``devices.py:829-942``): field gain
    ``sqrt(G)``, ASE of power ``NF h f0 (G - 1) fs`` split over two polarisations x two quadratures
    added to ``.noise``, then an optical ``BPF`` of bandwidth ``BW`` if given.  Output is always
    dual-polarisation (a single-polarisation input gets an empty y signal, but ASE in both).

    ``rng`` as in :func:`PD`: ``"numpy"`` (default) draws the ASE field from NumPy's global generator exactly as the
    reference does (seed-for-seed identical), ``"device"`` from the library's Philox generator on the GPU: 1.5 ms
    instead of 54 ms at 2^20 x 2 (35x; profiles/r04_final_cfg_times.txt) -- the four 2^20-sample host draws are
    all of the cost."""
    from scipy.constants import h
    t0 = time.time()
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    _check_rng(rng)
    g = np.sqrt(_idb(G))
    # gain, ASE loading and the optical filter on the GPU; only the source of the Gaussian field differs with `rng`
    dev = default_device() if device is None else int(device)
    raw_s, raw_n = input._raw("signal"), input._raw("noise")
    n = input.size

    def two_rows(a):                                      # (N,) -> (2, N) with an empty y polarisation; (2, N) as it is
        d = _dev_array(a, np.complex128, dev)
        if d.ndim == 2:
            return _lib.scale_add_device(d, g)
        out2 = _lib.zeros_device((2, n), np.complex128, dev)                      # empty y polarisation
        x = _lib.scale_add_device(d, g)
        _lib.api.ssfm_device_copy(dev, out2, x, n * 16, _lib.COPY_D2D)
        return out2
    sig = two_rows(raw_s)
    P_ase = _idb(NF) * h * grid.f0 * (_idb(G) - 1) * grid.fs
    if rng == "device":
        ase = _device_randn((2, n), np.sqrt(P_ase / 4), np.complex128, dev)
    else:                                                 # the reference's draws (devices.py:930-931), uploaded as they are
        draws = np.sqrt(P_ase / 4) * np.random.randn(4, n)
        ase = _lib.DeviceArray.from_host(draws[:2] + 1j * draws[2:], np.complex128, dev)
    noi = ase if raw_n is NULL else two_rows(raw_n) + ase
    output = _wrap_out(optical_signal, sig, noi, n_pol=2)
    if BW is not None:
        output = _bpf_on_grid(output, BW, grid, device)
    output.execution_time = time.time() - t0
    return back(output)


# ----------------------------------------------------------------------------- PRBS
_PRBS_TAPS = {7: (7, 6), 9: (9, 5), 11: (11, 9), 15: (15, 14), 20: (20, 3), 23: (23, 18), 31: (31, 28)}


def PRBS(order: int, len: int = None, seed: int = None, return_seed: bool = False, *, device=None):
    """Pseudo-random binary sequence of the reference's LFSR (``devices.py:63-182``), bit for bit: polynomial
    ``x^order + x^t2 + 1`` (PRBS-7/9/11/15/20/23/31), state seeded with ``seed % 2**order`` (default all ones;
    0 becomes 1 with a UserWarning), output = bit 0 of the state before every shift.  With ``return_seed`` also
    the final state, to continue the sequence.

    The reference walks the register one bit per Python iteration.  Here the bits are generated by a HIP kernel
    (``ssfm_prbs``, csrc/prbs.hip): a shift is a linear map over GF(2), so every thread jumps to its chunk of the
    sequence with powers of the shift matrix and walks it exactly as the reference does.  The sequence stays in GPU
    memory (``binary_sequence.from_device``) until somebody reads ``.data``; a ``DAC`` takes it from there.
    """
    import warnings
    t0 = time.time()
    if seed is not None:
        seed = seed % (2 ** order)
    else:
        seed = (1 << order) - 1
    if seed == 0:
        seed = 1
        warnings.warn("The seed can't be 0 or a multiple of 2**order. It has been changed to 1.", UserWarning)
    if len is not None:
        if not isinstance(len, int):
            raise TypeError("The parameter `len` must be an integer.")
        if len <= 0:
            raise ValueError("The parameter `len` must be an integer greater than cero.")
    else:
        len = 2 ** order - 1
    if order not in _PRBS_TAPS:
        raise ValueError("The parameter `order` must be one of the following values (7, 9, 11, 15, 20, 23, 31).")
    dev = default_device() if device is None else int(device)
    bits, last = _lib.prbs_device(order, len, seed, dev)
    output = binary_sequence.from_device(bits)
    if not KEEP_ON_DEVICE:
        output.data                                         # noqa: B018 -- the attribute read downloads
    output.execution_time = time.time() - t0
    if not return_seed:
        return output
    return output, last


# ----------------------------------------------------------------------------- DAC
_DAC_SHAPES = ["nrz", "gaussian", "rcos"]


def _pulse_grid(span, sps):
    """``t = linspace(-span/2, span/2, span*sps + 1)`` as (npts, start, step, stop), NumPy's own arithmetic."""
    npts = span * sps + 1
    start, stop = -span / 2, span / 2
    return npts, start, (stop - start) / (npts - 1), stop


def _nrz_spec(span, sps, T):
    """reference ``utils.py:1924-1947``: 1 on [-T/2, T/2)."""
    return (0,) + _pulse_grid(span, sps) + (0, [-T / 2, T / 2]), False


def _gauss_spec(span, sps, T=1, m=1, c=0.0):
    """reference ``utils.py:1880-1922``: ``exp(-(alpha (1 + j c) t)^(2m))``, ``alpha = 2 sqrt(ln 2) / T``; complex."""
    if 2 * m > 98:
        raise ValueError("The parameter `m` must be below 50.")
    k = 2 * np.sqrt(np.log(2)) / T * (1 + 1j * c)
    return (1,) + _pulse_grid(span, sps) + (2 * m, [k.real, k.imag]), True


def _rcos_spec(beta, span, sps, shape="sqrt"):
    """reference ``utils.py:1791-1878`` (MATLAB ``rcosdesign`` without the energy normalisation)"""
    if not (0 <= beta <= 1):
        raise ValueError("beta must be in [0, 1]")
    if shape not in ("sqrt", "normal"):
        raise ValueError("shape must be 'sqrt' or 'normal'")
    grid = _pulse_grid(span, sps)
    if beta == 0:
        return (4,) + grid + (0, []), False
    if shape == "normal":
        return (2,) + grid + (0, [2 * beta, np.pi * beta, (np.pi / 4) * np.sinc(1 / (2 * beta))]), False
    at_zero = (1 - beta) + 4 * beta / np.pi
    at_special = (beta / np.sqrt(2)) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
    return (3,) + grid + (0, [beta, 4 * beta, 1 - beta, 1 + beta, 1 / (4 * beta), at_zero, at_special]), False


def _upfir_device(bits, h, up: int, dev: int, spec=None) -> "_lib.DeviceArray":
    """``upfir`` of the reference (``utils.py:1949-1981``): zero-stuffing at offset ``up//2`` and the 'same' part of
    the linear convolution with the pulse -- as ONE circular convolution on a power-of-two complex128 plan
    (``x <- ifft(fft(x) * fft(h))``, three launches); SciPy's ``fftconvolve`` does the same on the host.
    The pulse is either an explicit impulse response ``h`` (uploaded) or ``spec = (args of Plan.load_pulse, complex?)``
    of a built-in shape, generated on the device.  ``bits``: a host array, or the uint8 device array a ``PRBS`` left
    in GPU memory (then nothing is uploaded at all)."""
    n = int(bits.size) * up
    if spec is None:
        h = np.asarray(h)
        taps, cplx = h.size, np.iscomplexobj(h)
    else:
        taps, cplx = spec[0][1], spec[1]
    full = n + taps - 1
    M = 1 << max(8, (full - 1).bit_length())
    lo, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if M > (1 << hi):
        raise ValueError(f"DAC: {bits.size} bits x {up} samples with a {taps}-tap pulse exceed the device path (2^{hi} points)")
    plan = get_plan(M, 1, _lib.C128, dev)
    with plan.lock:
        if spec is None:
            hd = _lib.DeviceArray.from_host(np.ascontiguousarray(h, dtype=np.complex128 if cplx else np.float64), None, dev)
            plan.load_padded(hd)                                # field <- h, zero-padded
        else:
            plan.load_pulse(*spec[0])                           # field <- the pulse, generated in place
        plan.table_from_field(0)                                # slot 0 <- fft(h)  (the plan drops the slot's old label itself)
        if _on_device(bits) and bits.dtype == np.uint8:
            plan.load_bits(bits, up)                            # field <- zero-stuffed bits, where the generator left them
        else:
            bd = _lib.DeviceArray.from_host(np.ascontiguousarray(bits, dtype=np.float64), np.float64, dev)
            plan.load_symbols(bd, up)                           # field <- zero-stuffed bits
        plan.apply_table(0)
        out = _lib.DeviceArray((n,), np.complex128, dev)
        plan.copy_from_field(((taps - 1) // 2) * 16, out.ptr, n * 16)          # 'same': centred with respect to the full output
    return out if cplx else _lib.real_device(out)


def _filter_device(sig, noise, h):
    """``scipy.signal.fftconvolve(x, h, mode='same')`` of a device-resident signal and its noise (``electrical_signal.filter``): the circular
    convolution of :func:`_upfir_device` on a power-of-two complex128 plan, the input loaded from where it lies.  With real signal, noise and
    taps the noise rides as the imaginary part of the signal's field: one convolution filters both and ``ssfm_signal_split`` parts them
    again (the peak of that field is the larger of the two, so a noise below 1e-12 of the signal loses its digits).  Returns
    ``(signal, noise or None)`` DeviceArrays."""
    h = np.asarray(h)
    if h.ndim != 1 or h.size < 1:
        raise ValueError(f"filter: `h` must be a 1D array of at least one tap, got shape {h.shape}")
    n, taps, dev = sig.size, h.size, sig.device
    cplx_h, cplx_x = np.iscomplexobj(h), sig.dtype.kind == "c"
    full = n + taps - 1
    M = 1 << max(8, (full - 1).bit_length())
    lo, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if M > (1 << hi):
        raise ValueError(f"filter: {n} samples with {taps} taps exceed the device path (2^{hi} points)")
    off = ((taps - 1) // 2) * 16                                # 'same': centred with respect to the full output
    plan = get_plan(M, 1, _lib.C128, dev)
    with plan.lock:
        hd = _lib.DeviceArray.from_host(np.ascontiguousarray(h, dtype=np.complex128 if cplx_h else np.float64), None, dev)
        plan.load_padded(hd)
        plan.table_from_field(0)                                # slot 0 <- fft(h)
        if not cplx_h and not cplx_x:
            x = sig
            if noise is not None:
                x = _lib.DeviceArray((n,), np.complex128, dev)
                _lib.api.ssfm_signal_pack(sig, noise, n, x)
            plan.load_padded(x)
            plan.apply_table(0)
            plan.synchronize()
            out_s = _lib.DeviceArray((n,), np.float64, dev)
            out_n = None if noise is None else _lib.DeviceArray((n,), np.float64, dev)
            _lib.api.ssfm_signal_split(plan.field_device_ptr + off, n, out_s, out_n)
            return out_s, out_n
        outs = []
        for x in (sig, noise):
            if x is None:
                outs.append(None)
                continue
            plan.load_padded(x)
            plan.apply_table(0)
            out = _lib.DeviceArray((n,), np.complex128, dev)
            plan.copy_from_field(off, out.ptr, n * 16)
            outs.append(out)
    return outs[0], outs[1]


def DAC(input, pulse_shape: str = "nrz", coupling: str = "DC", Vpp: float = 1.0, offset: float = 0.0, h=None, BW: float = None,
        *, device=None, **kwargs) -> electrical_signal:
    """Digital-to-analog converter (reference ``devices.py:185-350``): a bit sequence becomes ``gv.sps`` samples
    per bit of the chosen pulse (``'nrz'`` with ``T``; ``'gaussian'`` with ``T``, ``m``, ``c``; ``'rcos'`` with
    ``beta``, ``rcos_type``; or an explicit impulse response ``h``), scaled by ``Vpp``, shifted by ``offset``,
    optionally AC-coupled and band-limited by ``LPF(BW)``.  The pulse spans ``max(4, bits - 4)`` symbols, i.e. the
    shaping is a convolution as long as the signal: it runs as an FFT convolution on the GPU."""
    t0 = time.time()
    seq = input if isinstance(input, binary_sequence) else binary_sequence(input)
    bits = seq.size
    sps = gv.sps
    dev = default_device() if device is None else int(device)
    data = seq._raw()                                       # host bits, or the device array a PRBS left in GPU memory
    if _on_device(data) and data.device != dev:
        data = seq.to_numpy()
    span = max(4, bits - 4)
    spec = None
    if h is not None:
        h = np.asarray(h)
    elif pulse_shape.lower() not in _DAC_SHAPES:
        raise ValueError(f"The parameter `pulse_shape` must be one of the following values {_DAC_SHAPES}")
    elif pulse_shape.lower() == "nrz":
        T = kwargs.get("T", 1)
        if not isinstance(T, int):
            raise TypeError("The parameter `T` must be an integer.")
        if T <= 0:
            raise ValueError("The parameter `T` must be greater than 0.")
        if T > 2 * sps:
            raise ValueError("The parameter `T` must be less than 2*sps.")
        spec = _nrz_spec(span, sps, T)
    elif pulse_shape.lower() == "gaussian":
        c, m, T = kwargs.get("c", 0.0), kwargs.get("m", 1), kwargs.get("T", 1)
        if not isinstance(c, (int, float)):
            raise TypeError("The parameter `c` must be a real number.")
        if not isinstance(m, int):
            raise TypeError("The parameter `m` must be an integer.")
        if not isinstance(T, int):
            raise TypeError("The parameter `T` must be an integer.")
        if m <= 0:
            raise ValueError("The parameter `m` must be greater than 0.")
        if T <= 0:
            raise ValueError("The parameter `T` must be greater than 0.")
        if T > 2 * sps:
            raise ValueError("The parameter `T` must be less than 2*sps.")
        spec = _gauss_spec(span, sps, T=T, m=m, c=c)
    else:
        spec = _rcos_spec(kwargs.get("beta", 0.25), span, sps, shape=kwargs.get("rcos_type", "normal"))
    if Vpp is not None:
        if not isinstance(Vpp, (int, float)):
            raise TypeError("The parameter `Vpp` must be a scalar value.")
        if Vpp <= 0 or Vpp > 48:
            raise ValueError("The parameter `Vpp` must be in the range (0, 48] Volts.")
    if offset is not None:
        if not isinstance(offset, (int, float)):
            raise TypeError("The parameter `offset` must be a scalar value.")
        if np.abs(offset) > 48:
            raise ValueError("The parameter `offset` must be in the range [-48, 48] Volts.")
    if coupling.upper() not in ("AC", "DC"):
        raise ValueError("The parameter `coupling` must be either 'AC' or 'DC'.")
    x = _upfir_device(data, h, sps, dev, spec)              # stays on the device: float64, or complex128 for a complex pulse
    if Vpp is not None:
        x = _lib.axpb_device(x, Vpp, 0.0)
    if offset is not None:
        x = _lib.axpb_device(x, 1.0, offset)
    if coupling.upper() == "AC":
        x = _lib.shift_device(x, -_lib.mean2_device(x))       # x - mean(x), real or complex, on the device
    output = _wrap_out(electrical_signal, x, NULL)
    if BW is not None:
        output = LPF(output, BW, device=dev)
    output.execution_time = time.time() - t0
    return output


# ----------------------------------------------------------------------------- LASER / MZM
# Elementwise HIP kernels (csrc/transmitter.hip) in the reference's own order of operations; the laser's random
# increments are drawn from NumPy's global generator with the reference's calls, so a seeded script gets the same laser
# noise.  They complete the transmitter chain PRBS -> DAC -> MZM(LASER) in front of FIBER, which stays in GPU memory.
def LASER(P0: float, lw: float = None, rin: float = None, df: float = None, *, device=None, rng: str = "numpy") -> optical_signal:
    """CW laser of ``P0`` dBm over ``gv.t`` (reference ``devices.py:353-510``): optional linewidth ``lw`` [Hz] (Wiener
    phase noise), relative intensity noise ``rin`` [dB/Hz] and frequency offset ``df`` [Hz]; single polarisation.
    Real-valued (float64) unless ``lw`` or ``df`` is given, as in the reference.  ``rng`` as in :func:`PD`:
    ``"numpy"`` draws the noise from NumPy's global generator with the reference's calls, ``"device"`` from the
    library's Philox generator (the running sum of the phase increments is then a device scan too)."""
    t0 = time.time()
    _check_rng(rng)
    t = gv.t
    n = t.size
    dev = default_device() if device is None else int(device)
    amp = float(np.sqrt(10 ** (P0 / 10 - 3)))
    phase = rin_noise = w = None
    if lw is not None:
        std = np.sqrt(2 * np.pi * lw * gv.dt)
        if rng == "device":
            phase = _lib.cumsum_device(_device_randn((n,), std, np.float64, dev))
        else:
            phase = _lib.DeviceArray.from_host(np.cumsum(np.random.normal(0, std, n)), np.float64, dev)
    if rin is not None:
        std = np.sqrt(_idb(rin) * gv.fs)
        if rng == "device":
            rin_noise = _device_randn((n,), std, np.float64, dev)
            lowest = _lib.min_device(rin_noise)
        else:
            r = np.random.normal(0, std, n)
            lowest = r.min()
            rin_noise = _lib.DeviceArray.from_host(r, np.float64, dev) if lowest >= -1 else None
        if lowest < -1:
            raise ValueError("Noise power is to high, try decrease RIN parameter.")
    if df is not None:
        if np.abs(df) > gv.fs / 2:
            raise ValueError("The laser frequency is out of the Nyquist range. Try increase the sampling frequency.")
        w = 2 * np.pi * df                                   # exp(1j*2*pi*df*t): the phase is (2 pi df) * t_i
    out = _lib.laser_device(n, amp, phase, rin_noise, w, float(t[1]) if n > 1 else 0.0, float(t[-1]), dev)
    output = _wrap_out(optical_signal, out, NULL)
    output.execution_time = time.time() - t0
    return output


def MZM(op_input: optical_signal, el_input, bias: float = 0.0, Vpi: float = 5.0, loss_dB: float = 0.0, ER_dB: float = 26.0,
        pol: str = "x", BW: float = None, *, device=None) -> optical_signal:
    """Mach-Zehnder modulator (reference ``devices.py:620-786``): ``out = in * sqrt(loss) (cos g + j eta/2 sin g)``,
    ``g = pi/(2 Vpi) (v + bias)``, ``eta = 2 sqrt(1/ER)``; the drive voltage's own noise enters ``g``, optical
    signal and optical noise are both multiplied; of a dual-polarisation input only ``pol`` survives; ``BW`` adds
    a ``BPF``."""
    t0 = time.time()
    op_input, grid, back = _adopt(op_input, "optical_signal")
    if not isinstance(op_input, optical_signal):
        raise TypeError("`op_input` must be of type 'optical_signal'.")
    if isinstance(el_input, electrical_signal) or type(el_input).__name__ == "electrical_signal":
        el_input = _adopt(el_input, "electrical_signal")[0]
    else:
        el_input = electrical_signal(el_input)
    if el_input.ndim > 1:
        raise ValueError("`el_input` must be a scalar or 1D-array.")
    if pol not in ["x", "y"]:
        raise ValueError("The parameter `pol` must be one of the following values ('x', 'y').")
    loss = _idb(-loss_dB)
    eta = 2 * _idb(-ER_dB) ** 0.5
    k = np.pi / 2 / Vpi
    raw_s, raw_n = op_input._raw("signal"), op_input._raw("noise")
    raw_v, raw_vn = el_input._raw("signal"), el_input._raw("noise")
    dev = default_device() if device is None else int(device)
    n = tuple(raw_s.shape)[-1]
    # one HIP kernel (ssfm_mzm, csrc/transmitter.hip) whatever the inputs are: a DAC output or a carrier that is
    # already in GPU memory is used where it lies, host arrays are uploaded (a scalar drive is spread over the grid)
    cplx = any(a is not NULL and a.dtype.kind == "c" for a in (raw_v, raw_vn))
    vdt = np.complex128 if cplx else np.float64

    def drive(a):
        if a is NULL:
            return None
        if _on_device(a) and tuple(a.shape) == (n,) and a.dtype == vdt:
            return _dev_array(a, vdt, dev)
        host = a.to_host() if _on_device(a) else np.asarray(a)
        return _lib.DeviceArray.from_host(np.broadcast_to(host, (n,)), vdt, dev)     # ValueError when the lengths disagree
    out_s, out_n = _lib.mzm_device(_dev_array(raw_s, np.complex128, dev), None if raw_n is NULL else _dev_array(raw_n, np.complex128, dev),
                                   drive(raw_v), drive(raw_vn), k, bias, loss ** 0.5, eta / 2, 1 if pol == "x" else 0)
    output = _wrap_out(optical_signal, out_s, NULL if out_n is None else out_n, n_pol=op_input.n_pol)
    if BW is not None:
        output = _bpf_on_grid(output, BW, grid, device)
    output.execution_time = time.time() - t0
    return back(output)


# ------------------------------------------------------------------ the OOK receiver: GET_EYE and SAMPLER (csrc/eye.hip)
# the state block of ssfm_eye_estimate / ssfm_eye_levels, in the order of eye.hip `enum Slot`
_EYE_SLOTS = ("C0 C1 T0 Y0 T1 Y1 IT1 DONE1 IT2 DONE2 VM NBOT NTOP TOPSTART BOT0 BOT1 TOP0 TOP1 V25 V75 STATE0 STATE1 YCT YC YL YR NBAND TMEAN MIND "
              "MU0 MU1 SD0 SD1 N0 N1 NC CMEAN CVAR INVH KDE SINGULAR NONFINITE").split()
_S = {name: k for k, name in enumerate(_EYE_SLOTS)}
_EYE_MAX_N = 1 << 21


def _real_sum_device(input, n: int, shift: int, dev: int) -> "_lib.DeviceArray":
    """``np.roll(Re(signal + noise)[:n], shift)`` as a float64 device array (one pass; host inputs are uploaded once)."""
    raws = [input._raw("signal")] + ([] if input._raw("noise") is NULL else [input._raw("noise")])
    cplx = any(np.iscomplexobj(np.empty(0, a.dtype)) for a in raws)
    arrs = [_dev_array(a, np.complex128 if cplx else np.float64, dev) for a in raws]
    out = _lib.DeviceArray((n,), np.float64, dev)
    _lib.api.ssfm_eye_prepare(dev, arrs[0], arrs[1] if len(arrs) > 1 else None, int(cplx), n, int(shift), out)
    return out


def _resample_device(x: "_lib.DeviceArray", m: int, dev: int) -> "_lib.DeviceArray":
    """``scipy.signal.resample(x, m)`` of a real device signal: the forward and inverse float64 transforms of ``_ChirpZ`` with the
    spectrum cut or zero-padded between them (csrc/eye.hip k_respectrum)."""
    n = x.size
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if 2 * max(n, m) - 1 > (1 << hi):
        raise ValueError(f"the device transform takes 2 ... 2^{hi - 1} samples, the resampling needs {n} -> {m} (there is no CPU fallback)")
    X = _lib.DeviceArray((1, n), np.complex128, dev)
    _lib.api.ssfm_eye_resample_stage(dev, 0, x, n, X, n)
    with _ChirpZ(n, 1, dev) as eng:
        eng.fourier(X, False)
    Y = _lib.DeviceArray((1, m), np.complex128, dev)
    _lib.api.ssfm_eye_resample_stage(dev, 1, X, n, Y, m)
    with _ChirpZ(m, 1, dev) as eng:
        eng.fourier(Y, True)
    y = _lib.DeviceArray((m,), np.float64, dev)
    _lib.api.ssfm_eye_resample_stage(dev, 2, Y, n, y, m)
    return y


def _nearest(levels: np.ndarray, v: float) -> float:
    return float(levels[np.argmin(np.abs(levels - v))])


def GET_EYE(input, nslots: int = 4096, sps_resamp: int = None, *, device=None, _grid=None):
    """Eye-diagram estimator, reference ``devices.py:1635-1868``: the same truncation, roll, resampling, levels, crossings, cluster
    moments and KDE threshold, computed on the GPU (csrc/eye.hip).  Returns :class:`~opticomlib_amd.typing.eye`.

    Two-means: a deterministic Lloyd iteration (1-D from (min, max), 2-D from the 25-75 % band split at its mean t) replaces
    sklearn's KMeans(n_init=10); for an open eye both reach the same fixed point (sklearn stops within its ``tol`` of it).

    Host round trips per call on a device-resident signal (``eye.round_trips``), every blocking host wait counted: the signal's
    preparation (1); without ``sps_resamp`` nothing more before the estimate, with it the three resampling stages and the two transforms (5); the estimate
    (the t-grid upload and one state read: 2, and one more read per 24 Lloyd steps beyond the first 24 of a two-means); the
    moments and threshold (one state read: 1).  So 4 without resampling and 9 with it, for an eye whose two-means converge in
    24 steps.

    A signal that holds NaN or infinity (after the resampling) raises ``ValueError``, as the reference's ``KMeans.fit`` does: the ends of
    the sorted copy flag it on the device, and the estimate stops at its first state read."""
    t0 = time.time()
    input, grid, _ = _adopt(input, "electrical_signal")
    grid = grid if _grid is None else _grid                 # (DSP: the grid of the caller's library)
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    if input.ndim != 1:
        raise ValueError("`input` must be a 1D-array.")
    sps, dt = int(grid.sps), grid.dt
    size = input.size - input.size % (2 * sps)
    nslots = min(size // sps, int(nslots))
    if nslots < 2 or nslots % 2:
        raise ValueError(f"GET_EYE needs an even number of slots >= 2, got {nslots} (signal of {input.size} samples at sps={sps})")
    n0 = nslots * sps
    s = int(sps_resamp) if sps_resamp else sps
    n = nslots * s
    if max(n0, n) > _EYE_MAX_N:
        raise ValueError(f"GET_EYE on the device takes up to 2^21 samples, got {max(n0, n)} (there is no CPU fallback)")
    dev = default_device() if device is None else int(device)
    x0 = _real_sum_device(input, n0, -sps // 2 + 1, dev)
    y = _resample_device(x0, n, dev) if sps_resamp else x0
    waits = 1 + (5 if sps_resamp else 0)                    # ssfm_eye_prepare; the three stages and the two transforms
    tg = np.linspace(-1, 1 - 1 / s, 2 * s)
    st = np.zeros(64)
    trips = _lib._I64(0)
    _lib.api.ssfm_eye_estimate(dev, y, n, _lib._ptr(tg), 2 * s, x0, n0, _lib._ptr(st), st.size, C.byref(trips))
    S = lambda name: float(st[_S[name]])
    if S("NONFINITE"):
        raise ValueError("GET_EYE: the signal holds NaN or infinity (the two-means take finite samples only)")
    for part, count in (("upper", S("NTOP")), ("lower", S("NBOT"))):
        if count < 2:
            raise ValueError(f"Computed lag ({int(count) // 2}) must be at least 1: the {part} half of the eye holds {int(count)} samples.")
    d = {"sps": sps, "dt": dt, "y": y, "_nslots": nslots, "execution_time": 0.0}
    if sps_resamp:
        d["sps_resamp"] = int(sps_resamp)
    d["top_int"] = np.array((S("TOP0"), S("TOP1")))
    d["bot_int"] = np.array((S("BOT0"), S("BOT1")))
    if S("NBAND") >= 2:
        c = np.array([[S("T0"), S("Y0")], [S("T1"), S("Y1")]])
        left, right = np.argmin(c[:, 0]), np.argmax(c[:, 0])
        t_left, t_right, t_c = _nearest(tg, c[left, 0]), _nearest(tg, c[right, 0]), _nearest(tg, c[:, 0].mean())
        d.update(y_left=S("YL"), y_right=S("YR"), _v25=S("V25"), _v75=S("V75"))
    else:                                                   # the reference's `except ValueError` branch
        t_left, t_right, t_c = -0.5, 0.5, 0.0
        d.update(y_left=None, y_right=None, _v25=None, _v75=None)
    t_dist = t_right - t_left
    t_span0, t_span1 = t_c - 0.05 * t_dist, t_c + 0.05 * t_dist
    d.update(t_left=t_left, t_right=t_right, t_opt=t_c, t_dist=t_dist, t_span0=t_span0, t_span1=t_span1, _y_center=S("YC"))
    k_c = int(np.abs(tg - t_c).argmin())                    # the first index of the minimum of |t - t_center| lies in the first period
    instant = k_c - s // 2 + 1
    d["i"] = int(instant / sps_resamp * sps) if sps_resamp else int(instant)
    ks = np.nonzero((t_span0 < tg) & (tg < t_span1))[0]
    k_lo, k_hi = (int(ks[0]), int(ks[-1]) + 1) if ks.size else (0, 0)
    lv = np.zeros(64)
    _lib.api.ssfm_eye_levels(dev, y, n, 2 * s, k_lo, k_hi, S("YC"), 500, _lib._ptr(lv), lv.size)
    L = lambda name: float(lv[_S[name]])
    mu0, mu1, s0, s1 = L("MU0"), L("MU1"), L("SD0"), L("SD1")
    d.update(mu0=mu0, mu1=mu1, s0=s0, s1=s1)
    d["threshold"] = None if L("SINGULAR") else float(np.linspace(mu0, mu1, 500)[int(L("KDE"))])
    with np.errstate(divide="ignore", invalid="ignore"):
        d["er"] = 10 * np.log10(mu1 / mu0) if mu0 > 0 else np.inf if mu0 == 0 else np.nan
    d["eye_h"] = mu1 - 3 * s1 - mu0 - 3 * s0
    d["round_trips"] = waits + int(trips.value) + 1
    d["execution_time"] = time.time() - t0
    return eye(**d)


def _slice_count(n: int, instant: int, step: int):
    start, stop, step = slice(int(instant), None, int(step)).indices(n)
    return start, len(range(start, stop, step))


def _sample_device(a, instant: int, step: int, dev: int, thr=None, noise=None):
    """``a[instant::step]`` of a float64 array (host or device) gathered on the device; with ``thr`` the uint8 decision
    ``a + noise > thr`` at those samples instead (``noise``: None or a float64 array of the same length)."""
    x = _dev_array(a, np.float64, dev)
    nz = None if noise is None else _dev_array(noise, np.float64, dev)
    start, count = _slice_count(x.size, instant, step)
    out = _lib.DeviceArray((max(count, 1),), np.uint8 if thr is not None else np.float64, dev)
    vals, bits = (None, out) if thr is not None else (out, None)
    _lib.api.ssfm_device_sample(dev, x, nz, start, int(step), count, float(thr or 0.0), vals, bits)
    if count == 0:
        return np.empty(0, np.uint8 if thr is not None else np.float64)
    return out


def SAMPLER(input, instant: int, *, device=None):
    """Digital sampler, reference ``devices.py:1871-1891``: ``input[instant::gv.sps]`` of signal and noise, gathered on the GPU
    (real signals; a complex signal is sliced where it lies)."""
    t0 = time.time()
    input, grid, back = _adopt(input, "electrical_signal")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    dev = default_device() if device is None else int(device)
    sps = int(grid.sps)
    outs = []
    for a in (input._raw("signal"), input._raw("noise")):
        if a is NULL:
            outs.append(NULL)
        elif np.iscomplexobj(np.empty(0, a.dtype)):
            outs.append((a.to_host() if _on_device(a) else np.asarray(a))[instant::sps])
        else:
            outs.append(_sample_device(a, instant, sps, dev))
    if any(isinstance(o, np.ndarray) for o in outs):
        output = electrical_signal(*[o.to_host() if _on_device(o) else o for o in outs])
    else:
        output = _wrap_out(electrical_signal, outs[0], outs[1])
    output.execution_time = time.time() - t0
    return back(output)


# ------------------------------------------------------------------ PM (csrc/transmitter.hip)
def PM(op_input: optical_signal, el_input, Vpi: float = 5.0, *, device=None) -> optical_signal:
    """Optical phase modulator (reference ``devices.py:513-612``): ``out = in * exp(j el_input pi / Vpi)``.  The drive's own noise enters
    the phase; optical signal and optical noise are both multiplied; the rows of a dual-polarisation input get the same phase.  One HIP
    kernel (``ssfm_pm``); a scalar drive is spread over the grid."""
    t0 = time.time()
    op_input, grid, back = _adopt(op_input, "optical_signal")
    if not isinstance(op_input, optical_signal):
        raise TypeError("`op_input` must be of type 'optical_signal'.")
    if isinstance(el_input, electrical_signal) or type(el_input).__name__ == "electrical_signal":
        el_input = _adopt(el_input, "electrical_signal")[0]
    else:
        el_input = electrical_signal(el_input)
    if el_input.ndim > 1:
        raise ValueError("`el_input` must be a scalar or 1D-array.")
    raw_s, raw_n = op_input._raw("signal"), op_input._raw("noise")
    raw_v, raw_vn = el_input._raw("signal"), el_input._raw("noise")
    dev = default_device() if device is None else int(device)
    shape = tuple(raw_s.shape)
    n, n_pol = _rows(shape)
    cplx = any(a is not NULL and a.dtype.kind == "c" for a in (raw_v, raw_vn))
    vdt = np.complex128 if cplx else np.float64

    def drive(a):
        if a is NULL:
            return None
        if _on_device(a) and tuple(a.shape) == (n,) and a.dtype == vdt:
            return _dev_array(a, vdt, dev)
        host = a.to_host() if _on_device(a) else np.asarray(a)
        return _lib.DeviceArray.from_host(np.broadcast_to(host, (n,)), vdt, dev)     # ValueError when the lengths disagree
    v, vn = drive(raw_v), drive(raw_vn)
    sig = _dev_array(raw_s, np.complex128, dev)
    noi = None if raw_n is NULL else _dev_array(raw_n, np.complex128, dev)
    out_s = _lib.DeviceArray(shape, np.complex128, dev)
    out_n = None if noi is None else _lib.DeviceArray(shape, np.complex128, dev)
    _lib.api.ssfm_pm(dev, out_s, out_n, sig, noi, n_pol, n, v, vn, int(cplx), float(Vpi))
    output = _wrap_out(optical_signal, out_s, NULL if out_n is None else out_n, n_pol=op_input.n_pol)
    output.execution_time = time.time() - t0
    return back(output)


# ------------------------------------------------------------------ ADC (csrc/eye.hip)
def _shortest_int_device(x: "_lib.DeviceArray", percent: float, dev: int):
    """``utils.shortest_int(x, percent)`` of a real float64 device array: sorted copy, shortest window of ``int(n percent / 100)`` lags."""
    n = x.size
    lag = int(n * percent / 100)
    if lag < 1:
        raise ValueError(f"Computed lag ({lag}) must be at least 1. The provided percent ({percent}%) is too small for the length of x ({n}). "
                         f"Choose a larger percent value (at least {100 / n:.4f}%).")
    if n > _EYE_MAX_N:
        raise ValueError(f"shortest_int on the device takes up to 2^21 samples, got {n} (there is no CPU fallback)")
    out = np.zeros(2)
    _lib.api.ssfm_shortest_int(dev, x, n, float(percent), _lib._ptr(out))
    return float(out[0]), float(out[1])


def ADC(input, fs: float = None, n: int = 8, otype: str = "v", *, device=None) -> electrical_signal:
    """Analog-to-digital converter (reference ``devices.py:1558-1632``): the signal, optionally ``scipy.signal.resample``-d to ``fs``,
    quantised to ``2^n - 1`` steps between the ends of its shortest 99.99 % interval (``np.round``: half to even).  ``otype='n'``: int64
    codes; ``'v'``: the codes back in volts.  Everything stays on the device (real signals).

    The noise is not quantised: the reference reads ``electrical_signal(input).signal``, and for an ``electrical_signal`` input that is its
    signal without the noise (the output has no noise either)."""
    t0 = time.time()
    input, grid, back = _adopt(input, "electrical_signal")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    if otype not in ("v", "n"):
        raise ValueError("`otype` must be 'v' or 'n'.")
    raw = input._raw("signal")
    if raw.dtype.kind == "c":
        raise TypeError("ADC on the device quantises real signals (got a complex one)")
    dev = default_device() if device is None else int(device)
    size = input.size
    x = _real_sum_device(electrical_signal.from_device(raw) if _on_device(raw) else electrical_signal(raw), size, 0, dev)
    if fs is not None:
        x = _resample_device(x, int(size * fs / grid.fs), dev)
    vmin, vmax = _shortest_int_device(x, 99.99, dev)
    levels = 2 ** int(n) - 1
    out = _lib.DeviceArray((x.size,), np.float64 if otype == "v" else np.int64, dev)
    _lib.api.ssfm_adc_quantize(dev, x, x.size, vmin, vmax, levels, int(otype == "v"), out)
    output = _wrap_out(electrical_signal, out, NULL)
    output.execution_time = time.time() - t0
    return back(output)


# ------------------------------------------------------------------ FBG (csrc/fbg.hip)
_FBG_APODIZATIONS = {"uniform": 0, "rcos": 1, "gaussian": 2, "parabolic": 3}
_FBG_CUSTOM = 4
_FBG_APO_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_void_p)


def _si(x, unit="s", k=1):
    """The engineering-prefix formatting of the reference's ``utils.si`` (its bands, its 'T' band scaled by 1e-9, None below 1e-15)."""
    bands = ((1e12, float("inf"), 1e-9, "T"), (1e9, 1e12, 1e-9, "G"), (1e6, 1e9, 1e-6, "M"), (1e3, 1e6, 1e-3, "k"), (1, 1e3, 1, ""),
             (1e-3, 1, 1e3, "m"), (1e-6, 1e-3, 1e6, "μ"), (1e-9, 1e-6, 1e9, "n"), (1e-12, 1e-9, 1e12, "p"), (1e-15, 1e-12, 1e15, "f"))
    for lo, hi, scale, prefix in bands:
        if lo <= x < hi:
            return f"{x * scale if scale != 1 else x:.{k}f} {prefix}{unit}"
    if x == 0:
        return f"{x:.{k}f} {unit}"
    return None


def _fbg_design(neff, v, landa_D, fc, kL, L, N, dneff, vdneff):
    """The grating design of the reference (devices.py:1933-2015): -> (landa_D, L, dneff, vdneff), with its ValueErrors."""
    c = _C_LIGHT
    pi = np.pi

    def length_from(by_kl):                                 # kL first, then N, else the given L
        if kL:
            return by_kl()
        if N:
            return N * landa_D / (2 * neff)
        return L

    if fc:
        if dneff:
            if not (L or kL or N):
                raise ValueError("If `fc` and `dneff` are specified, `L`, `kL` or `N` must be specified.")
            landa_D = 1 / (1 + dneff / neff) * c / fc
            vdneff = dneff * v
            L = length_from(lambda: kL / (pi * dneff * v / landa_D))
        elif vdneff:
            if not (L or kL or N):
                raise ValueError("If `fc` and `vdneff` are specified, `L`, `kL` or `N` must be specified.")
            landa_D = c / fc
            dneff = 0
            L = length_from(lambda: kL / (pi * vdneff / landa_D))
        else:
            raise ValueError("If `fc` is specified, `dneff` or `vdneff` must be specified.")
    elif landa_D:
        if dneff:
            if not (L or kL or N):
                raise ValueError("If `landa_D` and `dneff` are specified, `L`, `kL` or `N` must be specified.")
            vdneff = dneff * v
            L = length_from(lambda: kL / (pi * vdneff / landa_D))
        elif vdneff:
            if not (L or kL or N):
                raise ValueError("If `landa_D` and `vdneff` are specified, `L`, `kL` or `N` must be specified.")
            dneff = 0
            L = length_from(lambda: kL / (pi * vdneff / landa_D))
        elif kL:
            if not (L or N):
                raise ValueError("If `landa_D` and `kL` are specified, `L` or `N` must be specified.")
            if N:
                L = N * landa_D / (2 * neff)
            vdneff = kL * landa_D / (pi * L)
            dneff = vdneff / v
        else:
            raise ValueError("If `landa_D` is specified, `dneff`, 'vdneff' or `kL` must be specified.")
    else:
        raise ValueError("Either `fc` or `landa_D` must be specified.")
    return landa_D, L, dneff, vdneff


def _unwrapped_phase(H):
    return np.unwrap(np.angle(H))


def _fbg_tau(H, fs, i):
    """``utils.tau_g(H, fs)[i]``: the unwrapped phase difference at i over dw = 2 pi fs / n, in ps (0 at i = 0).  The unwrap runs over
    H[:i + 1] only: its cumulative 2 pi corrections up to i are those of the whole array."""
    if i == 0:
        return 0.0
    ph = _unwrapped_phase(H[:i + 1])
    return float((ph[i] - ph[i - 1]) / (2 * np.pi * fs / H.size) * 1e12)


def _fbg_dispersion(H, fs, f0, i):
    """``utils.dispersion(H, fs, f0)[i]`` in ps/nm."""
    f = np.fft.fftshift(np.fft.fftfreq(H.size, d=1 / fs))
    dlam = np.diff(_C_LIGHT / (f + f0))[0] * 1e9
    ph = _unwrapped_phase(H)
    tau = np.diff(ph, prepend=ph[0]) / (2 * np.pi * fs / H.size) * 1e12
    return np.diff(tau, prepend=tau[0])[i] / dlam


def _fbg_report(H, ic, δλ, fc, Λ, N, L, vdneff, kL, F, fs, print_params):
    """The bandwidth report of devices.py:2096-2150 on the host copy of H (fftshift order): its warnings, and the parameter block when
    ``print_params``.  The warnings need only ``find_peaks``; ``peak_widths`` runs when the block is printed."""
    from scipy import signal as sg
    c, pi = _C_LIGHT, np.pi
    y = np.abs(H)
    peaks, _ = sg.find_peaks(y)
    H_max = y[ic]
    if (y > 0.5).all():
        warnings.warn("Bandwidth of the grating is too large for current sampling rate (`fs`). Consider increasing `fs`.")
        bandwith_str = f' - Δf = >{_si(fs, "Hz")} (Δλ = >{_si(fs * c / fc ** 2, "m")})'
    elif len(peaks):
        bandwith_str = None
        if print_params:                                    # (peak_widths only feeds the printed line: seconds for 10^4 sidelobe peaks)
            widths = sg.peak_widths(y, peaks)
            BW_λ = widths[0].max() * δλ
            BW_f = fc ** 2 * BW_λ / c
            bandwith_str = f' - Δf = {_si(BW_f, "Hz")} (Δλ = {_si(BW_λ, "m")})'
    else:
        warnings.warn("No peaks found in the reflectivity of the grating.")
        bandwith_str = " - Δf = -- GHz (Δλ = -- nm)"

    if print_params:
        D = _fbg_dispersion(H, fs, fc, ic)
        with np.errstate(divide="ignore"):
            loss = -(10 * np.log10(H_max ** 2))
        print("\n*** Fiber Bragg Grating Features ***")
        print(f' - Λ = {_si(Λ, "m")}')
        print(f" - N = {N}")
        print(f' - L = {_si(L, "m")}')
        print(f' - λc = {_si(c / fc, "m", 4)}')
        print(bandwith_str)
        print(f" - ρo = {y.max():.2f}")
        print(f" - loss = {loss:.1f} dB")
        print(f" - vδneff = {vdneff:.1e}")
        print(f" - kL = {kL:.1f}")
        print(f" - D(λc) = {D:.1f} ps/nm")
        if F:
            print(f" - F = {F:.1f}")
            print(f' - ΔΛ = {_si(np.abs(Λ * F / (2 * pi * N)), "m")}')
        print("************************************\n")


def FBG(input: optical_signal, neff: float = 1.45, v: float = 1.0, landa_D: float = None, fc: float = None, kL: float = None, L: float = None,
        N: int = None, dneff: float = None, vdneff: float = None, apodization="uniform", F: float = 0, print_params: bool = True,
        filtfilt: bool = True, retH: bool = False, *, rtol: float = 1e-3, atol: float = 1e-6, device=None):
    """Fibre Bragg grating (reference ``devices.py:1894-2173``): the reflection transfer function H of the coupled-mode equations, solved on
    the GPU with the step control of ``scipy.integrate.solve_ivp(method="RK45")`` (csrc/fbg.hip), applied to signal and noise separately as
    ``ifft(fft(x) ifftshift(H))``.  ``rtol`` / ``atol`` (keyword-only extension) are solve_ivp's, with its defaults.

    The built-in apodizations run on the device; a callable apodization is evaluated on the host at the six stage positions of every
    attempted step (one host wait per attempted step instead of one per 32).  H is read back once per call for the bandwidth report and its
    warnings (``scipy.signal.find_peaks``).  A dual-polarisation input gets the same H on both rows (the reference fails on it).  With
    ``retH``: ``(output, H)``, H after the ``filtfilt`` correction, on the host; ``execution_time`` is then not set, as in the reference.
    ``FBG.last_steps`` / ``last_attempts`` / ``last_waits``: accepted and attempted RK45 steps and blocking host waits of the last solve."""
    t0 = time.time()
    input, grid, back = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if 2 * input.size - 1 > (1 << hi):                     # the filtering's chirp-z plan (M >= 2n - 1): checked before the solve
        raise ValueError(f"FBG on the device filters up to 2^{hi - 1} samples, got {input.size} (there is no CPU fallback)")
    c, pi = _C_LIGHT, np.pi
    landa_D, L, dneff, vdneff = _fbg_design(neff, v, landa_D, fc, kL, L, N, dneff, vdneff)

    λ_D = landa_D
    Λ = λ_D / (2 * neff)
    λc = (1 + dneff / neff) * λ_D
    fc = c / λc
    w = np.fft.fftshift(np.fft.fftfreq(input.size, grid.dt) * 2 * np.pi)          # input.w(shift=True)
    λ = 2 * pi * c / (w + 2 * pi * grid.f0)
    δλ = λ[1] - λ[0]
    N = int(L / Λ)
    kL = pi / λ_D * vdneff * L
    δ = 2 * pi * neff * (1 / λ - 1 / λ_D) * L
    s = 2 * pi * dneff / λ * L
    k = pi * vdneff / λ * L
    δ, s, k = (np.ascontiguousarray(np.broadcast_to(a, λ.shape), dtype=np.float64) for a in (δ, s, k))

    apo_fn, user_apo = None, None
    if isinstance(apodization, str) and apodization in _FBG_APODIZATIONS:
        apo = _FBG_APODIZATIONS[apodization]
    elif callable(apodization):
        apo, user_apo = _FBG_CUSTOM, apodization
    elif isinstance(apodization, str):
        warnings.warn("Apodization function not recognized. Using uniform apodization.")
        apo = _FBG_APODIZATIONS["uniform"]
    else:
        raise ValueError("Apodization must be a string or a function.")
    failure = []
    if user_apo is not None:
        def _cb(z, count, p, _user):
            try:
                for j in range(count):
                    p[j] = float(user_apo(np.float64(z[j])))
                return 0
            except BaseException as exc:                    # noqa: BLE001 -- re-raised below, after the solve returns
                failure.append(exc)
                return 1
        apo_fn = _FBG_APO_FN(_cb)

    dev = default_device() if device is None else int(device)
    n = λ.size
    Hd = _lib.DeviceArray((n,), np.complex128, dev)
    info = (_lib._I64 * 3)()
    rc = _lib.load().ssfm_fbg_solve(dev, n, _lib._ptr(δ), _lib._ptr(s), _lib._ptr(k), float(F), apo, float(rtol), float(atol), apo_fn, None, Hd, info)
    if failure:
        raise failure[0]
    _lib._check(rc, "ssfm_fbg_solve")
    FBG.last_steps, FBG.last_attempts, FBG.last_waits = int(info[0]), int(info[1]), int(info[2])

    H = Hd.to_host()
    ic = int(np.argmin(np.abs(λ - c / fc)))
    _fbg_report(H, ic, δλ, fc, Λ, N, L, vdneff, kL, F, grid.fs, print_params)

    tau = _fbg_tau(H, grid.fs, ic) if filtfilt else 0.0
    Hnat = _lib.DeviceArray((n,), np.complex128, dev)
    _lib.api.ssfm_fbg_delay(dev, Hd, Hnat, n, float(grid.dt), tau, int(bool(filtfilt)))

    # ifft(fft(x) ifftshift(H)) on the chirp-z engine (any length)
    raw_s, raw_n = input._raw("signal"), input._raw("noise")
    outs = _chirpz_transfer([raw_s] if raw_n is NULL else [raw_s, raw_n], Hnat, False, dev)
    output = _wrap_out(optical_signal, outs[0], outs[1] if len(outs) > 1 else NULL, n_pol=input.n_pol)
    if retH:
        return back(output), Hd.to_host()
    output.execution_time = time.time() - t0
    return back(output)


FBG.last_steps = FBG.last_attempts = FBG.last_waits = None
