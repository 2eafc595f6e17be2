"""M-ary pulse-position modulation, reference ``opticomlib/ppm.py``: ``PPM_ENCODER``, ``PPM_DECODER``, ``HDD``, ``SDD``, ``THRESHOLD_EST``,
``DSP``, ``BER_analizer`` and ``theory_BER``, with the reference's names, arguments, defaults and exceptions.

The bit and slot work runs on the GPU (csrc/ppm.hip) and its results stay in GPU memory: the encoder, the decoder, the per-symbol slot
decision (argmax for ``SDD``, ``> rth`` with the ON count for the hard decision) and ``HDD``'s choice for the symbols that do not hold
exactly one ON slot.  ``HDD`` draws that choice as the reference does -- ``np.random.randint(M)`` for each empty symbol in ascending order,
then ``np.random.choice`` among the ON slots of each multi-ON symbol in ascending order, from NumPy's global generator -- so it is seed for
seed the reference's (``rng="numpy"``, the default); the host makes only those draws.  ``rng="device"`` draws on the GPU instead
(Philox4x32-10 keyed by the device seed of :func:`~opticomlib_amd.devices.device_rng_seed` and the symbol index), with no host wait.
``THRESHOLD_EST``, the estimator and ``theory_BER`` are host scalars, as in the reference.

Unlike the reference, ``HDD`` does not write into the caller's array (the reference's ``output = input[:]`` is a view of it).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Literal

import numpy as np
from scipy.integrate import quad
from scipy.special import erfc

from . import _lib
from .devices import _DEVICE_RNG, GET_EYE, _adopt, _check_rng, _dev_array, default_device
from .typing import NULL, binary_sequence, electrical_signal, eye

__all__ = ["PPM_ENCODER", "PPM_DECODER", "HDD", "SDD", "THRESHOLD_EST", "DSP", "BER_analizer", "theory_BER"]

_Array_Like = (list, tuple, np.ndarray)
_MAX_M = 1 << 16                                          # csrc/ppm.hip


def _Q(x):
    return 0.5 * erfc(x / 2 ** 0.5)


def _check_pow2(M):
    if not M & (M - 1) == 0:
        raise ValueError("`M` must be a power of 2.")
    if not 2 <= M <= _MAX_M:
        raise ValueError(f"`M` must lie in 2 ... 2^16 on the device, got {M}")


def _bits(input) -> "_lib.DeviceArray | np.ndarray":
    """The reference's accepted bit inputs (str, list, tuple, ndarray, binary_sequence) as a device array as they lie, or host uint8 0 / 1."""
    if isinstance(input, binary_sequence):
        raw = input._raw()
        if isinstance(raw, _lib.DeviceArray):
            return raw
        a = np.asarray(raw) != 0
    elif isinstance(input, _lib.DeviceArray):
        return input
    elif isinstance(input, str):
        a = np.asarray(binary_sequence(input).data) != 0
    elif isinstance(input, _Array_Like):
        a = np.array(input, dtype=bool).ravel()
    else:
        raise TypeError("`input` must be of type (str, list, tuple, ndarray, binary_sequence)")
    return np.ascontiguousarray(a, dtype=np.uint8)


def _on(bits, dev: int) -> "_lib.DeviceArray":
    return _dev_array(bits, np.uint8, dev)


def _bits_device(input, dev: int) -> "_lib.DeviceArray":
    b = _bits(input)
    return _on(b, dev) if b.size else b


def _wrap(arr, t0):
    out = binary_sequence.from_device(arr) if isinstance(arr, _lib.DeviceArray) else binary_sequence(arr)
    out.execution_time = time.time() - t0
    return out


def _device(device) -> int:
    return default_device() if device is None else int(device)


def PPM_ENCODER(input, M: int, *, device=None) -> binary_sequence:
    """PPM encoder (reference ``ppm.py:27-80``): each group of ``k = int(log2(M))`` bits, MSB first, is the ON slot of an ``M``-slot
    symbol; the input is truncated to ``len // k * k`` bits.  The slots stay in GPU memory (``DAC`` takes them from there)."""
    t0 = time.time()
    bits = _bits(input)
    if not 2 <= M <= _MAX_M:
        raise ValueError(f"`M` must lie in 2 ... 2^16, got {M}")
    k = int(np.log2(M))
    nsym = bits.size // k
    if nsym == 0:
        return _wrap(np.empty(0, np.uint8), t0)
    dev = _device(device)
    bits = _on(bits, dev)
    out = _lib.DeviceArray((nsym * M,), np.uint8, dev)
    _lib.api.ssfm_ppm_encode(dev, bits, nsym, int(M), out)
    return _wrap(out, t0)


def PPM_DECODER(input, M: int, *, device=None) -> binary_sequence:
    """PPM decoder (reference ``ppm.py:83-125``), for any input: every ON slot at position ``p`` emits the ``log2(M)`` bits of ``p % M``, so
    a symbol without an ON slot emits nothing and one with two emits two groups.  One host read: the output length."""
    t0 = time.time()
    slots = _bits(input)
    _check_pow2(M)
    if slots.size == 0:
        return _wrap(np.empty(0, np.uint8), t0)
    dev = _device(device)
    slots = _on(slots, dev)
    n_bits = _lib._I64(0)
    _lib.api.ssfm_ppm_decode(dev, slots, slots.size, int(M), None, 0, C.byref(n_bits))
    if n_bits.value == 0:
        return _wrap(np.empty(0, np.uint8), t0)
    out = _lib.DeviceArray((n_bits.value,), np.uint8, dev)
    _lib.api.ssfm_ppm_decode(dev, slots, slots.size, int(M), out, n_bits.value, None)
    return _wrap(out, t0)


def _scratch(nbytes: int, dev: int) -> "_lib.DeviceArray":
    return _lib.DeviceArray((max(int(nbytes), 1),), np.uint8, dev)


def _decide(x, noise, is_u8: bool, start: int, step: int, nsym: int, M: int, hard: bool, thr: float, want: str, rng: str, dev: int):
    """The per-symbol decision of ``nsym`` symbols of ``M`` slots read at ``x[start + q step]`` (+ ``noise``), then (hard) ``HDD``'s choice for
    the symbols without exactly one ON slot.  ``want``: 'bits' (the decoded ``k`` bits per symbol) or 'slots' (one-hot symbols)."""
    k = int(np.log2(M))
    out = _lib.DeviceArray((nsym * (k if want == "bits" else M),), np.uint8, dev)
    bits, slots = (out, None) if want == "bits" else (None, out)
    counts = _scratch(4 * nsym, dev) if hard else None
    _lib.api.ssfm_ppm_decide(dev, x, noise, int(is_u8), start, step, nsym, M, int(hard), float(thr), bits, slots, counts)
    if not hard:
        return out
    resolve = lambda idx, draws, n_list, seed, stream: _lib.api.ssfm_ppm_resolve(
        dev, x, noise, int(is_u8), start, step, nsym, M, float(thr), counts, idx, draws, n_list, seed, stream, bits, slots)
    if rng == "device":
        _DEVICE_RNG["stream"] += 1
        resolve(None, None, 0, _DEVICE_RNG["seed"] & (2 ** 64 - 1), _DEVICE_RNG["stream"])
        return out
    idx, cnt, nf = _scratch(4 * nsym, dev), _scratch(4 * nsym, dev), _lib._I64(0)
    _lib.api.ssfm_ppm_faulty(dev, counts, nsym, idx, cnt, C.byref(nf))
    nf = int(nf.value)
    if nf:
        c = np.empty(nf, np.int32)
        _lib.api.ssfm_device_copy(dev, _lib._ptr(c), cnt, c.nbytes, _lib.COPY_D2H)
        draws = _hdd_draws(c, M)
        d = _lib.DeviceArray.from_host(draws.view(np.uint8), np.uint8, dev)
        resolve(idx, d, nf, 0, 0)
    return out


def _hdd_draws(counts: np.ndarray, M: int) -> np.ndarray:
    """The reference's draws (``ppm.py:184-190``) for the faulty symbols' ON counts in ascending symbol order: ``randint(M)`` for every
    empty symbol first, then the index among the ON slots for every multi-ON symbol (``choice(j)`` takes ``j[randint(len(j))]``, and
    ``randint`` over an array of bounds draws as the loop of scalar calls does)."""
    draws = np.zeros(counts.size, np.int32)
    empty = counts == 0
    if empty.any():
        draws[empty] = np.random.randint(M, size=int(empty.sum()))
    if (~empty).any():
        draws[~empty] = np.random.randint(0, counts[~empty].astype(np.int64))
    return draws


def HDD(input, M: int, *, device=None, rng: str = "numpy") -> binary_sequence:
    """Hard decision decoder (reference ``ppm.py:128-195``): a symbol without an ON slot gets one at random, a symbol with more than one
    keeps one of them at random, the others are kept.  ``rng="numpy"``: the reference's draws from NumPy's global generator, seed for seed;
    ``rng="device"``: Philox draws on the GPU.  Raises ``ValueError`` if ``M`` is not a power of 2 or the length is not a multiple of ``M``."""
    t0 = time.time()
    _check_rng(rng)
    slots = _bits(input)
    _check_pow2(M)
    if slots.size % M != 0:
        raise ValueError("The length of `input` must be a multiple of `M`.")
    if slots.size == 0:
        return _wrap(np.empty(0, np.uint8), t0)
    dev = _device(device)
    slots = _on(slots, dev)
    return _wrap(_decide(slots, None, True, 0, 1, slots.size // M, M, True, 0.5, "slots", rng, dev), t0)


def _samples(input, grid, dev):
    """(signal, noise or None) of a real electrical signal or array as float64 device arrays, and the sampling grid."""
    input, g, _ = _adopt(input, "electrical_signal")
    grid = g if grid is None else grid
    if isinstance(input, _Array_Like):
        input = electrical_signal(np.asarray(input))
    if not isinstance(input, electrical_signal):
        raise TypeError("`input` must be of type `electrical_signal` or `Array_Like`.")
    sig, noi = input._raw("signal"), input._raw("noise")
    for a in (sig, noi):
        if a is not NULL and np.iscomplexobj(np.empty(0, a.dtype)):
            raise TypeError("the PPM decisions take a real signal (PD output): the reference would compare complex values lexicographically")
    return _dev_array(sig, np.float64, dev), (None if noi is NULL else _dev_array(noi, np.float64, dev)), input.size, grid


def SDD(input, M: int, *, device=None) -> binary_sequence:
    """Soft decision decoder (reference ``ppm.py:198-258``): ``np.argmax`` over the ``M`` slot samples ``(signal + noise)[sps//2 :: sps]`` of
    each symbol (the first index wins a tie, NaN is the maximum), as one-hot symbols in GPU memory.  Real signals only (``TypeError``)."""
    t0 = time.time()
    _check_pow2(M)
    dev = _device(device)
    x, noise, size, grid = _samples(input, None, dev)
    sps = int(grid.sps)
    if size % (M * sps) != 0:
        raise ValueError("The length of `input` must be a multiple of `M*sps`.")
    return _wrap(_decide(x, noise, False, sps // 2, sps, size // sps // M, M, False, 0.0, "slots", "numpy", dev), t0)


def _is_eye(e) -> bool:
    return isinstance(e, eye) or type(e).__name__ == "eye"


def THRESHOLD_EST(eye_obj, M: int):
    """Decision threshold for M-PPM (reference ``ppm.py:261-306``): the minimiser of ``1 - Q((r - mu1)/s1) (1 - Q((r - mu0)/s0))^(M-1)``
    over ``linspace(mu0, mu1, 1000)``."""
    if not M & (M - 1) == 0:
        raise ValueError("`M` must be a power of 2.")
    if not _is_eye(eye_obj):
        raise TypeError("`eye_obj` must be of type `eye`.")
    mu0, mu1, s0, s1 = eye_obj.mu0, eye_obj.mu1, eye_obj.s0, eye_obj.s1
    r = np.linspace(mu0, mu1, 1000)
    return r[np.argmin(1 - _Q((r - mu1) / s1) * (1 - _Q((r - mu0) / s0)) ** (M - 1))]


def DSP(input, M: int, decision: Literal["hard", "soft"] = "hard", threshold=None, *, device=None, rng: str = "numpy"):
    """PPM receiver (reference ``ppm.py:309-416``), on the GPU: ``'soft'`` is ``SDD`` then the decoder; ``'hard'`` takes ``threshold`` or,
    without it, ``GET_EYE(x, nslots=8192)``'s ``threshold`` or else :func:`THRESHOLD_EST`, then ``(signal + noise)[sps//2 :: sps] > rth``,
    ``HDD`` and the decoder.  Returns the received bits (a ``binary_sequence`` in GPU memory), as the reference does; the eye (hard decision
    with an estimated threshold) and the threshold used are attached to it as ``.eye_obj`` and ``.rth``.

    Deviation: the reference's ``GET_EYE`` runs sklearn's ``KMeans``, which takes draws from NumPy's global generator before ``HDD`` does;
    this ``GET_EYE`` takes none.  So with an estimated threshold and ``rng="numpy"``, the draws for the faulty symbols differ from the
    reference's for the same seed; with ``threshold=`` given they are the same.  Complex signals raise ``TypeError``."""
    t0 = time.time()
    _check_rng(rng)
    input, grid, _ = _adopt(input, "electrical_signal")
    if not isinstance(input, (electrical_signal,) + _Array_Like):
        raise TypeError("`input` must be of type `electrical_signal` or `Array_Like`.")
    if not isinstance(input, electrical_signal):
        input = electrical_signal(input)
    sps = int(grid.sps)
    if input.size < sps:
        raise ValueError("`input` must have at least `sps` samples.")
    _check_pow2(M)
    dev = _device(device)
    kind = decision.lower()
    if kind not in ("hard", "soft"):
        raise ValueError('`decision` must be "hard" or "soft"')
    x, noise, size, _ = _samples(input, grid, dev)
    eye_obj, rth = None, None
    if kind == "hard":
        if threshold is not None:
            rth = threshold
        else:
            eye_obj = GET_EYE(input, nslots=8192, device=dev, _grid=grid)
            rth = eye_obj.threshold if eye_obj.threshold is not None else THRESHOLD_EST(eye_obj, M)
        nslot = len(range(sps // 2, size, sps))
        if nslot % M != 0:
            raise ValueError("The length of `input` must be a multiple of `M`.")
        out = _decide(x, noise, False, sps // 2, sps, nslot // M, M, True, float(rth), "bits", rng, dev) if nslot else np.empty(0, np.uint8)
    else:
        if size % (M * sps) != 0:
            raise ValueError("The length of `input` must be a multiple of `M*sps`.")
        out = _decide(x, noise, False, sps // 2, sps, size // sps // M, M, False, 0.0, "bits", rng, dev)
    output = _wrap(out, t0)
    output.eye_obj, output.rth = eye_obj, rth
    return output


def BER_analizer(mode: Literal["counter", "estimator"], *, device=None, **kwargs):
    """Bit error rate (reference ``ppm.py:419-505``): ``'counter'`` compares ``Rx`` with ``Tx[:Rx.size]`` on the GPU; ``'estimator'``
    evaluates the hard (``Q`` at the threshold of :func:`THRESHOLD_EST`) or soft (``scipy.integrate.quad``) symbol error probability of
    ``eye_obj`` and scales it by ``M / 2 / (M - 1)``."""
    if mode.lower() == "counter":
        Tx, Rx = kwargs.get("Tx", None), kwargs.get("Rx", None)
        if Tx is None or Rx is None:
            raise KeyError("`Tx` and `Rx` are required arguments for `mode='counter'`.")
        dev = _device(device)
        rx, tx = _bits_device(Rx, dev), _bits_device(Tx, dev)
        n = rx.size
        assert min(tx.size, n) == n, "Error: `Tx` and `Rx` must have the same length."
        if n == 0:
            return np.float64(np.nan)
        errs = _lib._I64(0)
        _lib.api.ssfm_device_count_diff(dev, tx, rx, n, C.byref(errs))
        return errs.value / n
    elif mode.lower() == "estimator":
        eye_obj, M = kwargs.get("eye_obj", None), kwargs.get("M", None)
        decision = kwargs.get("decision", "soft")
        if eye_obj is None or M is None:
            raise KeyError("`eye_obj` and `M` are required arguments for `mode='estimator'`.")
        if not M & (M - 1) == 0:
            raise ValueError("`M` must be a power of 2.")
        if decision.lower() not in ["hard", "soft"]:
            raise ValueError("`decision` must be 'hard' or 'soft'.")
        I1, I0, s1, s0 = eye_obj.mu1, eye_obj.mu0, eye_obj.s1, eye_obj.s0
        um = THRESHOLD_EST(eye_obj, M)
        if decision == "hard":
            Pe_sym = 1 - _Q((um - I1) / s1) * (1 - _Q((um - I0) / s0)) ** (M - 1)
        elif decision == "soft":
            Pe_sym = 1 - 1 / (2 * np.pi) ** 0.5 * quad(lambda x: (1 - _Q((I1 - I0 + s1 * x) / s0)) ** (M - 1) * np.exp(-x ** 2 / 2), -np.inf, np.inf)[0]
        return M / 2 / (M - 1) * Pe_sym
    else:
        raise ValueError("Invalid mode. Use `counter` or `estimator`.")


def theory_BER(mu1, s0, s1, M: int, decision: Literal["soft", "hard"] = "soft"):
    """Theoretical bit error probability of M-PPM (reference ``ppm.py:508-577``), vectorised over ``mu1``, ``s0`` and ``s1`` as the
    reference does: ``M / 2 / (M - 1)`` times the symbol error probability, a ``quad`` integral (soft) or the minimum over
    ``linspace(0, mu1, 1000)`` (hard)."""
    if not M & (M - 1) == 0:
        raise ValueError("`M` must be a power of 2.")
    if decision == "soft":
        fun = np.vectorize(lambda mu1, s0, s1, M: 1 - 1 / (2 * np.pi) ** 0.5 * quad(
            lambda x: (1 - _Q((mu1 + s1 * x) / s0)) ** (M - 1) * np.exp(-x ** 2 / 2), -np.inf, np.inf)[0])
    elif decision == "hard":
        @np.vectorize
        def fun(mu1_, s0_, s1_, M_):
            r = np.linspace(0, mu1_, 1000)
            return np.min(1 - _Q((r - mu1_) / s1_) * (1 - _Q(r / s0_)) ** (M_ - 1))
    else:
        raise ValueError("`decision` must be `soft` or `hard`.")
    return fun(mu1, s0, s1, M) * 0.5 * M / (M - 1)
