"""The coherent receiver for square QAM: ``QAM_ENCODER``, ``QAM_DECODER``, ``SHAPE``, ``CPR``, ``DSP``, ``EVM`` and ``BER``.  The reference library
has no counterpart (its receivers -- ``ook``, ``ppm``, ``lab`` -- detect intensity); this module closes the chain
``bits -> QAM -> FIBER -> DBP / DM -> carrier recovery -> bits -> BER`` that the propagator's polarisation-multiplexed fields ask for.

Everything runs on the GPU (csrc/coherent.hip) and stays in GPU memory: device-resident bits, symbols and fields are used where they lie, host
inputs are uploaded once, results come back as device-resident ``binary_sequence`` / ``electrical_signal`` / ``optical_signal`` objects or
``DeviceArray`` s.  There is no CPU fallback, and every argument error is raised before the library is loaded.

Constellation: ``M`` in 4, 16, 64, 256; ``k = log2 M`` bits per symbol, MSB first, the first ``k / 2`` the in-phase and the last ``k / 2`` the
quadrature level; a level's bits read as binary-reflected Gray code, level ``g`` of ``L = sqrt(M)`` has the amplitude ``a (2 g - (L - 1))`` with
``a = 1 / sqrt(2 (M - 1) / 3)`` (unit mean power).  ``M = 4`` is ``workloads.prbs_field``'s ``((2 b0 - 1) + 1j (2 b1 - 1)) / sqrt(2)``.  A real
component ``x`` is decided as ``g = clip(floor(x / (2 a) + L / 2), 0, L - 1)``: a value on a boundary takes the upper level, ``+-0`` gives ``L / 2``.

Carrier recovery is the feed-forward blind phase search (Pfau, Hoffmann, Noe, JLT 27(8), 2009), in float64 whatever the input type:
``B = test_phases`` rotations ``phi_b = (b - B / 2) pi / (2 B)``, the squared distance of every rotated symbol to its decision, summed over the
``2 W + 1`` symbols around each symbol (fewer at the record's ends), the first ``b`` of the smallest sum, unwrapped over the quarter turn.  The
search leaves a multiple of ``pi / 2`` undetermined: ``DSP`` resolves it only against ``ref=``.

Out of scope: polarisation demultiplexing or equalisation (CMA) -- a field scrambled by ``FIBER(pmd=...)`` with scattering cannot be received yet
-- timing recovery, frequency-offset estimation, differential coding, non-square constellations, joint phase estimation across polarisations.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib
from .devices import _DAC_SHAPES, _adopt, _gauss_spec, _nrz_spec, _on_device, _rcos_spec, _row_block, _wrap_out, default_device, get_plan
from .ppm import _bits
from .typing import NULL, binary_sequence, electrical_signal, gv, optical_signal

__all__ = ["QAM_ENCODER", "QAM_DECODER", "SHAPE", "CPR", "DSP", "EVM", "BER", "Received", "CPR_TILE"]

CPR_TILE = 256                                     # csrc/coherent_tiles.hpp kTile: symbols of one row a workgroup of the search owns
_ORDERS = {4: (2, 2), 16: (4, 4), 64: (6, 8), 256: (8, 16)}          # M -> (k, L)
_MAX_PHASES, _MAX_WINDOW, _MAX_SYMBOLS = 64, 256, 1 << 26            # csrc/coherent_tiles.hpp
_Array_Like = (list, tuple, np.ndarray)


def _order(M) -> int:
    if M not in _ORDERS:
        raise ValueError(f"`M` must be one of 4, 16, 64, 256 (square QAM), got {M}")
    return int(M)


def _half_spacing(M: int) -> float:
    return 1.0 / math.sqrt(2.0 * (M - 1) / 3.0)


def _check_search(test_phases, window):
    B, W = int(test_phases), int(window)
    if B != test_phases or W != window:
        raise ValueError(f"`test_phases` and `window` must be integers, got {test_phases} and {window}")
    if B % 2 or not 2 <= B <= _MAX_PHASES:
        raise ValueError(f"`test_phases` must be even and lie in 2 ... {_MAX_PHASES}, got {B}")
    if not 0 <= W <= _MAX_WINDOW:
        raise ValueError(f"`window` must lie in 0 ... {_MAX_WINDOW}, got {W}")
    return B, W


def _device(device) -> int:
    return default_device() if device is None else int(device)


def _same_gpu(raw, dev: int):
    if _on_device(raw) and raw.device != dev:
        raise ValueError(f"the record lies on GPU {raw.device}, not on GPU {dev}")


def _record(symbols):
    """A record of one sample per symbol as a host array or a ``DeviceArray``: the signal (+ noise, added where it lies) of a signal object, a
    ``DeviceArray`` or array_like; complex, of shape ``(n,)`` or ``(2, n)``."""
    if isinstance(symbols, (electrical_signal, optical_signal)):
        raw, noi = symbols._raw("signal"), symbols._raw("noise")
        if noi is not NULL:
            if _on_device(raw) or _on_device(noi):
                t = np.result_type(raw.dtype, noi.dtype)
                raw = _as_device(raw, t, (raw if _on_device(raw) else noi).device) + _as_device(noi, t, (raw if _on_device(raw) else noi).device)
            else:
                raw = raw + noi
    elif _on_device(symbols):
        raw = symbols
    elif isinstance(symbols, _Array_Like):
        raw = np.asarray(symbols)
    else:
        raise TypeError("`symbols` must be an `electrical_signal`, an `optical_signal`, a `DeviceArray` or array_like")
    if np.dtype(raw.dtype).kind != "c":
        raise TypeError(f"the coherent receiver takes a complex record, got {np.dtype(raw.dtype)}")
    if raw.ndim not in (1, 2) or (raw.ndim == 2 and raw.shape[0] != 2) or raw.shape[-1] < 1:
        raise ValueError(f"a record has shape (n,) or (2, n) with n >= 1, got {tuple(raw.shape)}")
    if raw.shape[-1] > _MAX_SYMBOLS:
        raise ValueError(f"a record holds at most 2^26 symbols per row, got {raw.shape[-1]}")
    return raw


def _as_device(raw, dtype, dev: int) -> "_lib.DeviceArray":
    """``raw`` on GPU ``dev`` as ``dtype``: where it lies when it is there already, uploaded once when it is a host array."""
    if _on_device(raw):
        _same_gpu(raw, dev)
        return raw if raw.dtype == np.dtype(dtype) else raw.astype(dtype)
    return _lib.DeviceArray.from_host(np.ascontiguousarray(raw, dtype=dtype), None, dev)


def _field(raw, dev: int) -> "_lib.DeviceArray":
    """A complex record for the search: complex64 and complex128 are read as they are, anything else is widened."""
    return _as_device(raw, np.complex64 if np.dtype(raw.dtype) == np.complex64 else np.complex128, dev)


def _wrap_bits(arr, t0) -> binary_sequence:
    out = binary_sequence.from_device(arr)
    out.execution_time = time.time() - t0
    return out


# ------------------------------------------------------------------------------------------------ mapper, decisions, pulse shaping
def QAM_ENCODER(bits, M: int, *, device=None) -> electrical_signal:
    """Square Gray-mapped QAM mapper: ``k = log2(M)`` bits per symbol (a ``binary_sequence`` on the host or in GPU memory, as ``PRBS`` leaves it,
    a string or array_like) become one complex128 sample per symbol, in GPU memory.  A size that is not a multiple of ``k`` raises ``ValueError``."""
    t0 = time.time()
    M = _order(M)
    k = _ORDERS[M][0]
    b = _bits(bits)
    if b.size % k or b.size == 0:
        raise ValueError(f"the number of bits must be a positive multiple of log2(M) = {k}, got {b.size}")
    dev = _device(device)
    b = _as_device(b, np.uint8, dev)
    out = _lib.DeviceArray((b.size // k,), np.complex128, dev)
    _lib.api.ssfm_qam_encode(b, out.size, M, _half_spacing(M), out)
    output = _wrap_out(electrical_signal, out, NULL)
    output.execution_time = time.time() - t0
    return output


def QAM_DECODER(symbols, M: int, *, device=None) -> binary_sequence:
    """Decisions of a one-row record of one sample per symbol: the ``log2(M)`` bits of each symbol's nearest constellation point (the rule of the
    module's head), uint8 in GPU memory."""
    t0 = time.time()
    M = _order(M)
    raw = _record(symbols)
    if raw.ndim != 1:
        raise ValueError(f"QAM_DECODER takes one row of symbols, got shape {tuple(raw.shape)}")
    dev = _device(device)
    z = _as_device(raw, np.complex128, dev)
    out = _lib.DeviceArray((z.size * _ORDERS[M][0],), np.uint8, dev)
    _lib.api.ssfm_qam_decide(z, z.size, M, _half_spacing(M), 0, out, None)
    return _wrap_bits(out, t0)


def _pulse_spec(pulse_shape: str, nsym: int, sps: int, kw: dict):
    """``DAC``'s built-in pulses with its keywords and its ``span`` rule."""
    span = max(4, nsym - 4)
    shape = pulse_shape.lower()
    if shape not in _DAC_SHAPES:
        raise ValueError(f"The parameter `pulse_shape` must be one of the following values {_DAC_SHAPES}")
    if shape == "rcos":
        return _rcos_spec(kw.get("beta", 0.25), span, sps, shape=kw.get("rcos_type", "normal"))
    T = kw.get("T", 1)
    if not isinstance(T, int):
        raise TypeError("The parameter `T` must be an integer.")
    if not 0 < T <= 2 * sps:
        raise ValueError("The parameter `T` must lie in 1 ... 2*sps.")
    if shape == "nrz":
        return _nrz_spec(span, sps, T)
    c, m = kw.get("c", 0.0), kw.get("m", 1)
    if not isinstance(c, (int, float)):
        raise TypeError("The parameter `c` must be a real number.")
    if not isinstance(m, int) or m <= 0:
        raise ValueError("The parameter `m` must be an integer greater than 0.")
    return _gauss_spec(span, sps, T=T, m=m, c=c)


def SHAPE(symbols, pulse_shape: str = "rcos", *, device=None, **kw) -> electrical_signal:
    """Pulse shaping of complex symbols: ``gv.sps`` samples per symbol, the symbols zero-stuffed at offset ``sps // 2`` and convolved with one of
    ``DAC``'s pulses (``'nrz'`` with ``T``; ``'gaussian'`` with ``T``, ``m``, ``c``; ``'rcos'`` with ``beta``, ``rcos_type``), which spans
    ``max(4, symbols - 4)`` symbols as there.  One FFT convolution per real component on a complex128 plan, as ``DAC`` runs it; the result is a
    complex128 ``electrical_signal`` in GPU memory.  ``LASER(...) * SHAPE(...)`` is the transmitter.  A complex pulse (a chirped Gaussian) is not
    taken: ``ValueError``."""
    t0 = time.time()
    raw = _record(symbols)
    if raw.ndim != 1:
        raise ValueError(f"SHAPE takes one row of symbols, got shape {tuple(raw.shape)}")
    sps, nsym = int(gv.sps), int(raw.shape[-1])
    spec, cplx = _pulse_spec(pulse_shape, nsym, sps, kw)
    if cplx and kw.get("c", 0.0) != 0.0:
        raise ValueError("SHAPE convolves each real component with a real pulse: a chirped Gaussian (`c` != 0) is not taken")
    n, taps = nsym * sps, spec[1]
    M = 1 << max(8, (n + taps - 2).bit_length())
    dev = _device(device)
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    if M > (1 << hi):
        raise ValueError(f"SHAPE: {nsym} symbols x {sps} samples with a {taps}-tap pulse exceed the device path (2^{hi} points)")
    z = _as_device(raw, np.complex128, dev)
    parts = [_lib.DeviceArray((nsym,), np.float64, dev) for _ in range(2)]
    _lib.api.ssfm_signal_split(z, nsym, parts[0], parts[1])
    off = ((taps - 1) // 2) * 16                            # 'same': centred with respect to the full output
    shaped = [_lib.DeviceArray((n,), np.float64, dev) for _ in range(2)]
    plan = get_plan(M, 1, _lib.C128, dev)
    with plan.lock:
        plan.load_pulse(*spec)
        plan.table_from_field(0)                            # slot 0 <- fft(pulse)
        for part, out in zip(parts, shaped):
            plan.load_symbols(part, sps)                    # field <- the component, zero-stuffed at sps // 2
            plan.apply_table(0)
            plan.synchronize()
            _lib.api.ssfm_signal_split(plan.field_device_ptr + off, n, out, None)
    out = _lib.DeviceArray((n,), np.complex128, dev)
    _lib.api.ssfm_signal_pack(shaped[0], shaped[1], n, out)
    output = _wrap_out(electrical_signal, out, NULL)
    output.execution_time = time.time() - t0
    return output


# ------------------------------------------------------------------------------------------------ blind phase search
def _phase_table(B: int):
    """``exp(-i phi_b)``, ``phi_b = (b - B / 2) pi / (2 B)``, as interleaved doubles, and the phase step; formed here in double, sent with the call."""
    step = np.pi / (2 * B)
    t = np.exp(-1j * ((np.arange(B) - B / 2) * step))
    return np.ascontiguousarray(t).view(np.float64), float(step)


def _row_power(x, rows: int, n: int, start: int, step: int, pitch: int) -> np.ndarray:
    out = (C.c_double * rows)()
    _lib.api.ssfm_cpr_power(x, int(x.dtype == np.complex64), rows, n, start, step, pitch, out)
    return np.array(out[:], dtype=np.float64)


def _unit_scales(power: np.ndarray) -> np.ndarray:
    if not np.all(power > 0):
        raise ValueError(f"a row of zero power cannot be brought to unit mean power (mean |x|^2 per row: {power.tolist()})")
    return np.array([1.0 / math.sqrt(p) for p in power], dtype=np.float64)


def _search(x, rows: int, n: int, start: int, step: int, pitch: int, scale, M: int, B: int, W: int, dev: int):
    """The three launches of ``ssfm_cpr_search`` on the record ``scale[r] x[r pitch + start + k step]``: ``(index int32, phase float64, symbols
    complex128)``, each a ``(rows, n)`` DeviceArray."""
    if x.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)) or rows not in (1, 2) or n < 1 or start < 0 or step < 1 \
            or start + (n - 1) * step >= pitch or rows * pitch > x.size:
        raise ValueError(f"the record (rows={rows}, n={n}, start={start}, step={step}, pitch={pitch}) does not lie inside the array of {x.size} {x.dtype} values")
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if scale.shape != (rows,):
        raise ValueError(f"one scale per row: expected {rows}, got shape {scale.shape}")
    table, phase_step = _phase_table(B)
    index = _lib.DeviceArray((rows, n), np.int32, dev)
    phase = _lib.DeviceArray((rows, n), np.float64, dev)
    symbols = _lib.DeviceArray((rows, n), np.complex128, dev)
    _lib.api.ssfm_cpr_search(x, int(x.dtype == np.complex64), rows, n, start, step, pitch, scale.ctypes.data_as(C.POINTER(C.c_double)), M,
                             _half_spacing(M), B, W, table.ctypes.data_as(C.POINTER(C.c_double)), phase_step, index, phase, symbols)
    return index, phase, symbols


def _reshaped(a: "_lib.DeviceArray", shape) -> "_lib.DeviceArray":
    a.shape = tuple(shape)                                   # (the same bytes: (1, n) <-> (n,))
    return a


def CPR(symbols, M: int, test_phases: int = 32, window: int = 32, *, normalize: bool = True, scale=None, device=None):
    """Carrier-phase recovery by blind phase search of a record of one sample per symbol: ``(n,)`` or ``(2, n)``, complex128 or complex64, on the
    host or in GPU memory (an ``electrical_signal``, an ``optical_signal``, a ``DeviceArray`` or array_like).  Returns ``(symbols, phase, index)``:
    the rotated symbols (complex128; an ``electrical_signal`` for one row, an ``optical_signal`` for two, in GPU memory), the estimated phase
    (float64 ``DeviceArray`` of the record's shape) and the unwrapped phase index ``u`` (int32 ``DeviceArray``), with
    ``phase = (u - B / 2) pi / (2 B)`` and ``symbols = y exp(-1j phase)``.  The rows are independent.

    ``normalize`` scales each row to unit mean power first (a row of zero power raises ``ValueError``); ``scale`` (one factor per row) is used
    instead when given.  ``test_phases`` is even and lies in 2 ... 64, ``window`` in 0 ... 256 (the sums run over ``2 window + 1`` symbols).
    A multiple of ``pi / 2`` stays undetermined.  A non-finite sample is outside the contract: the call still ends and writes every output, and as
    a NaN compares false the chosen phase stays where the comparison leaves it."""
    t0 = time.time()
    M = _order(M)
    B, W = _check_search(test_phases, window)
    raw = _record(symbols)
    rows, n = (1 if raw.ndim == 1 else 2), int(raw.shape[-1])
    dev = _device(device)
    x = _field(raw, dev)
    if scale is not None:
        s = np.atleast_1d(np.asarray(scale, dtype=np.float64))
    elif normalize:
        s = _unit_scales(_row_power(x, rows, n, 0, 1, n))
    else:
        s = np.ones(rows)
    index, phase, z = _search(x, rows, n, 0, 1, n, s, M, B, W, dev)
    shape = tuple(raw.shape)
    out = _wrap_out(electrical_signal if rows == 1 else optical_signal, _reshaped(z, shape), NULL)
    out.execution_time = time.time() - t0
    return out, _reshaped(phase, shape), _reshaped(index, shape)


# ------------------------------------------------------------------------------------------------ alignment, EVM, BER, the receiver
def _sums(z, ref, n: int, M, turns: int) -> np.ndarray:
    out = (C.c_double * 4)()
    _lib.api.ssfm_qam_sums(z, ref, n, 0 if M is None else M, 0.0 if M is None else _half_spacing(M), turns, out)
    return np.array(out[:], dtype=np.float64)


def _is_bits(ref) -> bool:
    if isinstance(ref, (binary_sequence, str)):
        return True
    if isinstance(ref, (electrical_signal, optical_signal)):
        return False
    return np.dtype(ref.dtype if hasattr(ref, "dtype") else np.asarray(ref).dtype).kind != "c"


def _ref_symbols(ref, M: int, n: int, dev: int) -> "_lib.DeviceArray":
    """The transmitted symbols of one row as a complex128 DeviceArray of ``n`` values, from symbols or from bits."""
    if _is_bits(ref):
        ref = QAM_ENCODER(ref, M, device=dev)
    raw = _record(ref)
    if raw.ndim != 1 or raw.shape[0] < n:
        raise ValueError(f"`ref` must hold the {n} transmitted symbols of each row, got shape {tuple(raw.shape)}")
    return _as_device(raw, np.complex128, dev)


def EVM(symbols, ref=None, M: int = None, *, device=None) -> float:
    """Error vector magnitude ``sqrt(sum |z - s|^2 / sum |s|^2)`` of one row of symbols against ``ref`` (symbols or bits, ``M`` then required for
    bits), or against the symbols' own decisions when ``M`` is given and ``ref`` is not.  A host scalar; the symbols stay where they are."""
    if ref is None and M is None:
        raise ValueError("EVM needs `ref` or `M`")
    if M is not None:
        M = _order(M)
    raw = _record(symbols)
    if raw.ndim != 1:
        raise ValueError(f"EVM takes one row of symbols, got shape {tuple(raw.shape)}")
    if ref is not None and _is_bits(ref) and M is None:
        raise ValueError("EVM against bits needs `M`")
    dev = _device(device)
    z = _as_device(raw, np.complex128, dev)
    s = None if ref is None else _ref_symbols(ref, M, z.size, dev)
    out = _sums(z, s, z.size, M if s is None else None, 0)
    return math.sqrt(out[2] / out[3])


def BER(tx_bits, rx_bits) -> float:
    """``hamming_distance / size`` of two bit sequences of one size, counted where they lie."""
    tx = tx_bits if isinstance(tx_bits, binary_sequence) else binary_sequence(tx_bits)
    rx = rx_bits if isinstance(rx_bits, binary_sequence) else binary_sequence(rx_bits)
    if tx.size != rx.size or tx.size == 0:
        raise ValueError(f"BER compares two sequences of one positive size, got {tx.size} and {rx.size}")
    return tx.hamming_distance(rx) / tx.size


class Received:
    """What :func:`DSP` returns: ``bits`` (``binary_sequence``), ``symbols`` (the recovered symbols after the alignment, an
    ``electrical_signal``), ``phase`` (float64 ``DeviceArray``, the search's estimate without the alignment's quarter turns), ``quarter_turns``
    (0 ... 3, or None without ``ref``) and ``evm`` (a float), all but the last two in GPU memory.  For a ``(2, N)`` field each is a tuple of two."""

    __slots__ = ("bits", "symbols", "phase", "quarter_turns", "evm", "execution_time")

    def __init__(self, rows):
        pick = (lambda key: rows[0][key]) if len(rows) == 1 else (lambda key: tuple(r[key] for r in rows))
        for key in ("bits", "symbols", "phase", "quarter_turns", "evm"):
            setattr(self, key, pick(key))
        self.execution_time = 0.0

    def __repr__(self):
        return f"Received(quarter_turns={self.quarter_turns}, evm={self.evm})"


def DSP(input, M: int, instant: int = None, test_phases: int = 32, window: int = 32, ref=None, *, device=None) -> Received:
    """The coherent receiver of an ``optical_signal`` of shape ``(N,)`` or ``(2, N)``, complex64 or complex128: the symbols
    ``input[..., instant::sps]`` (``instant`` defaults to ``sps // 2``), each row scaled to unit mean power (zero power: ``ValueError``), the
    blind phase search of :func:`CPR`, the optional quarter-turn alignment and the decisions.  The strided read and the scaling happen inside
    the search's loads: no symbol array is formed in between.  The rows are received independently.

    ``ref``: the transmitted symbols or bits of each row (for two rows a pair, or a ``(2, n)`` array of symbols).  With it each row takes
    ``q = argmax_t Re(i^-t sum z conj(s))``, ``t = 0 ... 3``, the first on ties, and turns ``z`` by ``i^-q``; ``evm`` is then measured against
    ``ref``.  Without it ``quarter_turns`` is None, the ambiguity of a multiple of ``pi / 2`` remains (the bits are those of an unknown one of
    four rotations) and ``evm`` is measured against the decisions.  Returns a :class:`Received`."""
    t0 = time.time()
    input, grid, _ = _adopt(input, "optical_signal")
    if not isinstance(input, optical_signal):
        raise TypeError("`input` must be of type 'optical_signal'.")
    M = _order(M)
    B, W = _check_search(test_phases, window)
    raw = _record(input)
    sps, N = int(grid.sps), int(raw.shape[-1])
    instant = sps // 2 if instant is None else int(instant)
    if not 0 <= instant < N:
        raise ValueError(f"`instant` must lie inside the {N} samples of the field, got {instant}")
    rows, n = (1 if raw.ndim == 1 else 2), len(range(instant, N, sps))
    refs = [None] * rows
    if ref is not None:
        refs = [ref] if rows == 1 else ([ref[0], ref[1]] if not isinstance(ref, (binary_sequence, str, electrical_signal)) and len(ref) == 2 else None)
        if refs is None:
            raise ValueError("`ref` of a (2, N) field is a pair: the transmitted symbols or bits of each row")
    dev = _device(device)
    x = _field(raw, dev)
    a = _half_spacing(M)
    index, phase, z = _search(x, rows, n, instant, sps, N, _unit_scales(_row_power(x, rows, n, instant, sps, N)), M, B, W, dev)
    out = []
    for r in range(rows):
        zr = z.ptr + r * n * 16
        s = None if refs[r] is None else _ref_symbols(refs[r], M, n, dev)
        q = None
        if s is not None:
            c = _sums(zr, s, n, None, 0)
            q = int(np.argmax([c[0], c[1], -c[0], -c[1]]))                # Re(i^-t (c0 + i c1)), t = 0 ... 3
        bits = _lib.DeviceArray((n * _ORDERS[M][0],), np.uint8, dev)
        turned = _lib.DeviceArray((n,), np.complex128, dev)
        _lib.api.ssfm_qam_decide(zr, n, M, a, q or 0, bits, turned)
        e = _sums(zr, s, n, M if s is None else None, q or 0)
        out.append({"bits": _wrap_bits(bits, t0), "symbols": _wrap_out(electrical_signal, turned, NULL),
                    "phase": _reshaped(phase, (n,)) if rows == 1 else _row_block(phase, r, (n,)), "quarter_turns": q, "evm": math.sqrt(e[2] / e[3])})
    del index, z
    result = Received(out)
    result.execution_time = time.time() - t0
    return result
