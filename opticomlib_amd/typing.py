"""Boundary types of the fibre path: the slice of ``opticomlib.typing`` that ``FIBER`` /
``DBP`` / ``DM`` touch, and nothing else.

* :data:`NULL`      -- "no noise" sentinel (reference ``typing.py:56-93``): ``x + NULL == x``.
* :data:`gv`        -- global sampling parameters; a signal does not carry its sample rate,
                       ``optical_signal.w()`` reads ``gv.dt`` at call time (``typing.py:1641``).
* :class:`optical_signal` -- ``.signal``, ``.noise``, ``.n_pol``, ``.size``, ``.execution_time``,
                       ``.w()``, ``.to_numpy()`` with the reference's shape -> ``n_pol`` rules
                       (``typing.py:2124-2196``).

``electrical_signal.psd()`` / ``optical_signal.psd()`` plot the Welch spectrum of :func:`opticomlib_amd.get_psd` (computed on the
GPU; matplotlib is imported when the method is called).  :class:`electrical_signal` has the reference's operators and methods, computed
where the signal lies, and so has :class:`optical_signal`.  The other plots, eye diagrams etc. are out of scope.

The two signal classes are the direct subclasses of the private :class:`_signal_base` (neither is the other's subclass, unlike the
reference's): the base has the storage, the metadata, the reads and protocols and every operator and method the two share, each class the
hooks that build, wrap and launch (``_make``, ``_wrap``, ``_parse``, ``_binary_device``, ``_unary_device``, ``_reduce_device``,
``_div_device``, ``_pow_device``, ``_filter_device``, ``__getitem__``) and the members that really differ.  The different-GPUs check, a
slice key's ``(start, step, count)`` and an integer index's bounds check are module-level functions that :class:`binary_sequence` shares.
The HIP binding is imported inside the functions that launch, never at module level: a host-only operation loads no device.
"""
from __future__ import annotations

import numbers

import numpy as np


_C_LIGHT = 299792458.0       # scipy.constants.c


class _NullType:
    """Additive identity that swallows everything else."""

    _inst = None

    def __new__(cls):
        if cls._inst is None:
            cls._inst = super().__new__(cls)
        return cls._inst

    def __repr__(self):
        return "NULL"

    def __add__(self, other):
        return other

    __radd__ = __add__

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        if method == "__call__" and ufunc in (np.add, np.subtract) and inputs[1] is self:
            return inputs[0]
        return self

    def __bool__(self):
        return False


NULL = _NullType()


class _GlobalVars:
    """Sampling grid shared by all signals (reference ``typing.py:106-388``, the part the path
    needs: ``sps``, ``R``, ``fs``, ``dt``, and ``wavelength`` / ``f0`` for the EDFA's ASE power)."""

    def __init__(self):
        self.default()

    def default(self):
        self.sps = 16
        self.R = 1e9
        self.fs = self.R * self.sps
        self.dt = 1 / self.fs
        self.wavelength = 1550e-9              # reference typing.py:207-209
        self.f0 = _C_LIGHT / self.wavelength
        self.N = 128                           # number of bit slots (typing.py:211); only LASER reads it, through `t`
        self.t = np.linspace(0, self.N * self.sps * self.dt, self.N * self.sps, endpoint=True)      # typing.py:213
        return self

    def __call__(self, sps=None, R=None, fs=None, wavelength=1550e-9, N=None, **extra):
        # same precedence as the reference (typing.py:306-335)
        if sps:
            self.sps = int(np.round(sps))
            if R:
                self.R = R
                self.fs = R * self.sps
            elif fs:
                self.fs = fs
                self.R = fs / self.sps
            else:
                self.fs = self.R * self.sps
        elif R:
            self.R = R
            if fs:
                self.fs = fs
                self.sps = int(np.round(fs / R))
            else:
                self.fs = R * self.sps
        elif fs:
            self.fs = fs
            self.sps = int(np.round(fs / self.R))
        self.dt = 1 / self.fs
        self.N = N if N is not None else self.N
        self.t = np.linspace(0, self.N * self.sps / self.fs, self.N * self.sps, endpoint=True)      # typing.py:357
        self.wavelength = wavelength           # reset to the default on every call, like the reference (typing.py:340-341)
        self.f0 = _C_LIGHT / wavelength
        for k, v in extra.items():
            setattr(self, k, v)
        return self


gv = _GlobalVars()


def _is_device(a) -> bool:
    """A ``_lib.DeviceArray`` (checked by duck typing so that this module never imports the HIP binding)."""
    return hasattr(a, "to_host") and hasattr(a, "ptr")


class _LazyArray:
    """``signal`` / ``noise`` attribute that may be backed by a device-resident array.

    Device calls hand their results over as ``DeviceArray``; the first host access downloads the data and
    the object is an ordinary NumPy-backed signal from then on (a host array may be modified in place, so
    the device copy is dropped rather than kept in sync).  Device-aware callers read ``obj._raw(name)``
    instead, which never transfers anything."""

    def __set_name__(self, owner, name):
        self.slot = "_" + name

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        a = obj.__dict__.get(self.slot, NULL)
        if _is_device(a):
            a = a.to_host()
            obj.__dict__[self.slot] = a
        return a

    def __set__(self, obj, value):
        obj.__dict__[self.slot] = value


def _one_gpu(what, devices):
    """The one GPU among ``devices`` (those of the operands that lie on one), or None; operands ``what`` on two GPUs are a ``ValueError``."""
    devs = set(devices)
    if len(devs) > 1:
        raise ValueError(f"Can't operate {what} that lie on different GPUs {sorted(devs)}: move one of them first")
    return devs.pop() if devs else None


def _slice_span(key, size):
    """``(start, step, count)`` of a slice of ``size`` values, clipped as Python clips it (``count`` may be 0)."""
    start, stop, step = key.indices(size)
    return start, step, len(range(start, stop, step))


def _checked_index(key, size, axis=0):
    """An integer index into ``size`` values as a position from the front, or NumPy's ``IndexError``."""
    if not -size <= key < size:
        raise IndexError(f"index {key} is out of bounds for axis {axis} with size {size}")
    return int(key) % size


class binary_sequence:
    """Bit sequence (uint8 0 / 1) with the algebra of the reference's class (``typing.py:402-1009``): ``~``, ``&``, ``|``, ``^``, ``!=`` (a
    ``binary_sequence`` mask of the differences), ``+`` (concatenation, either order), ``*`` (an ``int`` above 1 tiles, anything else is ``&``),
    ``[]``, ``flip``, ``hamming_distance``, ``dac``, ``prbs``, ``ones``, ``zeros``, ``size``, ``sizeof``, ``print``, ``to_numpy``.  The other
    operand may be a sequence, a string (``'1010'``), a list, an array or a scalar: it goes through ``binary_sequence(other)``, so a value other
    than 0 / 1 is the constructor's ``ValueError``.  The lengths are equal or one of them is 1 (NumPy's broadcast); anything else is a ``ValueError``.
    ``ndarray + a`` and ``ndarray * a`` come to ``a``'s own operators through ``__array_ufunc__``.

    Residency: ``PRBS``, ``x > thr``, ``SAMPLER`` and the receivers leave their bits in GPU memory (``from_device``).  An operation on such a
    sequence is computed there by the HIP kernels of ``csrc/bits.hip`` and its result lies there too; a host operand is uploaded once, two
    sequences on different GPUs are a ``ValueError``.  ``ones``, ``zeros``, ``hamming_distance`` and an integer index bring one integer back and
    leave the sequence where it is; a slice (any step, empty results, bounds clipped as Python clips them) stays on the GPU; an index of another
    kind (a mask, an index array) materialises on the host.  ``dac(h)`` uploads nothing but ``h``.  An operation between host-only sequences is
    NumPy on the host, as in the reference, and loads no device.  ``.data`` downloads the bits on first access and the object is a host sequence
    from then on.

    ``==`` returns a host bool array (callers write ``(a == b).all()``), not the reference's mask; ``!=`` returns the mask.

    Not provided: ``plot``, the reference's ``__getattr__`` delegation to ``ndarray`` and ``__array_function__``.  A NumPy ufunc other than the
    two reflected operators sees the materialised bits and returns NumPy's own result."""

    data = _LazyArray()

    @classmethod
    def from_device(cls, bits):
        """Wrap a device-resident uint8 array of 0 / 1 values without copying it to the host."""
        self = cls.__new__(cls)
        if bits.ndim != 1 or np.dtype(bits.dtype) != np.uint8:
            raise ValueError(f"Binary sequence must be a 1D uint8 array, got {bits.dtype} {bits.shape}")
        self.data = bits
        self.execution_time = 0.0
        return self

    def _raw(self):
        return self.__dict__.get("_data")

    def __init__(self, data):
        if isinstance(data, binary_sequence):
            data = data.data
        if isinstance(data, str):
            data = [int(ch) for ch in data.replace(" ", "").replace(",", "")]
        d = np.asarray(data)
        if d.ndim == 0:
            d = d[np.newaxis]
        if d.ndim != 1:
            raise ValueError(f"Binary sequence must be 1D, invalid shape {d.shape}")
        if not np.all((d == 0) | (d == 1)):
            raise ValueError("Binary sequence must contain only 0 and 1 values.")
        self.data = d.astype(np.uint8)
        self.execution_time = 0.0

    # -- metadata (no transfer)
    @property
    def size(self) -> int:
        return int(self._raw().size)

    @property
    def type(self):
        return binary_sequence

    @property
    def on_device(self) -> bool:
        """True while the bits live in GPU memory only (no host copy has been asked for)."""
        return _is_device(self._raw())

    @property
    def sizeof(self) -> int:
        """Bytes the bits occupy, on the host or on the GPU: one per bit."""
        return self.size * np.dtype(np.uint8).itemsize

    def __len__(self):
        return self.size

    # -- one integer back from the GPU: the sequence stays where it is
    @property
    def ones(self) -> int:
        if self.on_device:
            from . import _lib
            return _lib.bits_count_device(self._raw())
        return int(np.count_nonzero(self.data))

    @property
    def zeros(self) -> int:
        return self.size - self.ones

    def _host(self) -> np.ndarray:
        """The bits as a host array; a device sequence is read, not converted."""
        raw = self._raw()
        return raw.to_host() if _is_device(raw) else raw

    def __iter__(self):
        return iter(self._host().tolist())

    def __array__(self, dtype=None, copy=None):
        return self.data if dtype is None else self.data.astype(dtype)

    def to_numpy(self, dtype=None) -> np.ndarray:
        return self.data if dtype is None else np.array(self.data, dtype=dtype)

    def __repr__(self):
        if _is_device(self._raw()):
            return f"binary_sequence(size={self.size}, on GPU {self._raw().device})"
        return f"binary_sequence({np.array2string(self.data, threshold=20)})"

    def __str__(self, title=None):
        title = 3 * "*" + f"    {self.__class__.__name__ if title is None else title}    " + 3 * "*"
        sub = len(title) * "-"
        where = f"on GPU {self._raw().device}" if self.on_device else np.array2string(self.data, threshold=100)
        return (f"\n{sub}\n{title}\n{sub}\n\tdata  :  {where} (shape: {(self.size,)})\n\tones  :  {self.ones}\n\tzeros :  {self.zeros}\n\t"
                f"size  :  {self.sizeof} bytes\n\ttime  :  {self.execution_time:.3g} s\n")

    def print(self, msg=None):
        """Print the sequence's parameters under the title ``msg``; returns ``self``."""
        print(self.__str__(msg))
        return self

    # -- operands: where they lie, and the one upload of a host operand
    def _pair(self, other):
        """``(other as a sequence, the GPU the operation runs on or None)``; the lengths are equal or one of them is 1."""
        o = other if isinstance(other, binary_sequence) else binary_sequence(other)
        return o, _one_gpu("binary_sequences", (x._raw().device for x in (self, o) if x.on_device))

    def _check_lengths(self, o):
        if self.size != o.size and 1 not in (self.size, o.size):
            raise ValueError(f"operands could not be broadcast together with shapes ({self.size},) ({o.size},)")

    def _on(self, dev):
        """The bits as a uint8 DeviceArray on GPU ``dev``."""
        if self.on_device:
            return self._raw()
        from . import _lib
        return _lib.DeviceArray.from_host(self.data, np.uint8, dev)

    def _logic(self, op, other):
        """``op``: 'and', 'or' or 'xor' between this sequence and ``other``, where the operands lie."""
        o, dev = self._pair(other)
        self._check_lengths(o)
        if dev is None:
            a, b = self.data, o.data
            return binary_sequence(a & b if op == "and" else (a | b if op == "or" else a ^ b))
        from . import _lib
        if 0 in (self.size, o.size):                            # (0,) against (0,) or (1,) is (0,), as NumPy broadcasts
            return binary_sequence.from_device(_lib.DeviceArray((0,), np.uint8, dev))
        code = {"and": _lib.BITS_AND, "or": _lib.BITS_OR, "xor": _lib.BITS_XOR}[op]
        return binary_sequence.from_device(_lib.bits_binary_device(code, self._on(dev), o._on(dev)))

    def _concat(self, other, reflected):
        o, dev = self._pair(other)
        first, second = (o, self) if reflected else (self, o)
        if dev is None:
            return binary_sequence(np.concatenate((first.data, second.data)))
        from . import _lib
        return binary_sequence.from_device(_lib.bits_concat_device(first._on(dev), second._on(dev)))

    # -- operators (reference typing.py:694-793)
    def __invert__(self):
        if self.on_device:
            from . import _lib
            return binary_sequence.from_device(_lib.bits_not_device(self._raw()))
        return binary_sequence(~self.data.astype(bool))

    def __and__(self, other):
        return self._logic("and", other)

    __rand__ = __and__

    def __or__(self, other):
        return self._logic("or", other)

    __ror__ = __or__

    def __xor__(self, other):
        return self._logic("xor", other)

    __rxor__ = __xor__

    def __ne__(self, other):
        """The mask of the positions that differ, as a ``binary_sequence`` (``hamming_distance`` is its sum).  ``==`` is not its mirror image
        here: it keeps returning a host bool array."""
        return self._logic("xor", other)

    def __eq__(self, other):
        """A host bool array (``(a == b).all()``); a device sequence is downloaded for it."""
        other = other.data if isinstance(other, binary_sequence) else np.asarray(other)
        return self.data == other

    def __add__(self, other):
        return self._concat(other, False)

    def __radd__(self, other):
        return self._concat(other, True)

    def __mul__(self, other):
        """An ``int`` above 1 repeats the sequence that many times; anything else (``0``, ``1``, ``True``, a sequence, an array) is ``&``
        with ``binary_sequence(other)``, so ``* 2.0`` and ``* -1`` are the constructor's ``ValueError`` (reference ``typing.py:747-761``)."""
        if isinstance(other, int) and other > 1:
            if self.on_device:
                from . import _lib
                return binary_sequence.from_device(_lib.bits_tile_device(self._raw(), other))
            return binary_sequence(np.tile(self.data, other))
        return self._logic("and", other)

    __rmul__ = __mul__

    def __getitem__(self, key):
        """An ``int``: the bit as a Python ``int``; a slice: a new sequence (on the GPU for a device sequence); any other index NumPy takes:
        the host array's answer."""
        raw = self._raw()
        if _is_device(raw) and isinstance(key, (int, np.integer, slice)) and not isinstance(key, (bool, np.bool_)):
            from . import _lib
            if isinstance(key, slice):
                return binary_sequence.from_device(_lib.bits_slice_device(raw, *_slice_span(key, raw.size)))
            return _lib.bits_count_device(raw, _checked_index(key, raw.size), 1)
        r = self.data[key]
        return binary_sequence(r) if isinstance(r, np.ndarray) else int(r)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        """``ndarray + a`` is ``a.__radd__(ndarray)`` and ``ndarray * a`` is ``a.__mul__(ndarray)`` (reference ``typing.py:606-614``); any
        other ufunc sees the materialised bits and its result comes back as NumPy made it."""
        if method == "__call__" and not kwargs.get("out") and len(inputs) == 2 and isinstance(inputs[1], binary_sequence):
            if ufunc is np.add:
                return inputs[1].__radd__(inputs[0])
            if ufunc is np.multiply:
                return inputs[1].__mul__(inputs[0])
        args = [a._host() if isinstance(a, binary_sequence) else a for a in inputs]
        return getattr(ufunc, method)(*args, **kwargs)

    # -- methods (reference typing.py:832-984)
    @staticmethod
    def prbs(order: int, len: int = None, seed: int = None, return_seed: bool = False):
        """Pseudo-random binary sequence: :func:`opticomlib_amd.devices.PRBS` (generated on the GPU, where it stays)."""
        from .devices import PRBS
        return PRBS(order, len, seed, return_seed)

    def flip(self):
        """``~self``."""
        return ~self

    def hamming_distance(self, other) -> int:
        """The number of positions at which the two sequences differ (lengths equal, or one of them 1), as a Python ``int``."""
        o, dev = self._pair(other)
        self._check_lengths(o)
        if dev is None:
            return int(np.count_nonzero(self.data != o.data))
        if self.size != o.size:                                 # one bit against n: the ones, or the zeros, of the longer sequence
            one, many = (self, o) if self.size == 1 else (o, self)
            return many.zeros if one[0] else many.ones
        if self.size == 0:
            return 0
        from . import _lib
        return _lib.count_diff_device(self._on(dev), o._on(dev))

    def dac(self, h):
        """``electrical_signal(upfir(bits, h, up=gv.sps))``: the bits held at offset ``sps // 2`` of ``gv.sps`` samples each, convolved with the
        impulse response ``h`` (``mode='same'``).  On the GPU for a device sequence (nothing but ``h`` is uploaded)."""
        if self.on_device:
            from . import devices
            raw = self._raw()
            if raw.size == 0:                                   # (what the constructor says to the host path's empty convolution)
                raise ValueError(f"Signal must be scalar or 1D array for electrical_signal, invalid shape {(0,)}")
            return electrical_signal.from_device(devices._upfir_device(raw, h, gv.sps, raw.device))
        import scipy.signal as sg
        xu = np.zeros(self.size * gv.sps)
        xu[gv.sps // 2::gv.sps] = self.data
        return electrical_signal(sg.fftconvolve(xu, h, mode="same"))


_DEVICE_DTYPES = (np.dtype(np.float64), np.dtype(np.complex128))
# enums of include/ssfm_amd.h (ssfm_signal_binary / ssfm_field_binary, ssfm_signal_unary / ssfm_field_unary)
_BINARY = {"add": 0, "sub": 1, "rsub": 2, "mul": 3, "gt": 4, "eq": 5}
_UNARY = {"neg": 0, "conj": 1, "div": 2, "floordiv": 3, "pow2": 4, "real": 5, "imag": 6, "abs_signal": 7, "abs_noise": 8, "abs_all": 9, "pow": 10}
# ssfm_field_*: the code of a device field's type (enum ssfm_precision and SSFM_F64_REAL of include/ssfm_amd.h), in the order the messages name them
_FIELD_CODES = {np.dtype(np.float64): 2, np.dtype(np.complex128): 1, np.dtype(np.complex64): 0}


def _type_names(types) -> str:
    """``'float64 and complex128'``, ``'float64, complex128 and complex64'``: the device types of a class, as its messages list them."""
    names = [str(t) for t in types]
    return ", ".join(names[:-1]) + " and " + names[-1]


# -- the host algebra that electrical_signal and optical_signal share: NumPy on materialised arrays, NULL for an absent noise
def _host_binary(make, op, s1, n1, s2, n2):
    """'add', 'sub', 'rsub' or 'mul' of (s1, n1) and (s2, n2) with the reference's signal / noise rules (``typing.py:1308-1348``);
    ``make(signal, noise)`` builds the result."""
    neg = lambda a: a if a is NULL else -a                                                           # noqa: E731
    if op == "add":
        return make(s1 + s2, n1 + n2)
    if op == "sub":                                             # a + (-b), as the reference forms it
        return make(s1 + (-s2), n1 + neg(n2))
    if op == "rsub":                                            # (-a) + b
        return make((-s1) + s2, neg(n1) + n2)
    noi = NULL                                                  # s1 n2 + n1 s2 + n1 n2; a product with NULL is NULL, a sum with it the other term
    for a, b in ((s1, n2), (n1, s2), (n1, n2)):
        if a is not NULL and b is not NULL:
            noi = noi + a * b
    return make(s1 * s2, noi)


def _host_map(make, f, x):
    """``make(f(signal), f(noise))``, an absent noise staying absent: neg, conj, real, imag, the quotient, sum, filter."""
    return make(f(x.signal), NULL if x.noise is NULL else f(x.noise))


def _host_pow(make, x, other):
    """``** 0``: ones; ``** 1``: the signal; ``** 2``: ``signal**2`` with the noise ``2 signal noise + noise**2``; any other exponent:
    ``(signal + noise) ** other`` without noise (reference ``typing.py:1400-1419``)."""
    if other == 0:
        return make(np.ones_like(x.signal), NULL)
    if other == 1:
        return make(x.signal, x.noise)
    if other == 2:
        return make(x.signal ** 2, NULL if x.noise is NULL else 2 * x.signal * x.noise + x.noise ** 2)
    return make((x.signal + x.noise) ** other, NULL)


def _check_divisor(number):
    """The reference's checks of ``/`` and ``//`` (``typing.py:1350-1357``; its texts name ``electrical_signal`` for both classes)."""
    if not isinstance(number, numbers.Complex):
        raise TypeError(f"Can't divide electrical_signal by type {type(number)}")
    if number == 0:
        raise ZeroDivisionError("Can't divide electrical_signal by zero")


def _reflected_ufunc(cls, ufunc, inputs):
    """``ndarray + x``, ``ndarray - x`` and ``ndarray * x`` as the operators of ``x`` (reference ``typing.py:1243-1255``), or NotImplemented."""
    if ufunc in (np.add, np.subtract, np.multiply) and len(inputs) == 2 and isinstance(inputs[1], cls):
        lhs, rhs = inputs
        if ufunc is np.add:
            return rhs.__add__(lhs)
        if ufunc is np.subtract:
            return (-rhs).__add__(lhs)
        return rhs.__mul__(lhs)
    return NotImplemented


def _signal_arrays(signal, noise, dtype):
    """The constructors' shared middle: ``signal`` and ``noise`` (or NULL) as arrays of one type, ``dtype`` or their ``result_type``, and of
    one shape; each class applies its own shape rules to them."""
    sig = np.asarray(signal)
    noi = noise
    if noi is not NULL:
        noi = np.asarray(noi)
        common = np.result_type(sig, noi) if dtype is None else dtype
        sig, noi = sig.astype(common, copy=False), noi.astype(common, copy=False)
        if sig.shape != noi.shape:
            raise ValueError(f"`signal` and `noise` must have the same shape, mismatch shapes {sig.shape} and {noi.shape}!")
    elif dtype is not None:
        sig = sig.astype(dtype, copy=False)
    return sig, noi


class _signal_base:
    """What :class:`electrical_signal` and :class:`optical_signal` have in common (in the reference the second inherits the first; here neither
    is the other's subclass): the lazy ``signal`` / ``noise`` storage, the metadata, the reads and NumPy protocols, and every operator and
    method whose two versions differed only in how the result is built.  Each operation is NumPy on the host for host-only operands and one
    launch on the GPU that holds a device-resident one.

    A class supplies the rest through hooks.  Attributes: ``_NOUN`` ("signal" / "field", for the messages), ``_DEVICE_TYPES`` (the types its
    device arrays take), ``_WRAPPED_NDIMS`` (the ufunc results that come back wrapped), ``_host_conj``; and, set once both classes exist,
    ``_FAMILY`` (the class of the two that an object descends from: the name in its messages, the operand its reflected ufuncs take) and
    ``_OPERANDS`` (the signal classes it takes as the other operand where they lie; anything else goes through the constructor).  Methods:
    ``_make`` (the class of a host result), ``_wrap`` (a device result), ``_parse``, ``_binary_device``, ``_unary_device``,
    ``_reduce_device`` (a ``(rows, 2)`` float64 array), ``_div_device``, ``_pow_device``, ``_filter_device`` and ``__getitem__``."""

    signal = _LazyArray()
    noise = _LazyArray()
    __hash__ = None                  # (an `__eq__` that returns an array: unhashable, as the reference's class)

    def _raw(self, name):
        return self.__dict__.get("_" + name, NULL)

    # -- metadata (reference typing.py:1216-1229, :1488-1522): no transfer
    @property
    def size(self) -> int:
        """Samples per polarisation (reference ``typing.py:2313-2320``)."""
        return int(self._raw("signal").shape[-1])

    @property
    def ndim(self) -> int:
        return self._raw("signal").ndim

    @property
    def shape(self):
        return tuple(self._raw("signal").shape)

    @property
    def on_device(self) -> bool:
        """True while ``signal`` lives in GPU memory only (no host copy has been asked for)."""
        return _is_device(self._raw("signal"))

    @property
    def type(self):
        return type(self)

    @property
    def fs(self):
        return gv.fs

    @property
    def sps(self):
        return gv.sps

    @property
    def dt(self):
        return gv.dt

    @property
    def t(self):
        return gv.t[:self.size]

    def __len__(self):
        return self.size

    # -- reads and protocols: __array__ / __iter__ / to_numpy materialise the signal on the host
    def __iter__(self):
        return iter(self.__array__())

    def __array__(self, dtype=None, copy=None):
        arr = self.signal + self.noise
        return arr if dtype is None else arr.astype(dtype)

    def to_numpy(self) -> np.ndarray:
        """``signal + noise`` (reference ``typing.py:1593-1597``)."""
        return np.asarray(self.signal + self.noise)

    def w(self, shift: bool = False) -> np.ndarray:
        """Angular frequency grid [rad/s], FFT order (reference ``typing.py:1628-1644``)."""
        w = np.fft.fftfreq(self.size, gv.dt) * 2 * np.pi
        return np.fft.fftshift(w, axes=-1) if shift else w

    def f(self, shift: bool = False) -> np.ndarray:
        """Frequency grid [Hz] (reference ``typing.py:1646-1660``)."""
        return self.w(shift) / (2 * np.pi)

    def __call__(self, domain, shift: bool = False):
        """New object holding the FFT (``'w'`` / ``'f'``) or inverse FFT (``'t'``) of signal and noise along the last axis
        (reference ``typing.py:1421-1462``); ``shift`` applies fftshift / ifftshift.  Computed on the GPU."""
        from . import devices
        return devices._fourier(self, domain, shift)

    def psd(self, fmt='-', mode='x', n=None, xlabel=None, ylabel=None, yscale='dbm', grid=False, hold=True, show=False, **kwargs):
        """Plot the power spectral density (reference ``typing.py:1850-1970``): Welch's estimate of the first ``n`` samples
        (default ``min(size, gv.t.size)``) with ``nperseg = min(2048, n)`` at ``fs = gv.fs * 1e-9`` [GHz], computed on the GPU.
        ``yscale``: ``'dbm'`` or ``'linear'`` (mW); ``mode``: ``'x'``, ``'y'`` or ``'both'`` polarisations.  Returns ``self``."""
        from .utils import plot_psd
        return plot_psd(self, fmt, mode, n, xlabel, ylabel, yscale, grid, hold, show, **kwargs)

    # -- device plumbing: the arrays where they lie
    def _device_arrays(self):
        """``(signal, noise or None)`` as DeviceArrays of one type (one of the class's ``_DEVICE_TYPES``) on one GPU, for a device-resident
        signal."""
        from . import _lib
        s, n = self._raw("signal"), self._raw("noise")
        name, noun = self._FAMILY.__name__, self._NOUN
        if s.dtype not in self._DEVICE_TYPES:
            raise TypeError(f"{name}: the device algebra takes {_type_names(self._DEVICE_TYPES)}, this {noun} lies on the GPU as {s.dtype}; "
                            f"there is no host fallback for a device-resident {noun} (convert it, or take .to_numpy())")
        if n is NULL:
            return s, None
        if not _is_device(n):                                   # (a noise that was assigned on the host afterwards)
            n = _lib.DeviceArray.from_host(np.ascontiguousarray(n, dtype=s.dtype), None, s.device)
        elif n.dtype != s.dtype or n.device != s.device:
            raise TypeError(f"{name}: signal ({s.dtype}, GPU {s.device}) and noise ({n.dtype}, GPU {n.device}) differ")
        return s, n

    def _shapes_error(self, shape):
        return ValueError(f"Can't operate '{self._make.__name__}'s with shapes {self.shape} and {tuple(shape)}")

    def _one_gpu(self, other):
        """The GPU that holds this signal or ``other`` (a signal or None); operands on two GPUs are a ``ValueError``."""
        return _one_gpu(f"'{self._make.__name__}'s", (x._raw("signal").device for x in (self, other) if x is not None and x.on_device))

    def _binary(self, op, other):
        """``op``: 'add', 'sub', 'rsub', 'mul', 'gt' or 'eq' between this signal and ``other``, where the operands lie."""
        if self.on_device or (isinstance(other, self._OPERANDS) and other.on_device):
            return self._binary_device(op, other)
        o = self._parse(other)
        s1, n1, s2, n2 = self.signal, self.noise, o.signal, o.noise
        if op in ("gt", "eq"):
            x, y = s1 + n1, s2 + n2
            return binary_sequence(x > y) if op == "gt" else x == y
        return _host_binary(self._make, op, s1, n1, s2, n2)

    # -- operators (reference typing.py:1308-1419)
    def __add__(self, other):
        return self._binary("add", other)

    def __radd__(self, other):
        return self._binary("add", other)

    def __sub__(self, other):
        return self._binary("sub", other)

    def __rsub__(self, other):
        return self._binary("rsub", other)

    def __mul__(self, other):
        """``(s1 + n1)(s2 + n2)``: the signal is ``s1 s2``, everything that contains a noise factor is noise."""
        return self._binary("mul", other)

    def __rmul__(self, other):
        return self.__mul__(other)

    def __eq__(self, other):
        """A host bool array (``(a == b).all()``); computed on the GPU for device operands, then read."""
        return self._binary("eq", other)

    def __neg__(self):
        if self.on_device:
            return self._unary_device("neg")
        return _host_map(self._make, lambda a: -a, self)

    def __truediv__(self, number):
        _check_divisor(number)
        if self.on_device:
            return self._div_device(number)
        return _host_map(self._make, lambda a: a / number, self)

    def __floordiv__(self, other):
        if self.on_device:
            _check_divisor(other)
            if self._raw("signal").dtype.kind == "c" or isinstance(other, (complex, np.complexfloating)):
                np.floor(np.zeros(1, np.complex128))            # NumPy's own TypeError: floor takes no complex values
            return self._unary_device("floordiv", float(other))
        return _host_map(self._make, np.floor, self / other)

    def __pow__(self, other):
        """``** 0``: ones; ``** 1``: the signal; ``** 2``: ``signal**2`` with the noise ``2 signal noise + noise**2`` (``2.0`` takes this
        branch too: the reference compares with ``==``); any other real exponent: ``(signal + noise) ** other`` without noise (on the GPU:
        of a complex signal, the exponents NumPy computes by products and ``0.5``)."""
        if not isinstance(other, numbers.Real):
            raise TypeError(f"Can't exponentiate electrical_signal by type {type(other)}")
        if self.on_device:
            return self._pow_device(other)
        return _host_pow(self._make, self, other)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        """``ndarray + x``, ``ndarray - x`` and ``ndarray * x`` go to the signal's own operators (the noise rules hold and no object array
        appears); ``np.abs`` of a device-resident signal stays there, as a signal; any other ufunc sees the materialised ``signal + noise``
        and a result of a dimension the class holds (1-D; for a field also 2-D) comes back wrapped (reference ``typing.py:1240-1275``)."""
        if method == "__call__" and not kwargs.get("out"):
            r = _reflected_ufunc(self._FAMILY, ufunc, inputs)
            if r is not NotImplemented:
                return r
            if ufunc is np.absolute and self.on_device and inputs[0] is self:
                return self._unary_device("abs_all", out_dtype=np.float64, single=True)
        make = self._make
        args = [a.__array__() if isinstance(a, make) else a for a in inputs]
        result = getattr(ufunc, method)(*args, **kwargs)
        if isinstance(result, np.ndarray) and result.ndim in self._WRAPPED_NDIMS:
            return make(result)
        return result

    # -- methods (reference typing.py:1476-1486, :1599-1780)
    @property
    def real(self):
        if self.on_device:
            return self._unary_device("real", out_dtype=np.float64)
        return _host_map(self._make, lambda a: a.real, self)

    @property
    def imag(self):
        if self.on_device:
            return self._unary_device("imag", out_dtype=np.float64)
        return _host_map(self._make, lambda a: a.imag, self)

    def conj(self):
        if self.on_device:
            return self._unary_device("conj")
        return _host_map(self._make, self._host_conj, self)

    def sum(self, axis=None):
        """Sums of signal and noise over the whole signal as a signal of size 1 (host values; on the device every row is summed in one
        launch, one small read each, and the rows are added on the host).  ``axis`` is the host path's, as NumPy's."""
        if self.on_device:
            s, n = self._device_arrays()

            def val(a):
                o = self._reduce_device(2, a).sum(axis=0)
                return a.dtype.type(complex(o[0], o[1])) if a.dtype.kind == "c" else np.float64(o[0])
            return self._make(val(s), NULL if n is None else val(n))
        return _host_map(self._make, lambda a: a.sum(axis=axis), self)

    def filter(self, h):
        """``scipy.signal.fftconvolve(., h, mode='same')`` of signal and noise (reference ``typing.py:1758-1780``): one polarisation,
        as SciPy's own ``ValueError`` says of a ``(2, N)`` field with 1-D taps.  On the GPU in double precision; a complex64 field is
        widened and the result rounded once."""
        if self.on_device:
            return self._filter_device(h)
        import scipy.signal as sg
        return _host_map(self._make, lambda a: sg.fftconvolve(a, h, mode="same"), self)


class electrical_signal(_signal_base):
    """1-D electrical signal with optional noise and the algebra of the reference's class (``typing.py:1022-1780``).

    ``+ - * / // **``, ``[]``, ``> < ==``, unary ``-``, ``abs``, ``power``, ``normalize``, ``phase``, ``conj``, ``sum``, ``filter``, ``w``,
    ``f``, ``t``, ``fs``, ``sps``, ``dt``, ``real``, ``imag`` and the NumPy protocols ``__array__`` / ``__array_ufunc__`` carry the reference's
    names, argument checks, error texts and signal / noise rules.

    Residency: an operation on a signal that lies in GPU memory (``on_device``: what ``PD``, ``LPF``, ``ADC``, ``DAC`` and ``SAMPLER``
    return) is computed there by the HIP kernels of ``csrc/signal_ops.hip`` and its result lies there too; a Python scalar is a kernel
    argument, a host array or host signal as the other operand is uploaded once, two signals on different GPUs are a ``ValueError``.
    Device arrays are float64 or complex128; any other device type raises ``TypeError``.  An operation on a host-only signal is NumPy on
    the host, as in the reference, and loads no device.  ``power``, ``sum`` and an integer index of a noiseless signal return host scalars;
    ``==`` returns a host bool array, ``>`` / ``<`` a ``binary_sequence`` (device-resident for device operands).  ``np.asarray(x)``,
    iteration and a NumPy ufunc other than the three reflected operators and ``np.abs`` materialise the signal on the host.

    On the device, ``filter`` with real signal, noise and taps carries the noise as the imaginary part of the signal's field through one
    convolution: a noise below ``1e-12`` of the signal loses its digits on that path.  ``**`` of a complex128 device signal takes the
    exponents NumPy computes by products (integers ``|p| < 100``) and ``0.5``; another exponent raises ``ValueError``.

    Not provided: ``plot``, ``print``, ``grid``, ``legend``, ``show``, ``sizeof``, the reference's ``__getattr__`` delegation
    to ``ndarray`` and ``__array_function__``."""

    _NOUN = "signal"
    _DEVICE_TYPES = _DEVICE_DTYPES
    _WRAPPED_NDIMS = (1,)
    _host_conj = staticmethod(lambda a: a.conj())               # (the reference's form: a real array is returned as it is, not copied)

    @property
    def _make(self):
        """A result has the class of the signal, so a subclass keeps its class."""
        return self.__class__

    @classmethod
    def from_device(cls, signal, noise=NULL):
        """Wrap device-resident 1-D arrays without copying them to the host."""
        self = cls.__new__(cls)
        if signal.ndim != 1 or (noise is not NULL and noise.shape != signal.shape):
            raise ValueError(f"Signal must be 1D array for electrical_signal, invalid shape {signal.shape}")
        self.signal, self.noise = signal, noise
        self.execution_time = 0.0
        return self

    def __init__(self, signal, noise=NULL, dtype=None):
        if isinstance(signal, electrical_signal):
            noise = signal.noise if noise is NULL else np.asarray(noise) + signal.noise
            signal = signal.signal
        sig, noi = _signal_arrays(signal, noise, dtype)
        if sig.ndim > 1 or sig.size < 1:
            raise ValueError(f"Signal must be scalar or 1D array for electrical_signal, invalid shape {sig.shape}")
        if sig.ndim == 0:
            sig = sig[np.newaxis]
            if noi is not NULL:
                noi = noi[np.newaxis]
        self.signal = sig
        self.noise = noi
        self.execution_time = 0.0

    MAX_EYE_TRACES = 4096

    def plot_eye(self, n_traces=None, cmap='jet', N_grid_bins=200, grid_sigma=5, style='dot', ax=None, **plot_kw):
        """Plot the eye diagram of signal + noise with ``gv.sps`` samples per symbol (reference ``typing.py:1971-2041``): at most
        ``min(n_traces, 4096)`` traces, the density computed where the signal lies (``utils.eyediagram`` has the styles and ``plot_kw``).
        Returns ``self``."""
        from .utils import eyediagram
        n_traces = self.MAX_EYE_TRACES if n_traces is None else min(n_traces, self.MAX_EYE_TRACES)
        eyediagram(self, gv.sps, n_traces, cmap, N_grid_bins, grid_sigma, style, ax, **plot_kw)
        return self

    def __repr__(self):
        where = " [device]" if self.on_device else ""
        return f"electrical_signal(size={self.size}, dtype={self._raw('signal').dtype}, noise={'NULL' if self._raw('noise') is NULL else 'array'}){where}"

    # -- device plumbing: uploads of the other operand, launches
    def _upload(self, dev):
        """This host signal's arrays on GPU ``dev`` as float64 / complex128 (the widening ``np.result_type`` would apply anyway)."""
        from . import _lib
        s = np.asarray(self.signal)
        dt = np.complex128 if s.dtype.kind == "c" else np.float64
        up = lambda a: _lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dt), None, dev)       # noqa: E731
        return up(s), (None if self.noise is NULL else up(self.noise))

    def _wrap(self, s, n=None):
        return self.__class__.from_device(s, NULL if n is None else n)

    def _parse(self, other):
        """The other operand as a signal of this class whose size is this one's or 1 (reference ``typing.py:1557-1573``)."""
        if not isinstance(other, self.type):
            other = self.__class__(other)
        if self.size != other.size and min(self.size, other.size) != 1:
            raise self._shapes_error(other.shape)
        return other

    def _binary_device(self, op, other):
        from . import _lib
        scalar = None
        if isinstance(other, (numbers.Number, np.number, np.bool_)):
            scalar = complex(other) if isinstance(other, (complex, np.complexfloating)) else float(other)
            size2, o = 1, None
        else:
            # (any electrical_signal is used where it lies, whatever its class: the constructor would read it to the host; the result is self's class)
            o = other if isinstance(other, self._OPERANDS) else self.__class__(other)
            size2 = o.size
        n = max(self.size, size2)
        if self.size != size2 and min(self.size, size2) != 1:
            raise self._shapes_error(o.shape)
        dev = self._one_gpu(o)
        s1, n1 = self._device_arrays() if self.on_device else self._upload(dev)
        s2 = n2 = None
        if o is not None:
            s2, n2 = o._device_arrays() if o.on_device else o._upload(dev)
        c1 = s1.dtype.kind == "c"
        c2 = isinstance(scalar, complex) if o is None else s2.dtype.kind == "c"
        if op in ("gt", "eq"):
            out = _lib.DeviceArray((n,), np.uint8, dev)
            out_n = None
        else:
            # the reference adds the noises with NULL as the identity, so a lone noise of size 1 meets a signal of size n in the constructor
            if op != "mul" and (n1 is None) != (n2 is None) and (n1 if n2 is None else n2).size != n:
                raise ValueError(f"`signal` and `noise` must have the same shape, mismatch shapes {(n,)} and {(1,)}!")
            dt = np.complex128 if (c1 or c2) else np.float64
            out = _lib.DeviceArray((n,), dt, dev)
            out_n = _lib.DeviceArray((n,), dt, dev) if (n1 is not None or n2 is not None) else None
        z = complex(scalar) if scalar is not None else 0j
        _lib.api.ssfm_signal_binary(_BINARY[op], 1, n, s1, n1, s1.size, int(c1), s2, n2, size2, int(c2), z.real, z.imag, out, out_n)
        if op == "gt":
            return binary_sequence.from_device(out)
        if op == "eq":
            return out.to_host().astype(bool)
        return self._wrap(out, out_n)

    def _unary_device(self, op, p=0.0, *, out_dtype=None, single=False):
        """One launch of ``ssfm_signal_unary``; ``out_dtype``: the result's type where it is not the signal's; ``single``: one result array
        without noise."""
        from . import _lib
        s, n = self._device_arrays()
        dt = s.dtype if out_dtype is None else out_dtype
        out = _lib.DeviceArray(s.shape, dt, s.device)
        out_n = None if (single or n is None) else _lib.DeviceArray(s.shape, dt, s.device)
        z = complex(p)
        _lib.api.ssfm_signal_unary(_UNARY[op], 1, s.size, s, n, int(s.dtype.kind == "c"), z.real, z.imag, int(isinstance(p, (complex, np.complexfloating))), out, out_n)
        return self._wrap(out, out_n)

    def _reduce_device(self, kind, s, n=None):
        """``ssfm_signal_reduce``: a ``(1, 2)`` float64 array."""
        from . import _lib
        import ctypes
        out = (ctypes.c_double * 2)()
        _lib.api.ssfm_signal_reduce(kind, 1, s.size, s, n, int(s.dtype.kind == "c"), out)
        return np.array(out[:], dtype=np.float64).reshape(1, 2)

    def _div_device(self, number):
        cplx = isinstance(number, (complex, np.complexfloating))
        return self._unary_device("div", complex(number) if cplx else float(number), out_dtype=np.complex128 if cplx else None)

    def _pow_device(self, other):
        s, n = self._device_arrays()
        if other == 0:
            from . import _lib
            ones = _lib.zeros_device(s.shape, s.dtype, s.device)
            return self._wrap(_lib.shift_device(ones, 1.0))
        if other == 1:
            return self._wrap(s, n)
        if other == 2:
            return self._unary_device("pow2")
        if s.dtype.kind == "c" and other != 0.5 and not (float(other).is_integer() and abs(other) < 100):
            raise ValueError(f"electrical_signal ** {other}: a complex128 signal on the GPU takes integer exponents below 100 and 0.5; "
                             "there is no host fallback for a device-resident signal")
        return self._unary_device("pow", float(other), single=True)

    def _filter_device(self, h):
        from . import devices
        s, n = self._device_arrays()
        return self._wrap(*devices._filter_device(s, n, h))

    def __getitem__(self, key):
        """A slice: a new signal (an empty one is the constructor's ``ValueError``); an ``int``: the value itself when there is no noise, a
        signal of size 1 otherwise (reference ``typing.py:1366-1376``)."""
        if not isinstance(key, (slice, int)):
            raise TypeError(f"Invalid argument type. {key} of type {type(key)}")
        if not self.on_device:
            if isinstance(key, int) and self.noise is NULL:
                return self.signal[key]
            return self.__class__(self.signal[key], NULL if self.noise is NULL else self.noise[key])
        from . import _lib
        s, n = self._device_arrays()
        if isinstance(key, slice):
            start, step, count = _slice_span(key, s.size)
            if count < 1:
                raise ValueError(f"Signal must be scalar or 1D array for electrical_signal, invalid shape {(0,)}")
        else:
            start, step, count = _checked_index(key, s.size), 1, 1
        out = _lib.DeviceArray((count,), s.dtype, s.device)
        out_n = None if n is None else _lib.DeviceArray((count,), s.dtype, s.device)
        _lib.api.ssfm_signal_slice(1, s.size, s, n, int(s.dtype.kind == "c"), start, step, count, out, out_n)
        if isinstance(key, int) and n is None:
            return out.to_host()[0]
        return self._wrap(out, out_n)

    def __gt__(self, other):
        return self._binary("gt", other)

    def __lt__(self, other):
        return other - self > 0                                 # (the reference's form: through `-`, not a comparison of its own)

    # -- methods (reference typing.py:1599-1780)
    def abs(self, of="all"):
        """``|signal|``, ``|noise|`` (zeros of the real type without noise) or ``|signal + noise|`` as a new signal."""
        if not isinstance(of, str):
            raise TypeError('`of` must be a string.')
        of = of.lower()
        if of not in ("signal", "noise", "all"):
            raise ValueError('`of` must be one of the following values ("signal", "noise", "all")')
        if self.on_device:
            if of == "noise" and self._raw("noise") is NULL:
                from . import _lib
                s = self._raw("signal")
                return self._wrap(_lib.zeros_device(s.shape, np.float64, s.device))
            return self._unary_device("abs_" + of, out_dtype=np.float64, single=True)
        if of == "signal":
            return self.__class__(np.abs(self.signal))
        if of == "noise":
            return self.__class__(np.zeros_like(self.signal.real) if self.noise is NULL else np.abs(self.noise))
        return np.abs(self)                                     # through __array_ufunc__, as the reference

    def power(self, unit="W", of="all"):
        """Mean ``|.|**2`` of the signal, the noise or both, in W or dBm (a host scalar)."""
        if of.lower() not in ("signal", "noise", "all"):
            raise ValueError('`of` must be one of the following values ("signal", "noise", "all")')
        if self.on_device:
            s, n = self._device_arrays()
            of = of.lower()
            if of == "noise" and n is None:
                p = np.float64(0.0)
            else:
                p = self._reduce_device(0, n if of == "noise" else s, n if of == "all" else None)[0, 0]
        else:
            p = np.mean(np.asarray(self.abs(of).signal) ** 2, axis=-1)
        unit = unit.lower()
        if unit == "w":
            return p
        if unit == "dbm":
            with np.errstate(divide="ignore"):
                return 10 * np.log10(p) + 30
        raise ValueError('`unit` must be one of the following values ("W", "dBm")')

    def normalize(self, by="power"):
        """The signal divided by the square root of its signal power, or by its largest ``|signal|``."""
        if by == "power":
            return self / self.power("W", "signal") ** 0.5
        if by == "amplitude":
            if self.on_device:
                return self / self._reduce_device(1, self._device_arrays()[0])[0, 0]
            return self / np.abs(self.signal).max()
        raise ValueError('`by` must be one of the following values ("power", "amplitude")')

    def phase(self):
        """``unwrap(angle(signal + noise))`` as a signal without noise."""
        if self.on_device:
            from . import _lib
            s, n = self._device_arrays()
            out = _lib.DeviceArray(s.shape, np.float64, s.device)
            _lib.api.ssfm_signal_phase(1, s.size, s, n, int(s.dtype.kind == "c"), out)
            return self._wrap(out)
        return self.__class__(np.unwrap(np.angle(self.__array__())))


def _field_total(x, dev):
    """``signal + noise`` of a field or an electrical signal, in its own type, as one array on GPU ``dev`` (the signal itself without noise)."""
    from . import _lib
    if not x.on_device:
        return np.asarray(x.signal + x.noise)                 # (uploaded once, as the operation's type, by the caller)
    s, n = x._device_arrays()
    if n is None:
        return s
    out = _lib.DeviceArray(s.shape, s.dtype, s.device)
    rows, cols = (s.shape[0] if s.ndim == 2 else 1), s.shape[-1]
    _lib.api.ssfm_field_binary(_BINARY["add"], _FIELD_CODES[s.dtype], rows, cols, s, None, rows, cols, n, None, rows, cols, 0.0, 0.0, out, None)
    return out


class optical_signal(_signal_base):
    """Optical field: ``signal`` (and optional ``noise``) of shape ``(N,)`` for one polarisation or ``(2, N)`` for two, with the algebra the
    reference's class inherits from ``electrical_signal`` (``typing.py:1308-1419``) and its own indexing (``typing.py:2261-2305``).

    ``+ - * / // **`` and the reflected forms, unary ``-``, ``==``, ``[]`` with a slice, an integer or ``x[pol, samples]``, ``conj``, ``real``,
    ``imag``, ``sum``, ``power``, ``normalize``, ``filter``, ``w``, ``f``, ``t``, ``fs``, ``sps``, ``dt``, ``type``, ``ndim``, ``__array__``,
    ``__iter__`` and ``__array_ufunc__`` carry the reference's names, argument checks, error texts (they say ``electrical_signal`` where the
    reference's do) and signal / noise rules.  Operands broadcast as NumPy's: a ``(2, N)`` field with an ``(N,)`` field, an
    ``electrical_signal`` (its signal and noise stay apart and serve both polarisations), a ``(2, 1)`` or ``(1,)`` value, an array or a
    scalar.  The result's ``n_pol`` follows its shape.  ``>`` and ``<`` raise the reference's ``NotImplementedError``.

    Residency, as ``electrical_signal``'s: an operation with a device-resident operand (``on_device``: what ``FIBER``, ``DBP``, ``DM``,
    ``BPF``, ``EDFA``, ``MZM``, ``LASER``, ``PM`` and ``FBG`` return) runs on that GPU, by the ``ssfm_field_*`` kernels of
    ``csrc/signal_ops.hip``, and its result lies there too.  A Python scalar is a kernel argument; a host array or host signal as the other
    operand is uploaded once; operands on two GPUs are a ``ValueError``; there is no silent copy to the host: a case the device path does
    not take raises.  Device fields are float64, complex128 or complex64; another device type is a ``TypeError``.  Host-only operands are
    NumPy on the host and load no device.

    Types on the device follow NumPy >= 2's ``result_type`` of the arrays the reference forms (a Python ``2.5`` is a float64 array there,
    so ``complex64 * 2.5`` is complex128; ``complex64 / 2.5`` stays complex64).  ``+ - *``, ``-x``, ``conj``, ``[]`` and the quotient by a
    scalar of complex64 operands are computed in single precision; a complex64 operand that meets a wider one is widened first (exact).
    ``**``, ``power``, ``sum``, ``normalize`` and ``filter`` of a complex64 field are computed in double precision from the widened values
    and rounded once.  ``power`` (a NumPy scalar, or a ``(2,)`` array), ``sum`` (a host field of size 1) and an element ``x[i]`` of a
    noiseless field bring numbers back, ``==`` a host bool array; ``np.asarray(x)``, iteration and a NumPy ufunc other than the three
    reflected operators and ``np.abs`` materialise the field on the host.

    ``abs(of)`` and ``phase()`` are reads, like ``.signal``: they return host NumPy arrays (the reference returns signal objects there).
    The device-resident magnitude is ``np.abs(x)``.

    Left to raise on the GPU: ``real``, ``imag`` and ``np.abs`` of a complex64 field (float32 in NumPy, a type the device arrays do not
    hold): ``TypeError``; ``**`` of a complex field with an exponent other than an integer ``|p| < 100`` or ``0.5``: ``ValueError``;
    ``filter`` of a two-polarisation field: SciPy's ``ValueError``, as on the host; a polarisation key other than an integer or ``:`` and
    a samples key other than an integer or a slice: ``TypeError``.

    Not provided: ``plot``, ``print``, ``sizeof``, the reference's ``__getattr__`` delegation to ``ndarray`` and ``__array_function__``."""

    _NOUN = "field"
    _DEVICE_TYPES = _FIELD_CODES
    _WRAPPED_NDIMS = (1, 2)
    _host_conj = staticmethod(np.conj)                          # (a copy, of a real array too)

    @property
    def _make(self):
        """A result is an ``optical_signal`` whose ``n_pol`` follows its shape, as in ``self.__class__(sig, noi)`` of the reference."""
        return optical_signal

    @classmethod
    def from_device(cls, signal, noise=NULL, n_pol=None):
        """Wrap device-resident arrays of shape ``(N,)`` or ``(2, N)`` without copying them to the host."""
        self = cls.__new__(cls)
        if signal.ndim not in (1, 2) or (signal.ndim == 2 and signal.shape[0] != 2):
            raise ValueError(f"device-resident optical_signal needs shape (N,) or (2, N), got {signal.shape}")
        if noise is not NULL and tuple(noise.shape) != tuple(signal.shape):
            raise ValueError(f"`signal` and `noise` must have the same shape, mismatch shapes {signal.shape} and {noise.shape}!")
        self.signal, self.noise = signal, noise
        self.n_pol = signal.ndim if n_pol is None else n_pol
        self.execution_time = 0.0
        return self

    def __init__(self, signal, noise=NULL, n_pol=None, dtype=None):
        if _is_device(signal) and (noise is NULL or _is_device(noise)) and dtype is None:      # device arrays: no copy to the host
            other = optical_signal.from_device(signal, noise, n_pol)
            self.__dict__.update(other.__dict__)
            return
        if _is_device(signal):
            signal = signal.to_host()
        if _is_device(noise):
            noise = noise.to_host()
        if isinstance(signal, optical_signal):
            if noise is NULL and n_pol in (None, signal.n_pol) and dtype is None:      # plain re-wrap: keep device residency
                self.signal, self.noise, self.n_pol, self.execution_time = signal._raw("signal"), signal._raw("noise"), signal.n_pol, 0.0
                return
            if noise is not NULL:
                noise = np.asarray(noise) + signal.noise
            else:
                noise = signal.noise
            signal = signal.signal
        sig, noi = _signal_arrays(signal, noise, dtype)

        if sig.ndim > 2 or (sig.ndim > 1 and sig.shape[0] > 2) or sig.size < 1:
            raise ValueError(f"Signal must be a scalar, 1D or 2D array for optical_signal, invalid shape {sig.shape}")
        if n_pol is not None and n_pol not in (1, 2):
            raise ValueError("n_pol must be either 1 or 2")

        def both(f):
            return f(sig), (noi if noi is NULL else f(noi))

        want_two = n_pol == 2
        if sig.ndim == 0:
            if want_two:
                sig, noi = both(lambda a: np.array([[a], [a]]))
            else:
                sig, noi = both(lambda a: a[np.newaxis])
                n_pol = 1
        elif sig.ndim == 1:
            if want_two:
                sig, noi = both(lambda a: np.array([a, a]))
            else:
                n_pol = 1
        elif sig.shape[0] == 1:            # (1, N): becomes dual-pol by tiling unless n_pol=1
            if n_pol in (None, 2):
                sig, noi = both(lambda a: np.tile(a, (2, 1)))
                n_pol = 2
            else:
                sig, noi = both(lambda a: a[0])
        else:                              # (2, N)
            if n_pol in (None, 2):
                n_pol = 2
            else:
                sig, noi = both(lambda a: a[0])

        self.signal = sig
        self.noise = noi
        self.n_pol = n_pol
        self.execution_time = 0.0

    # -- reads: NumPy arrays on the host, like `.signal` (the reference returns signal objects here; the device-resident |x| is np.abs(x))
    def abs(self, of: str = "all") -> np.ndarray:
        """``|signal|``, ``|noise|`` (zeros without noise) or ``|signal + noise|`` as a host array: a read, like ``.signal``."""
        of = of.lower()
        if of == "signal":
            return np.abs(self.signal)
        if of == "noise":
            return np.zeros_like(np.real(self.signal)) if self.noise is NULL else np.abs(self.noise)
        if of == "all":
            return np.abs(self.to_numpy())
        raise ValueError('`of` must be one of the following values ("signal", "noise", "all")')

    def phase(self) -> np.ndarray:
        """``unwrap(angle(signal + noise))`` as a host array: a read, like ``.signal``."""
        return np.unwrap(np.angle(self.to_numpy()))

    def power(self, unit: str = "W", of: str = "all"):
        """Mean power per polarisation of the signal, the noise or both, in W or dBm: a NumPy scalar, or a ``(2,)`` array.  Reduced on the
        GPU for a device-resident field (every row in one launch; a complex64 field is widened and the result rounded once to float32)."""
        single = False
        if self.on_device:
            if of.lower() not in ("signal", "noise", "all"):
                raise ValueError('`of` must be one of the following values ("signal", "noise", "all")')
            s, n = self._device_arrays()
            single = s.dtype == np.complex64                    # float64 up to the end, then rounded once to NumPy's float32
            of = of.lower()
            if of == "noise" and n is None:
                p = np.zeros(s.shape[:-1])[()]
            else:
                p = self._reduce_device(0, n if of == "noise" else s, n if of == "all" else None)[:, 0]
                p = p if s.ndim == 2 else p[0]
        else:
            p = np.mean(self.abs(of) ** 2, axis=-1)
        unit = unit.lower()
        if unit == "w":
            return p.astype(np.float32) if single else p
        if unit == "dbm":
            p = 10 * np.log10(p) + 30
            return p.astype(np.float32) if single else p
        raise ValueError('`unit` must be one of the following values ("W", "dBm")')

    # -- device plumbing: the one upload of a host operand, launches
    @staticmethod
    def _wrap(s, n=None):
        """A device result as a field; ``n_pol`` follows the shape, as in ``self.__class__(sig, noi)`` of the reference."""
        return optical_signal.from_device(s, NULL if n is None else n)

    @staticmethod
    def _as(a, dt, dev):
        """Array ``a`` (device or host, or None) on GPU ``dev`` as type ``dt``: widened on the device (exact), or uploaded once as ``dt``."""
        from . import _lib
        if a is None:
            return None
        if _is_device(a):
            return a if a.dtype == dt else a.astype(dt)
        return _lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dt), None, dev)

    def _parse(self, other):
        """The other operand as a field whose size is this one's or 1 (reference ``typing.py:1557-1573``); an ``electrical_signal`` keeps its
        signal and noise apart and broadcasts over the polarisations."""
        if isinstance(other, electrical_signal):
            other = optical_signal(other.signal, other.noise)
        elif not isinstance(other, optical_signal):
            other = optical_signal(other)
        if self.size != other.size and min(self.size, other.size) != 1:
            raise self._shapes_error(other.shape)
        return other

    def _binary_device(self, op, other):
        """One launch of ``ssfm_field_binary`` on the GPU that holds a device-resident operand.  The result's type is NumPy's
        ``result_type`` of the arrays the reference would form (a scalar is ``np.array(scalar)``: a Python float is float64 there);
        an operand of a narrower type is widened first, which is exact."""
        from . import _lib
        scalar = None
        if isinstance(other, (numbers.Number, np.number, np.bool_)):
            scalar, o = complex(other), None
            shape2, dt2 = (1,), np.asarray(other).dtype
        else:
            if isinstance(other, self._OPERANDS):
                o = other
            else:
                o = optical_signal(other)                       # a host array: the constructor's shape rules and errors
            shape2, dt2 = tuple(o._raw("signal").shape), o._raw("signal").dtype
        if self.size != shape2[-1] and min(self.size, shape2[-1]) != 1:
            raise self._shapes_error(shape2)
        dev = self._one_gpu(o)
        for x in (self, o):
            if x is not None and x.on_device:
                x._device_arrays()                              # (the TypeError of a device type the kernels do not take)
        shape = np.broadcast_shapes(self.shape, shape2)
        dt = np.result_type(self._raw("signal").dtype, dt2)
        if dt not in _FIELD_CODES:
            raise TypeError(f"optical_signal: the device algebra takes {_type_names(_FIELD_CODES)}, not the {dt} this operation gives")
        part = lambda x: [None if a is NULL else a for a in (x._raw("signal"), x._raw("noise"))]     # noqa: E731
        (s1, n1), (s2, n2) = part(self), ((None, None) if o is None else part(o))
        if op == "eq":                                          # signal + noise of each operand in its own type first, as NumPy forms it
            s1, n1 = _field_total(self, dev), None
            if o is not None:
                s2, n2 = _field_total(o, dev), None
        elif op != "mul" and (n1 is None) != (n2 is None):
            # the reference adds the noises with NULL as the identity: a lone noise meets the signal's shape in the constructor
            nshape = tuple((n1 if n2 is None else n2).shape)
            if nshape != shape:
                raise ValueError(f"`signal` and `noise` must have the same shape, mismatch shapes {shape} and {nshape}!")
        s1, n1, s2, n2 = (self._as(a, dt, dev) for a in (s1, n1, s2, n2))
        rows, n = (shape[0] if len(shape) == 2 else 1), shape[-1]
        dims = lambda sh: ((sh[0] if len(sh) == 2 else 1), sh[-1])                                   # noqa: E731
        if op == "eq":
            out, out_n = _lib.DeviceArray(shape, np.uint8, dev), None
        else:
            out = _lib.DeviceArray(shape, dt, dev)
            out_n = _lib.DeviceArray(shape, dt, dev) if (n1 is not None or n2 is not None) else None
        z = scalar if scalar is not None else 0j
        _lib.api.ssfm_field_binary(_BINARY[op], _FIELD_CODES[dt], rows, n, s1, n1, *dims(self.shape), s2, n2, *dims(shape2), z.real, z.imag, out, out_n)
        if op == "eq":
            return out.to_host().astype(bool)
        return self._wrap(out, out_n)

    def _unary_device(self, op, p=0.0, *, out_dtype=None, single=False, wide=False, back=False):
        """One launch of ``ssfm_field_unary``.  ``out_dtype``: the result's type where it is not the field's; ``single``: one result array
        without noise; ``wide``: a complex64 field is widened (exact) and computed in double precision; ``back``: the result of that is
        rounded once to complex64.  ``real``, ``imag`` and ``np.abs`` of a complex64 field are float32 arrays in NumPy, a type the device
        arrays do not have: ``TypeError``."""
        from . import _lib
        s, n = self._device_arrays()
        what = {"real": "real", "imag": "imag", "abs_all": "np.abs"}.get(op)
        if what and s.dtype == np.complex64:
            raise TypeError(f"optical_signal: {what} of a complex64 field on the GPU would be float32, which the device arrays do not hold; "
                            "widen the field first (x * np.complex128(1)) or take .to_numpy()")
        narrow = back and wide and s.dtype == np.complex64
        if wide and s.dtype == np.complex64:
            s, n = s.astype(np.complex128), (None if n is None else n.astype(np.complex128))
        dt = s.dtype if out_dtype is None else np.dtype(out_dtype)
        out = _lib.DeviceArray(s.shape, dt, s.device)
        out_n = None if (single or n is None) else _lib.DeviceArray(s.shape, dt, s.device)
        z = complex(p)
        rows, cols = (s.shape[0] if s.ndim == 2 else 1), s.shape[-1]
        _lib.api.ssfm_field_unary(_UNARY[op], _FIELD_CODES[s.dtype], rows, cols, s, n, z.real, z.imag, int(isinstance(p, (complex, np.complexfloating))), out, out_n)
        if narrow and dt == np.complex128:
            out, out_n = out.astype(np.complex64), (None if out_n is None else out_n.astype(np.complex64))
        return self._wrap(out, out_n)

    def _reduce_device(self, kind, s, n=None):
        """``ssfm_field_reduce`` of every row in one launch: a ``(rows, 2)`` float64 array (a complex64 field is widened first)."""
        from . import _lib
        import ctypes
        if s.dtype == np.complex64:
            s, n = s.astype(np.complex128), (None if n is None else n.astype(np.complex128))
        rows = s.shape[0] if s.ndim == 2 else 1
        out = (ctypes.c_double * (2 * rows))()
        _lib.api.ssfm_field_reduce(kind, rows, s.shape[-1], s, n, int(s.dtype.kind == "c"), out)
        return np.array(out[:], dtype=np.float64).reshape(rows, 2)

    def _div_device(self, number):
        s, _ = self._device_arrays()
        dt = np.result_type(s.dtype, number)                    # NumPy >= 2: a Python scalar does not widen a complex64 field, a float64 scalar does
        cplx = isinstance(number, (complex, np.complexfloating))
        return self._unary_device("div", complex(number) if cplx else float(number), out_dtype=dt, wide=dt != np.complex64)

    def _pow_device(self, other):
        s, n = self._device_arrays()
        if other == 0:
            from . import _lib
            ones = _lib.shift_device(_lib.zeros_device(s.shape, np.complex128 if s.dtype.kind == "c" else np.float64, s.device), 1.0)
            return self._wrap(ones if ones.dtype == s.dtype or s.dtype.kind != "c" else ones.astype(s.dtype))
        if other == 1:
            return self._wrap(s, n)
        if other == 2:
            return self._unary_device("pow2", wide=True, back=True)
        if s.dtype.kind == "c" and other != 0.5 and not (float(other).is_integer() and abs(other) < 100):
            raise ValueError(f"optical_signal ** {other}: a complex field on the GPU takes integer exponents below 100 and 0.5; "
                             "there is no host fallback for a device-resident field")
        return self._unary_device("pow", float(other), single=True, wide=True, back=True)

    def _filter_device(self, h):
        from . import devices
        s, n = self._device_arrays()
        h = np.asarray(h)
        if s.ndim != h.ndim:
            raise ValueError("in1 and in2 should have the same dimensionality")
        single = s.dtype == np.complex64
        if single:
            s, n = s.astype(np.complex128), (None if n is None else n.astype(np.complex128))
        out, out_n = devices._filter_device(s, n, h)
        if single and np.result_type(np.complex64, h.dtype) == np.complex64:
            out, out_n = out.astype(np.complex64), (None if out_n is None else out_n.astype(np.complex64))
        return self._wrap(out, out_n)

    # -- operators of its own (reference typing.py:1308-1419, :2261-2305)
    def __mul__(self, other):
        """``(s1 + n1)(s2 + n2)``: the signal is ``s1 s2``, everything that contains a noise factor is noise."""
        raw_s, raw_n = self._raw("signal"), self._raw("noise")
        if isinstance(other, (int, float)) and not isinstance(other, bool) and _is_device(raw_s) and raw_s.dtype in (np.complex128, np.float64) \
                and (raw_n is NULL or (_is_device(raw_n) and raw_n.dtype == raw_s.dtype)):
            from . import _lib                                 # a real gain / loss factor on a device-resident signal
            return optical_signal.from_device(_lib.scale_add_device(raw_s, float(other)),
                                              NULL if raw_n is NULL else _lib.scale_add_device(raw_n, float(other)), n_pol=self.n_pol)
        return self._binary("mul", other)

    def __gt__(self, other):
        raise NotImplementedError('The > operator is not implemented for optical_signal objects.')

    def __lt__(self, other):
        raise NotImplementedError('The < operator is not implemented for optical_signal objects.')

    def __getitem__(self, key):
        """The reference's indexing (``typing.py:2261-2305``): a slice cuts the samples of every polarisation; an integer is a sample of a
        one-polarisation field (the value itself without noise) or a polarisation of a two-polarisation field; ``x[pol, samples]`` takes
        both.  On the GPU a polarisation is an integer or ``:`` and the samples an integer or a slice; other keys raise ``TypeError``."""
        if self.on_device:
            return self._getitem_device(key)
        sig_, noi_, two = self.signal, self.noise, self.n_pol == 2
        if isinstance(key, tuple):
            if len(key) != 2:
                raise IndexError('Too many indices for optical_signal object.')
            pol_idx, time_idx = key
            if not two and pol_idx not in [0, -1, slice(None)]:
                raise IndexError('Optical signal has only one polarization (index 0).')
            sig = sig_[pol_idx, time_idx] if two else sig_[time_idx]
            if noi_ is not NULL:
                noi = noi_[pol_idx, time_idx] if two else noi_[time_idx]
            elif isinstance(time_idx, int):
                return sig[time_idx]
            else:
                noi = NULL
            return optical_signal(sig, noi, n_pol=1 if sig.ndim != 2 else self.n_pol)
        if isinstance(key, slice):
            cut = (lambda a: a[:, key]) if two else (lambda a: a[key])
            return optical_signal(cut(sig_), NULL if noi_ is NULL else cut(noi_), n_pol=self.n_pol)
        if not two:
            sig = sig_[key]
            if noi_ is NULL:
                return sig
            noi = noi_[key]
        else:
            sig = sig_[key, :]
            noi = NULL if noi_ is NULL else noi_[key, :]
        return optical_signal(sig, noi, n_pol=1 if sig.ndim != 2 else self.n_pol)

    def _getitem_device(self, key):
        from . import _lib
        s, n = self._device_arrays()
        two, size = self.n_pol == 2 and s.ndim == 2, s.shape[-1]
        bad_shape = lambda sh: ValueError(f"Signal must be a scalar, 1D or 2D array for optical_signal, invalid shape {sh}")     # noqa: E731
        is_int = lambda k: isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_))                            # noqa: E731

        def probe(k):
            """NumPy's own exception for a key it does not take (asked of an array of this shape that holds no data)."""
            np.broadcast_to(np.zeros(1, np.uint8), s.shape)[k]

        def column(k):
            """(start, step, count, is a single sample) of the samples' key."""
            if isinstance(k, slice):
                return *_slice_span(k, size), False
            if not is_int(k):
                probe((slice(None), k) if two else k)
                raise TypeError(f"optical_signal on the GPU takes an integer or a slice for the samples, not {k!r} of type {type(k)}; "
                                "there is no host fallback for a device-resident field")
            return _checked_index(k, size, 1 if two else 0), 1, 1, True

        def row(k):
            if not is_int(k):
                probe(k)
                raise TypeError(f"optical_signal on the GPU takes an integer or ':' for the polarisation, not {k!r} of type {type(k)}; "
                                "there is no host fallback for a device-resident field")
            return _checked_index(k, 2)

        def cut(row0, nrows, start, step, count, shape):
            out = _lib.DeviceArray(shape, s.dtype, s.device)
            out_n = None if n is None else _lib.DeviceArray(shape, s.dtype, s.device)
            _lib.api.ssfm_field_slice(_FIELD_CODES[s.dtype], 2 if s.ndim == 2 else 1, size, s, n, row0, nrows, start, step, count, out, out_n)
            return out, out_n

        if isinstance(key, tuple):
            if len(key) != 2:
                raise IndexError('Too many indices for optical_signal object.')
            pol_idx, time_idx = key
            if not two and pol_idx not in [0, -1, slice(None)]:
                raise IndexError('Optical signal has only one polarization (index 0).')
            all_rows = not two or (isinstance(pol_idx, slice) and pol_idx == slice(None))
            r0 = 0 if all_rows else row(pol_idx)
            start, step, count, one = column(time_idx)
            nrows = 2 if (two and all_rows) else 1
            if n is None and isinstance(time_idx, int):         # the reference indexes its result once more by the sample's key
                if nrows == 1:
                    raise IndexError("invalid index to scalar variable.")
                return cut(_checked_index(time_idx, 2), 1, start, 1, 1, (1,))[0].to_host()[0]
            if count < 1:
                raise bad_shape((2, 0) if nrows == 2 else (0,))
            shape = ((2,) if nrows == 2 else (1,)) if one else ((2, count) if nrows == 2 else (count,))
            return self._wrap(*cut(r0, nrows, start, step, count, shape))
        if isinstance(key, slice):
            start, step, count, _ = column(key)
            if count < 1:
                raise bad_shape((2, 0) if two else (0,))
            return self._wrap(*cut(0, 2 if two else 1, start, step, count, (2, count) if two else (count,)))
        if not two:
            start, _, _, _ = column(key)
            out, out_n = cut(0, 1, start, 1, 1, (1,))
            return out.to_host()[0] if n is None else self._wrap(out, out_n)
        return self._wrap(*cut(row(key), 1, 0, 1, size, (size,)))

    def normalize(self, by="power"):
        """The field divided by the square root of its signal power (one polarisation: the quotient is by a scalar), or by its largest
        ``|signal|`` over both polarisations."""
        if by not in ("power", "amplitude"):
            raise ValueError('`by` must be one of the following values ("power", "amplitude")')
        if not self.on_device:
            return self / (self.power("W", "signal") ** 0.5 if by == "power" else np.abs(self.signal).max())
        s = self._device_arrays()[0]
        if by == "power":
            d = self._reduce_device(0, s)[:, 0] ** 0.5
            d = d if s.ndim == 2 else d[0]
        else:
            amp = self._reduce_device(1, s)[:, 0]
            d = amp[np.isnan(amp)][0] if np.isnan(amp).any() else amp.max()
        if s.dtype != np.complex64 or np.ndim(d) or d == 0:     # (two powers: the quotient's TypeError, as the (2,) array of power() gives it)
            return self / (d.astype(np.float32) if s.dtype == np.complex64 else d)
        return self._unary_device("div", float(d), wide=True, back=True)      # float64 up to the end, then rounded once to complex64

    def __repr__(self):
        where = " [device]" if self.on_device else ""
        return f"optical_signal(n_pol={self.n_pol}, size={self.size}, dtype={self._raw('signal').dtype}, noise={'NULL' if self._raw('noise') is NULL else 'array'}){where}"


# set once both classes exist: the class of the two that an object descends from, and the signal classes it takes as the other operand where
# they lie (a host electrical_signal reads a device-resident optical_signal through its constructor, as it reads an array)
electrical_signal._FAMILY, electrical_signal._OPERANDS = electrical_signal, (electrical_signal,)
optical_signal._FAMILY, optical_signal._OPERANDS = optical_signal, (optical_signal, electrical_signal)


class EyeShowOptions:
    """What ``eye.plot`` draws beside the eye itself (reference ``typing.py:2440-2457``): ``averages``, ``threshold``, ``cross_points``,
    ``legends``, ``t_opt``, ``histogram``; an option left None takes ``all_none`` (False: a default plot draws the eye alone)."""

    def __init__(self, averages: bool = None, threshold: bool = None, cross_points: bool = None, legends: bool = None, t_opt: bool = None,
                 histogram: bool = None, all_none: bool = False):
        self.averages = averages if averages is not None else all_none
        self.threshold = threshold if threshold is not None else all_none
        self.cross_points = cross_points if cross_points is not None else all_none
        self.legends = legends if legends is not None else all_none
        self.t_opt = t_opt if t_opt is not None else all_none
        self.histogram = histogram if histogram is not None else all_none


class _KnownSlots(_LazyArray):
    """``eye.ones`` / ``eye.zeros``: a lazy array that only the eye of ``lab.GET_EYE_v2`` has (an ``AttributeError`` on any other eye)."""

    def __get__(self, obj, objtype=None):
        if obj is not None and self.slot not in obj.__dict__:
            raise AttributeError(f"'eye' object has no attribute '{self.slot[1:]}'")
        return super().__get__(obj, objtype)


class eye:
    """Eye-diagram parameters: what ``GET_EYE`` returns, with the reference's attribute names (``typing.py`` class ``eye``), ``plot`` and
    ``show``.  ``plot`` computes the picture where ``y`` lies (:func:`opticomlib_amd.utils.eye_fold_density`) and does not download it.

    ``y`` (the possibly resampled, rolled signal) stays on the GPU until it is read; ``t``, ``y_25_75``, ``y_top`` and ``y_bot`` are
    formed from it on first access (NaN outside their masks, as in the reference).  The eye of ``lab.GET_EYE_v2`` also has ``ones`` and
    ``zeros`` (the samples of the slots sent as 1 / as 0, on the GPU until they are read) and their slot grids ``t1`` / ``t0``."""

    y = _LazyArray()
    ones = _KnownSlots()
    zeros = _KnownSlots()

    def __init__(self, **kw):
        y = kw.pop("y", None)
        known = {k: kw.pop(k) for k in ("ones", "zeros") if k in kw}
        self.__dict__.update(kw)
        self.y = y
        for k, v in known.items():
            setattr(self, k, v)
        self._cache = {}

    def _tgrid(self):
        s = getattr(self, "sps_resamp", None) or self.sps
        return np.linspace(-1, 1 - 1 / s, 2 * s)

    def _masked(self, name, keep):
        if name not in self._cache:
            y = self.y.copy()
            y[~keep(y)] = np.nan
            self._cache[name] = y
        return self._cache[name]

    @property
    def t(self):
        if "t" not in self._cache:
            self._cache["t"] = np.kron(np.ones(self._nslots // 2), self._tgrid())
        return self._cache["t"]

    def _slot_grid(self, name, count):
        """``t0`` / ``t1``: the grid of one slot tiled over the slots of that level (``lab.GET_EYE_v2`` only)."""
        if count not in self.__dict__:
            raise AttributeError(f"'eye' object has no attribute '{name}'")
        if name not in self._cache:
            self._cache[name] = np.kron(np.ones(self.__dict__[count]), np.linspace(-0.5, 0.5, self.sps, endpoint=False))
        return self._cache[name]

    @property
    def t0(self):
        return self._slot_grid("t0", "_n0")

    @property
    def t1(self):
        return self._slot_grid("t1", "_n1")

    @property
    def y_25_75(self):
        if self._v25 is None:                              # the fallback branch: no band
            return None
        return self._masked("y_25_75", lambda y: (y > self._v25) & (y < self._v75))

    @property
    def y_top(self):
        return self._masked("y_top", lambda y: (y > self._y_center) & (self.t_span0 < self.t) & (self.t < self.t_span1))

    @property
    def y_bot(self):
        return self._masked("y_bot", lambda y: (y < self._y_center) & (self.t_span0 < self.t) & (self.t < self.t_span1))

    def plot(self, show_options: EyeShowOptions = EyeShowOptions(), hlines: list = [], vlines: list = [], style='dark', cmap='winter',
             smooth: bool = True, title: str = '', savefig: str = None, ax=None):
        """Plot the eye diagram (reference ``typing.py:2577-2796``), artist for artist: the blurred 350 x 350 density as an image
        (``smooth=True``) or one ``LineCollection`` per trace coloured by it, and what ``show_options`` asks for -- the decision instant and its
        span, the crossing points, the threshold, the means, legends, and a side panel with the density's profile at the centre (``smooth``) or
        the step histogram of the samples within the span.  ``hlines`` / ``vlines``: further lines.  ``style``: 'dark' or 'light' (applied when
        the axes are created here).  ``savefig``: a file name ('.png' at 300 dpi).  Returns the eye.

        The grid, the colours and the histogram come from :func:`opticomlib_amd.utils.eye_fold_density`: for an eye whose ``y`` lies in GPU
        memory they are computed there and ``y`` stays there."""
        from .utils import EYE_PLOT_BINS, eye_fold_density
        if self.__dict__.get("_y") is None or "t_opt" not in self.__dict__ or "sps" not in self.__dict__:
            raise ValueError('Empty eye diagram object.')
        if style == 'dark':
            style_context, t_opt_color, means_color = 'dark_background', '#60FF86', 'white'
        elif style == 'light':
            style_context, t_opt_color, means_color = 'default', 'green', '#5A5A5A'
        else:
            raise TypeError("The `style` argument must be one of the following values ('dark', 'light')")
        import matplotlib.pyplot as plt
        from contextlib import nullcontext
        dt = self.dt
        with plt.style.context(style_context) if ax is None else nullcontext():
            if show_options.histogram:
                fig, ax = plt.subplots(1, 2, gridspec_kw={'width_ratios': [4, 1], 'wspace': 0.03}, figsize=(8, 5))
            elif ax is None:
                fig, ax = plt.subplots(1, 1)
                ax = [ax, ax]
            else:
                ax = [ax, ax]
            if title:
                plt.suptitle(f'Eye diagram {title}')
            ax[0].set_xlim(-1 - dt, 1)
            ax[0].set_ylim(self.mu0 - 4 * self.s0, self.mu1 + 4 * self.s1)
            ax[0].set_ylabel(r'Amplitude [V]', fontsize=12)
            ax[0].grid(color='grey', ls='--', lw=0.5, alpha=0.5)
            ax[0].set_xticks([-1, -0.5, 0, 0.5, 1])
            ax[0].set_xlabel(r'Time [$t/T_{slot}$]', fontsize=12)
            if show_options.t_opt:
                ax[0].axvline(self.t_opt, color=t_opt_color, ls='--', alpha=0.7)
                ax[0].axvline(self.t_span0, color=t_opt_color, ls='-', alpha=0.4)
                ax[0].axvline(self.t_span1, color=t_opt_color, ls='-', alpha=0.4)
            if show_options.cross_points:
                if self.y_right and self.y_left:
                    ax[0].plot([self.t_left, self.t_right], [self.y_left, self.y_right], 'xr')
            if show_options.threshold:
                ax[0].axhline(self.threshold, c='r', ls='--')
                if show_options.histogram:
                    ax[1].axhline(self.threshold, c='r', ls='--', label='th')
                    if show_options.legends:
                        ax[1].legend()
            for hl in hlines:
                ax[0].axhline(hl, c='y')
                if show_options.histogram:
                    ax[1].axhline(hl, c='y')
            for vl in vlines:
                ax[0].axvline(vl, c='y')
                if show_options.histogram:
                    ax[1].axvline(vl, c='y')
            if show_options.legends:
                ax[0].legend([r'$t_{opt}$'], fontsize=12, loc='upper right')
            if show_options.averages:
                ax[0].axhline(self.mu1, color=means_color, ls=':', alpha=0.7)
                ax[0].axhline(self.mu0, color=means_color, ls='-.', alpha=0.7)
                if show_options.histogram:
                    ax[1].axhline(self.mu1, color=means_color, ls=':', alpha=0.7, label=r'$\mu_1$')
                    ax[1].axhline(self.mu0, color=means_color, ls='-.', alpha=0.7, label=r'$\mu_0$')
                    if show_options.legends:
                        ax[1].legend()
            if show_options.histogram:
                ax[1].sharey(ax[0])
                ax[1].tick_params(axis='x', which='both', length=0, labelbottom=False)
                ax[1].tick_params(axis='y', which='both', length=0, labelleft=False)
                ax[1].grid(color='grey', ls='--', lw=0.5, alpha=0.5)

            # the eye itself: computed where the record lies
            step_hist = show_options.histogram and not smooth
            d = eye_fold_density(self, colors=not smooth,
                                 hist=(self.t_opt - 0.05 * self.t_dist, self.t_opt + 0.05 * self.t_dist) if step_hist else None)
            if smooth:
                from scipy.special import expit
                heatmap = d.counts.astype(np.float64)
                vmin, vmax = heatmap.min(), heatmap.max()
                alpha_values = expit((d.grid - (vmin + 0.05 * (vmax - vmin))) * 100 / (vmax - vmin)).T * 0.8
                ax[0].imshow(d.grid.T, extent=[d.xedges[0], d.xedges[-1], d.yedges[0], d.yedges[-1]], origin='lower', aspect='auto',
                             alpha=alpha_values, cmap=cmap, interpolation='bicubic', resample=True)
            else:
                from matplotlib.collections import LineCollection
                L = 2 * self.sps
                t = d.x[:L]
                for c, y in zip(d.colors.reshape(-1, L), d.y.reshape(-1, L)):
                    points = np.array([t, y]).T.reshape(-1, 1, 2)
                    segments = np.concatenate([points[:-1], points[1:]], axis=1)
                    ax[0].add_collection(LineCollection(segments, colors=getattr(plt.cm, cmap)(c[:-1]), linewidth=1, alpha=0.05))
            if show_options.histogram:
                if smooth:
                    ax[1].plot(d.grid[170:180].sum(axis=0), np.linspace(d.extent[2], d.extent[3], EYE_PLOT_BINS), color=t_opt_color)
                else:                                           # np.histogram's counts, drawn as the reference's ax.hist draws them
                    ax[1].hist(d.hist_edges[:-1], bins=d.hist_edges, weights=d.hist_counts.astype(np.int64), density=True,
                               orientation='horizontal', color=t_opt_color, alpha=0.9, histtype='step')
            if savefig:
                if savefig.endswith('.png'):
                    plt.savefig(savefig, dpi=300)
                else:
                    plt.savefig(savefig)
        return self

    def show(self):
        """``plt.show()`` (reference ``typing.py:2798-2808``); returns the eye."""
        import matplotlib.pyplot as plt
        plt.show()
        return self

    def __repr__(self):
        return (f"eye(sps={self.sps}, t_opt={self.t_opt}, i={self.i}, mu0={self.mu0:.6g}, mu1={self.mu1:.6g}, s0={self.s0:.3g}, "
                f"s1={self.s1:.3g}, threshold={self.threshold})")
