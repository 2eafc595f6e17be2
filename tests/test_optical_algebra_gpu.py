"""The optical_signal algebra on the MI355X: every fixture again with the operands uploaded first, a sweep against live NumPy at tile and grid
edges with rows that start off 16 bytes, every key form at the first and last row and column, the refusals of the entry points, a chain
between devices without host transfers, determinism.

Bounds.  eps is 2^-52 for float64 / complex128 results and 2^-23 for complex64 ones; "u" is a distance in units of eps |want| (of the
modulus for complex values).  The double-precision cases keep the bounds derived in the docstring of tests/test_signal_algebra_gpu.py:
* + - neg conj real imag [] == floor, everything real-typed, and the quotient of a complex field by a REAL scalar: NumPy's bits.  So are
  + - neg conj [] == of complex64 operands (single precision, no contraction), and a complex64 operand that meets a wider one (the widening
  is exact and the arithmetic from there on is the double-precision kernel's).
* Complex products and the three-term noise, x ** 2 with its noise included: elementwise |d| <= 8 eps (|s1||s2| resp. |s1||n2| + |n1||s2| +
  |n1||n2|), with the eps of the result's type.  Complex128 ** 3: |d| <= 2 x 8 eps |s + n|^3.
* The quotient by a COMPLEX scalar and complex128 ** -1: 1 u; the complex64 quotient by any scalar is the same restatement of NumPy's loop
  in single precision: 1 u of 2^-23.  np.abs of complex128 and real ** p: 2 u.  Complex128 ** 0.5: 2.75 u.  normalize('amplitude') of a
  complex128 field: 3 u.
* power, sum, filter and normalize('power') in double precision: 1e-12 of the peak.
* What a complex64 field computes in float64 and rounds once (** other than 0 / 1 / 2, power, sum, normalize, filter): NumPy's
  single-precision result and the device's are each held against the float64 restatement (the same operation on the widened operands, on
  the host); the device may be no further from it than NumPy is, plus one 2^-23 of the result's scale.  No number is fixed in advance.
  filter() with single-precision taps, or of a complex64 field with double-precision taps, is held in the same way although its result
  is complex128: SciPy transforms the single-precision operand in single precision, so its own result lies 2e-8 to 1e-6 (absolute, on
  values of order 1 to 10) from the float64 restatement and cannot carry the 1e-12; the device's lies 1e-7 or less from it (the rows
  'filter fixtures ... numpy vs float64' and '... device vs float64' of profiles/field_ops_margins.txt).
real, imag and np.abs of a complex64 field on the GPU are float32 in NumPy, a type the device arrays do not hold: they raise TypeError
(class docstring), and the replay holds them to that.  Every measured distance is recorded (tools/margins_digest.py folds the records into
profiles/field_ops_margins.txt).

The sweep runs every pairing of shapes with every placement up to n = 257.  From 65535 on every pairing runs at one placement each, and
the placements rotate over the pairings, the types and the row counts, so every placement occurs at every size but not every combination
of pairing and placement.  The two largest sizes are there for the later passes of the grid-stride loops alone, and the host's own NumPy
arithmetic on 2 x 2^20 complex values is what a case costs: they run two rows only, every pairing with one of + - * (the three share
one loop), one array and one scalar operand, and a subset of the unary operations, cuts and reductions.  The launch is min(ceil(units / 256), 2048) workgroups of 256 lanes per row: a
lane of the one-value kernel (complex128) takes a second pass from n = 2^19 + 1 on, so 2^20 + 1 gives it a third; a lane of the two-value
kernels (float64, complex64) moves two values, and with the peeled head of row 1 its pairs pass 2^19 first at n = 2^20 + 3, the odd size
that is there for it.  At both sizes the (N,), (2, 1), (1,) and electrical operands are read in those later passes too.  The size-1
reads and the two-value reads off a 16-byte boundary (an (N,) operand under row 1 of an odd (2, N) result) are among them."""
import ctypes
import os

import numpy as np
import pytest

import margins
import optical_cases as oc
from opticomlib_amd import NULL, _lib, electrical_signal, gv, optical_signal
from test_optical_algebra_cpu import CASES, expected, load_group, load_namespace, same

pytestmark = pytest.mark.gpu
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 65535, (1 << 20) + 1, (1 << 20) + 3)
ULP = {"hypot": 2.0, "pow": 2.0, "cquot": 1.0, "csqrt": 2.75, "cnorm": 3.0}
SINGLE = (np.dtype(np.complex64), np.dtype(np.float32))
CODE = {np.dtype(np.complex64): 0, np.dtype(np.complex128): 1, np.dtype(np.float64): 2}


def eps_of(a):
    return EPS32 if np.asarray(a).dtype in SINGLE else EPS64


def dev(x):
    """The object with its arrays uploaded as they are."""
    up = lambda a: _lib.DeviceArray.from_host(np.ascontiguousarray(a))       # noqa: E731
    cls = electrical_signal if isinstance(x, electrical_signal) else optical_signal
    return cls.from_device(up(x.signal), NULL if x.noise is NULL else up(x.noise))


def widen(x):
    """A host object with its single-precision arrays as double-precision ones: the operand of the float64 restatement."""
    if isinstance(x, (optical_signal, electrical_signal)):
        w = lambda a: a.astype(np.result_type(a.dtype, np.float64))          # noqa: E731
        return type(x)(w(x.signal), NULL if x.noise is NULL else w(x.noise))
    return x.astype(np.result_type(x.dtype, np.float64)) if isinstance(x, np.ndarray) and x.dtype in SINGLE else x


def O(s, n=None, on=True):
    x = optical_signal(s) if n is None else optical_signal(s, n)
    return dev(x) if on else x


def ulps(got, want, what, bound):
    """Largest |got - want| in units of eps |want| (of the modulus for complex values), eps of want's type; recorded, then held to `bound`."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(want[fin]).astype(np.float64), np.finfo(np.float64).tiny) * eps_of(want)
        d = float(np.max(np.abs(got[fin].astype(np.complex128) - want[fin].astype(np.complex128)) / scale)) if fin.any() else 0.0
    return margins.within(got, want, bound=bound, what=f"{what} [ulp]", measured=d)


def peak(got, want, what, bound=1e-12, pk=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, got.shape, want.shape)
    fin = np.isfinite(want)
    if not fin.all():                            # (-inf dBm of a zero power: the value itself, nothing to measure)
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
        if not fin.any():
            return True
    pk = float(np.max(np.abs(want[fin]))) if pk is None else pk
    return margins.within(got, want, bound=bound, what=what, measured=float(np.max(np.abs(got[fin] - want[fin]))) / (pk or 1.0))


def rounded_once(got, want, exact, what):
    """A single-precision result that the device computes in float64 and rounds once: NumPy's result and the device's each against the
    float64 restatement `exact`; the device may be no further from it than NumPy is, plus one 2^-23 of the result's scale."""
    got, want, exact = np.asarray(got), np.asarray(want), np.asarray(exact)
    assert got.shape == want.shape == exact.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, got.shape, exact.shape)
    fin = np.isfinite(exact) & np.isfinite(want)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), what
    if not fin.any():
        return True
    wide = np.complex128 if exact.dtype.kind == "c" else np.float64
    d_np = float(np.max(np.abs(want[fin].astype(wide) - exact[fin])))
    d_dev = float(np.max(np.abs(got[fin].astype(wide) - exact[fin])))
    slack = EPS32 * float(np.max(np.abs(exact[fin])))
    if d_np + slack == 0.0:                      # (a result that is zero throughout, e.g. the power of an absent noise)
        return d_dev == 0.0
    margins.record(f"{what} numpy vs float64", None, d_np, d_np + slack)
    return margins.within(got, want, bound=d_np + slack, what=f"{what} device vs float64", measured=d_dev)


def parts(x):
    """(|signal|, |noise| or 0) of an operand: a signal, an array or a scalar."""
    if isinstance(x, (optical_signal, electrical_signal)):
        return np.abs(x.signal).astype(np.float64), (0.0 if x.noise is NULL else np.abs(x.noise).astype(np.float64))
    return np.abs(np.asarray(x)).astype(np.float64), 0.0


def product_ok(got, want, a, b, what):
    """|d| <= 8 eps |s1||s2| for the signal and 8 eps (|s1||n2| + |n1||s2| + |n1||n2|) for the noise, elementwise; eps of the result's type."""
    (s1, n1), (s2, n2) = parts(a), parts(b)
    ok = True
    for key, m in (("signal", s1 * s2), ("noise", s1 * n2 + n1 * s2 + n1 * n2)):
        if key in want:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].dtype, want[key].dtype, got[key].shape)
            d = np.abs(got[key].astype(np.complex128) - want[key].astype(np.complex128))
            bound = 8 * eps_of(want[key]) * np.broadcast_to(m, d.shape)
            worst = float(np.max(d / np.maximum(bound, np.finfo(np.float64).tiny)))
            ok &= margins.within(got[key], want[key], bound=1.0, what=f"{what} {key} [|d| / (8 eps terms)]", measured=worst)
    return ok


def cube_ok(got, want, x, what):
    """Complex128 ** 3 = (z z) z: two products, elementwise |d| <= 2 x 8 eps |z|^3 with z = signal + noise."""
    z = np.abs(np.asarray(x.signal + x.noise))
    assert got.dtype == want.dtype and got.shape == want.shape
    worst = float(np.max(np.abs(got - want) / np.maximum(16 * EPS64 * z ** 3, np.finfo(np.float64).tiny)))
    return margins.within(got, want, bound=1.0, what=f"{what} [|d| / (16 eps |z|^3)]", measured=worst)


def split_id(name, v):
    for i, ch in enumerate(name):
        if ch in "+-*" and i > 0 and (name[:i] in v or name[:i] in oc.SCALARS) and (name[i + 1:] in v or name[i + 1:] in oc.SCALARS):
            return name[:i], ch, name[i + 1:]
    raise AssertionError(name)


def check_values(group, name, got, want, v, exact):
    """The bound that belongs to the case (module docstring).  `exact()`: the case on the widened host operands, described."""
    what = f"{group}/{name}"
    if want.keys() != got.keys():
        return False
    kind = str(want["kind"])
    if kind == "error":
        return str(want["type"]) == str(got["type"]) and str(want["text"]) == str(got["text"])
    arrs = [k for k in want if k in ("signal", "noise", "data", "value")]
    if kind == "signal" and str(want["cls"]) != str(got["cls"]):
        return False
    if any(got[k].dtype != want[k].dtype or got[k].shape != want[k].shape for k in arrs):
        return False
    cplx = any(want[k].dtype.kind == "c" for k in arrs)
    single = any(want[k].dtype in SINGLE for k in arrs)
    once = lambda: all(rounded_once(got[k], want[k], exact()[k], what + " " + k) for k in arrs)       # noqa: E731
    if group.startswith("binary") or group == "reflected":
        a, op, b = split_id(name, v)
        if op == "*" and cplx:
            return product_ok(got, want, v[a] if a in v else oc.SCALARS[a], v[b] if b in v else oc.SCALARS[b], what)
    elif group == "scalar" and "/" in name and "//" not in name and cplx:
        if name.split("/")[1] != "1+1j" and not single:      # a real divisor in double precision: NumPy's bits
            return all(same(got[k], want[k]) for k in arrs)
        return all(ulps(got[k], want[k], what + " " + k, ULP["cquot"]) for k in arrs)
    elif group == "pow":
        x, p = v[name.split("**")[0]], name.split("**")[1]
        if cplx and p in ("2", "2.0"):
            return product_ok(got, want, x, x, what)
        if single and p not in ("0", "1"):
            return once()
        if cplx and p == "3":
            return cube_ok(got["signal"], want["signal"], x, what)
        if cplx and p in ("-1", "0.5"):
            return ulps(got["signal"], want["signal"], what, ULP["cquot"] if p == "-1" else ULP["csqrt"])
        if p in ("3", "0.5", "-1"):
            return ulps(got["signal"], want["signal"], what, ULP["pow"])
    elif group == "methods":
        if single and (".power" in name or ".sum" in name or ".normalize" in name):
            return once()
        if ".normalize(amplitude)" in name and cplx:
            return all(ulps(got[k], want[k], what + " " + k, ULP["cnorm"]) for k in arrs)
        if ".power" in name or ".sum" in name or ".normalize(power)" in name:
            return all(peak(got[k], want[k], what + " " + k) for k in arrs)
    elif group == "filter":
        # SciPy transforms a single-precision operand in single precision, whatever the result's type: field or taps
        if single or v[name.split(".")[0]].signal.dtype in SINGLE or v[name[name.index("(") + 1:-1]].dtype in SINGLE:
            return once()
        pk = max(float(np.max(np.abs(want[k]))) for k in arrs)
        return all(peak(got[k], want[k], what + " " + k, pk=pk) for k in arrs)
    elif group == "protocol" and name.startswith("np.abs(") and cplx is False and not single and v[name[7:-1]].signal.dtype.kind == "c":
        return all(ulps(got[k], want[k], what + " " + k, ULP["hypot"]) for k in arrs)
    return all(same(got[k], want[k]) for k in arrs)


def float32_result(group, name, v):
    """The cases the class leaves to raise on the GPU: real, imag and np.abs of a complex64 field."""
    if group == "methods" and name.endswith((".real", ".imag")):
        return v[name.split(".")[0]].signal.dtype == np.complex64
    return group == "protocol" and name.startswith("np.abs(") and v[name[7:-1]].signal.dtype == np.complex64


@pytest.mark.parametrize("group", oc.GROUPS)
def test_fixtures_with_uploaded_operands(group):
    gv.default()
    fix, v, host = load_group(group), load_namespace(dev), load_namespace()
    wide = {k: widen(x) for k, x in host.items()}
    signals = (optical_signal, electrical_signal)
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        for x in v.values():
            assert not isinstance(x, signals) or x.on_device, cid                    # no case brings an operand to the host
        d2h = _lib.TRANSFERS["d2h"]
        materialises = group == "protocol" and name.startswith(("asarray(", "np.exp(")) or name.endswith(".iter")
        try:
            with np.errstate(all="ignore"):
                r = fn(v)
        except Exception as e:                  # noqa: BLE001
            r = e
        if float32_result(group, name, host):
            assert isinstance(r, TypeError) and "float32" in str(r) and _lib.TRANSFERS["d2h"] == d2h, (cid, r)
            continue
        if isinstance(r, optical_signal) and not name.endswith(".sum") and not materialises:
            assert r.on_device and _lib.TRANSFERS["d2h"] == d2h, cid                 # the result lies on the device, nothing was read
        if materialises:
            v = load_namespace(dev)              # (np.asarray brought the operand to the host: upload it again)
        got = oc.describe(r, NULL)
        if not check_values(group, name, got, expected(fix, name), host, lambda fn=fn: oc.outcome(fn, wide, NULL)):
            bad.append((cid, {k: (str(a) if a.ndim == 0 else (a.dtype, a.shape)) for k, a in got.items()}))
    assert not bad, (len(bad), bad[:10])


def field(rng, shape, dtype, noise):
    def mk(s):
        a = rng.standard_normal(shape) * s
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.standard_normal(shape) * s
        return a.astype(dtype)
    return mk(1.0), (mk(0.05) if noise else None)


@pytest.mark.parametrize("n", SIZES)
def test_sweep_against_numpy(n):
    """Both row counts, the three types, every broadcast pairing ((rows, n) with itself, an (n,) field, a (2, 1) and a (1,) value, an
    electrical signal, a field of a wider type), every placement (device / host field, host array, scalar), noise on either side."""
    rng = np.random.default_rng(n)
    ok, level = True, (0 if n <= 257 else (1 if n < (1 << 20) else 2))
    for dtype in (np.float64, np.complex128, np.complex64):
        name = np.dtype(dtype).name
        single, cplx = np.dtype(dtype) == np.complex64, np.dtype(dtype).kind == "c"
        for rows in ((1, 2) if level < 2 else (2,)):
            shape = (n,) if rows == 1 else (2, n)
            sa, za = field(rng, shape, dtype, True)
            ha = O(sa, za, on=False)
            x = dev(ha)
            pairings = {"same": O(*field(rng, shape, dtype, True), on=False), "row": O(*field(rng, (n,), dtype, False), on=False),
                        "col": O(*field(rng, (2, 1), np.complex128 if cplx else np.float64, True), on=False), "one": O(*field(rng, (1,), dtype, False), on=False),
                        "electrical": electrical_signal(*field(rng, (n,), np.float64, True)), "wider": O(*field(rng, shape, np.complex128, True), on=False)}
            all_places = ("dev-dev", "dev-host", "host-dev")
            for pi, (pname, hb) in enumerate(pairings.items()):
                for place in (all_places if level == 0 else (all_places[(pi + rows + len(name)) % 3],)):
                    a = x if place != "host-dev" else ha
                    b = dev(hb) if place != "dev-host" else hb
                    tag = f"sweep n={n} {name} rows={rows} {pname} {place}"
                    d2h = _lib.TRANSFERS["d2h"]
                    res = []
                    for k, (sym, op) in enumerate(oc.OPS.items()):
                        if level == 2 and k != pi % 3:              # one operator per pairing at the largest sizes: the three share one loop
                            continue
                        try:
                            w = op(ha, hb)
                        except ValueError as e:                     # a lone noise of another shape: the constructor's error, on both paths
                            with pytest.raises(ValueError) as got:
                                op(a, b)
                            assert str(got.value) == str(e), tag
                            continue
                        res.append((sym, op(a, b), w))
                    assert _lib.TRANSFERS["d2h"] == d2h and all(r.on_device for _, r, _ in res), tag
                    for sym, r, w in res:
                        assert (r.noise is NULL) == (w.noise is NULL) and r.n_pol == w.n_pol, (tag, sym)
                        g_, w_ = oc.describe(r, NULL), oc.describe(w, NULL)
                        if sym == "*" and w.signal.dtype.kind == "c":
                            ok &= product_ok(g_, w_, ha, hb, f"{tag} *")
                        else:
                            assert all(same(g_[k], w_[k]) for k in w_), (tag, sym, {k: (g_[k].dtype, w_[k].dtype) for k in w_})
            arr = field(rng, (n,), dtype, False)[0]
            for bi, b in enumerate((arr, 1.75, np.float32(0.5), 2 - 1j) if level < 2 else (arr, 1.75)):       # dev-array, dev-scalar
                tag = f"sweep n={n} {name} rows={rows} dev-{type(b).__name__}"
                d2h = _lib.TRANSFERS["d2h"]
                fns = {"+": lambda q: q + b, "-": lambda q: q - b, "r": lambda q: b - q, "*": lambda q: q * b}
                if level == 2:                                      # the reflected difference of an array, the product with a scalar
                    fns = {k: fns[k] for k in ("r*"[bi],)}
                res = [f(x) for f in fns.values()]
                assert _lib.TRANSFERS["d2h"] == d2h and all(r.on_device for r in res), tag
                want = [f(ha) for f in fns.values()]
                for r, w, sym in zip(res, want, fns):
                    assert (r.noise is NULL) == (w.noise is NULL) and r.n_pol == w.n_pol, (tag, sym)
                    g_, w_ = oc.describe(r, NULL), oc.describe(w, NULL)
                    if sym == "*" and w.signal.dtype.kind == "c":
                        ok &= product_ok(g_, w_, ha, b, f"{tag} *")
                    else:
                        assert all(same(g_[k], w_[k]) for k in w_), (tag, sym, {k: (g_[k].dtype, w_[k].dtype) for k in w_})
            assert same(x == 0.5, ha == 0.5) and (level == 2 or same(x == dev(ha), ha == ha))
            # unary operations, slices and reductions
            fs = {"neg": lambda q: -q, "div_c": lambda q: q / (1.5 - 2j), "pow2": lambda q: q ** 2, "rev2": lambda q: q[::-2],
                  "row-1 cut": lambda q: q[rows - 1, n // 2:]}
            if level < 2:
                fs.update({"conj": lambda q: q.conj(), "div": lambda q: q / 3.0, "pow3": lambda q: q ** 3, "step3": lambda q: q[::3] if n > 2 else q[:],
                           "mid": lambda q: q[n // 3: n - n // 5 if n > 4 else n], "row-1": lambda q: q[-1, :] if rows == 2 else q[0, :],
                           "col": lambda q: q[:, n - 1]})
                if not single:
                    fs.update({"real": lambda q: q.real, "imag": lambda q: q.imag, "abs": lambda q: np.abs(q)})
                if not cplx:
                    fs.update({"floordiv": lambda q: q // 0.3, "pow1.7": lambda q: q ** 1.7})
            d2h = _lib.TRANSFERS["d2h"]
            outs = {k: f(x) for k, f in fs.items()}
            assert _lib.TRANSFERS["d2h"] == d2h and all(o.on_device for o in outs.values())
            hw = widen(ha)
            with np.errstate(all="ignore"):
                for k, f in fs.items():
                    o, w = outs[k], f(ha)
                    assert (o.noise is NULL) == (w.noise is NULL) and o.n_pol == w.n_pol and o.shape == w.shape, k
                    g_, w_ = oc.describe(o, NULL), oc.describe(w, NULL)
                    tag = f"sweep n={n} {name} rows={rows} {k}"
                    keys = [q for q in ("signal", "noise") if q in w_]
                    if cplx and k == "pow2":
                        ok &= product_ok(g_, w_, ha, ha, tag)
                    elif k == "div_c" or (single and k == "div"):
                        ok &= all(ulps(g_[q], w_[q], tag + " " + q, ULP["cquot"]) for q in keys)
                    elif single and k == "pow3":
                        ok &= rounded_once(g_["signal"], w_["signal"], f(hw).signal, tag)
                    elif cplx and k == "pow3":
                        ok &= cube_ok(g_["signal"], w_["signal"], ha, tag)
                    elif cplx and k == "abs":
                        ok &= ulps(g_["signal"], w_["signal"], tag, ULP["hypot"])
                    elif k in ("pow3", "pow1.7"):
                        ok &= ulps(g_["signal"], w_["signal"], tag, ULP["pow"])
                    else:                                               # NumPy's bits
                        assert all(same(g_[q], w_[q]) for q in w_), (tag, {q: (g_[q].dtype, w_[q].dtype) for q in w_})
            tag = f"sweep n={n} {name} rows={rows}"
            for of in (("signal", "noise", "all") if level < 2 else ("all",)):
                p1, p2, w = x.power("W", of), x.power("W", of), ha.power("W", of)
                assert same(p1, p2) and np.asarray(p1).dtype == np.asarray(w).dtype and np.shape(p1) == np.shape(w), (tag, of)
                if single:
                    ok &= rounded_once(p1, w, hw.power("W", of), f"{tag} power {of}")
                else:
                    ok &= peak(np.asarray(p1), np.asarray(w), f"{tag} power {of}", pk=float(np.max(ha.power("W", "all"))))
            s1, s2, w = x.sum(), x.sum(), ha.sum()
            assert same(s1.signal, s2.signal) and same(s1.noise, s2.noise) and not s1.on_device
            if single:
                ok &= rounded_once(s1.signal, w.signal, hw.sum().signal, f"{tag} sum")
            else:
                ok &= peak(s1.signal, w.signal, f"{tag} sum", pk=float(np.sum(np.abs(sa))))
            if level == 2:
                continue
            a1, a2, w = x.normalize("amplitude"), x.normalize("amplitude"), ha.normalize("amplitude")
            assert a1.on_device and a2.on_device and same(a1.signal, a2.signal)
            if single:
                ok &= rounded_once(a1.signal, w.signal, hw.normalize("amplitude").signal, f"{tag} normalize amplitude")
            elif cplx:
                ok &= ulps(a1.signal, w.signal, f"{tag} normalize amplitude", ULP["cnorm"])
            else:
                assert same(a1.signal, w.signal)
    assert ok


def test_every_key_form_at_the_first_and_last_row_and_column():
    n = 257
    rng = np.random.default_rng(2261)
    last = n - 1
    two = [slice(None), slice(0, 1), slice(last, None), slice(None, None, -1), slice(last, 0, -7), 0, 1, -1, -2, (0, 0), (1, last), (-1, -1), (0, slice(0, 1)),
           (1, slice(last, None)), (1, slice(None, None, -1)), (slice(None), 0), (slice(None), last), (slice(None), -n), (slice(None), slice(last, None)),
           (slice(None), slice(0, 1)), (slice(None), slice(None, None, -2)), (-2, slice(None)), (1, slice(-1, None, -1))]
    one = [slice(None), slice(0, 1), slice(last, None), slice(None, None, -1), 0, last, -1, -n, (0, 0), (0, last), (-1, slice(last, None)), (slice(None), 0),
           (slice(None), slice(0, 1)), (0, slice(None, None, -3))]
    errors = [2, -3, (2, 0), (0, n), (0, -n - 1), (slice(None), n), (0, 1, 2), "a", (0, "a"), slice(5, 5), (1, slice(9, 9)), (slice(None), slice(7, 7))]
    for dtype in (np.float64, np.complex128, np.complex64):
        for rows, keys in ((2, two), (1, one)):
            for noise in (False, True):
                h = O(*field(rng, (2, n) if rows == 2 else (n,), dtype, noise), on=False)
                x = dev(h)
                for key in keys + errors + ([n, -n - 1] if rows == 1 else []):
                    got, want = (oc.outcome(lambda v: v[key], q, NULL) for q in (x, h))
                    assert got.keys() == want.keys() and all(same(got[k], want[k]) for k in want), (np.dtype(dtype).name, rows, noise, key, got, want)
                assert x.on_device
    with pytest.raises(TypeError, match="an integer or a slice for the samples"):
        x[np.array([1, 2])]
    with pytest.raises(TypeError, match="an integer or ':' for the polarisation"):
        O(np.ones((2, 8), complex))[0:1, 2:4]


def test_the_entry_points_refuse_bad_shapes_types_and_devices():
    """Each refusal returns an error and launches nothing: the result buffer keeps its zeros."""
    lib = _lib.load()
    n = 64
    a = _lib.DeviceArray.from_host(np.ones((2, n), np.complex128))
    row = _lib.DeviceArray.from_host(np.ones(n, np.complex128))
    out = _lib.zeros_device((2, n), np.complex128)
    out_n = _lib.zeros_device((2, n), np.complex128)
    host = np.ones((2, n), np.complex128)
    P = _lib._ptr
    off = lambda d, b: ctypes.c_void_p(d.ptr + b)                            # noqa: E731  (an address inside a device array)
    binary = lambda *args: lib.ssfm_field_binary(*args)                      # noqa: E731
    good = (0, 1, 2, n, a, None, 2, n, row, None, 1, n, 0.0, 0.0, out, None)

    def with_(**kw):
        names = ("op", "dtype", "rows", "n", "s1", "n1", "rows1", "len1", "s2", "n2", "rows2", "len2", "re2", "im2", "out", "out_n")
        args = dict(zip(names, good))
        args.update(kw)
        return tuple(args[k] for k in names)
    refusals = {"op": with_(op=4), "op high": with_(op=6), "dtype": with_(dtype=3), "rows": with_(rows=3, rows1=3), "n": with_(n=0, len1=0, len2=0),
                "rows1": with_(rows1=1, rows2=1), "len1": with_(len1=n - 1), "len2": with_(len2=2), "rows2": with_(rows2=3),
                "no first operand": with_(s1=None), "no result": with_(out=None), "noise without out_noise": with_(n1=a), "out_noise without noise": with_(out_n=out_n),
                "scalar with noise": with_(s2=None, n2=row), "host memory": with_(s1=P(host)), "host second operand": with_(s2=P(host[0])),
                "misaligned operand": with_(s2=off(row, 8), len2=1), "misaligned result": with_(out=off(out, 8), rows=1, rows1=1, s1=row)}
    for what, args in refusals.items():
        assert binary(*args) != 0, what
        assert lib.ssfm_last_error(), what
    assert not out.to_host().any() and not out_n.to_host().any()                              # nothing was launched
    assert binary(*good) == 0
    assert np.array_equal(out.to_host(), np.full((2, n), 2.0 + 0j))
    _lib.api.ssfm_device_copy(0, out, None, out.nbytes, _lib.COPY_ZERO)
    c64 = _lib.DeviceArray.from_host(np.ones((2, n), np.complex64))
    o64 = _lib.zeros_device((2, n), np.complex64)
    assert lib.ssfm_field_unary(5, 0, 2, n, c64, None, 0.0, 0.0, 0, o64, None) == 2            # real of complex64: unsupported
    assert lib.ssfm_field_unary(0, 0, 3, n, c64, None, 0.0, 0.0, 0, o64, None) == 1            # rows
    assert lib.ssfm_field_unary(2, 0, 2, n, c64, None, 0.0, 0.0, 0, o64, None) == 1            # division by zero
    assert lib.ssfm_field_unary(0, 0, 2, n, c64, c64, 0.0, 0.0, 0, o64, None) == 1             # noise without out_noise
    assert lib.ssfm_field_unary(0, 0, 2, n, P(host), None, 0.0, 0.0, 0, o64, None) == 1        # host memory
    assert lib.ssfm_field_unary(0, 7, 2, n, c64, None, 0.0, 0.0, 0, o64, None) == 1            # dtype
    h64 = np.zeros((2, n), np.complex64)
    assert lib.ssfm_field_unary(0, 0, 2, n, c64, None, 0.0, 0.0, 0, P(h64), None) == 1          # a result in host memory
    assert lib.ssfm_field_unary(0, 0, 2, n, c64, P(h64), 0.0, 0.0, 0, o64, o64) == 1            # a noise in host memory
    assert lib.ssfm_field_slice(1, 2, n, a, None, 0, 2, 0, 1, 4, P(host), None) == 1            # a result in host memory
    assert lib.ssfm_field_slice(1, 2, n, a, None, 0, 2, 1, 2 ** 62, 3, out, None) == 1          # a step that would overflow the last index
    assert lib.ssfm_field_slice(1, 2, n, a, None, 0, 2, 1, 1, 2 ** 62, out, None) == 1          # a count beyond the row
    assert not h64.any()
    for args in ((1, 2, n, a, None, 2, 1, 0, 1, n), (1, 2, n, a, None, 0, 3, 0, 1, n), (1, 2, n, a, None, -1, 1, 0, 1, n), (1, 2, n, a, None, 0, 2, n, 1, 1),
                 (1, 2, n, a, None, 0, 2, 0, 1, n + 1), (1, 2, n, a, None, 0, 2, 5, -1, 7), (1, 2, n, a, None, 0, 2, 0, 0, 4), (1, 2, n, a, None, 0, 2, -1, 1, 4),
                 (1, 2, n, a, None, 0, 0, 0, 1, 4), (1, 2, n, a, None, 0, 2, 0, 1, 0), (5, 2, n, a, None, 0, 2, 0, 1, 4), (1, 3, n, a, None, 0, 2, 0, 1, 4),
                 (1, 2, n, P(host), None, 0, 2, 0, 1, 4)):
        assert lib.ssfm_field_slice(*args, out, None) == 1, args
    assert lib.ssfm_field_slice(1, 2, n, a, a, 0, 2, 0, 1, 4, out, None) == 1                   # noise without out_noise
    res = (ctypes.c_double * 4)()
    assert lib.ssfm_field_reduce(0, 3, n, a, None, 1, res) == 1 and lib.ssfm_field_reduce(3, 2, n, a, None, 1, res) == 1
    assert lib.ssfm_field_reduce(0, 2, 0, a, None, 1, res) == 1 and lib.ssfm_field_reduce(0, 2, n, P(host), None, 1, res) == 1
    assert lib.ssfm_field_reduce(0, 2, n, a, off(a, 8), 1, res) == 1                            # a noise that starts off 16 bytes
    assert not out.to_host().any() and not out_n.to_host().any() and not o64.to_host().any()   # nothing was launched
    x = optical_signal.from_device(a)
    assert same((-x).signal, -np.ones((2, n), np.complex128))                                   # the library goes on working after a refusal
    assert same(x.power(), np.ones(2))


def test_types_shapes_and_devices_the_class_refuses():
    x, short = O(np.ones((2, 8), complex)), O(np.ones(5, complex))
    before = dict(_lib.TRANSFERS)
    with pytest.raises(TypeError, match="float64, complex128 and complex64"):
        optical_signal.from_device(_lib.DeviceArray((8,), np.uint8)) + 1
    with pytest.raises(TypeError, match="float64, complex128 and complex64"):
        x * optical_signal.from_device(_lib.DeviceArray((8,), np.int64))
    with pytest.raises(ValueError, match=r"Can't operate 'optical_signal's with shapes \(2, 8\) and \(5,\)"):
        x + short
    with pytest.raises(ValueError, match="integer exponents below 100 and 0.5"):
        x ** 1.5
    with pytest.raises(ValueError, match="same dimensionality"):
        x.filter(np.ones(3))
    for zero in (0, 0.0, 0j, np.float64(0)):
        with pytest.raises(ZeroDivisionError, match="Can't divide electrical_signal by zero"):
            x / zero
    fake = optical_signal.from_device(_lib.DeviceArray((2, 8), np.complex128, 0))
    fake._raw("signal").device = 1               # (one GPU here: the check reads the arrays' device numbers before anything is launched)
    try:
        with pytest.raises(ValueError, match="different GPUs"):
            x + fake
    finally:
        fake._raw("signal").device = 0
    assert _lib.TRANSFERS == before and x.on_device


def test_chain_between_devices_without_host_transfers():
    """FIBER -> * g -> + other -> [:, :n] -> BPF -> PD: nothing crosses PCIe between the fibre's output and the photodetector's."""
    from opticomlib_amd import BPF, FIBER, PD
    gv(sps=16, R=10e9)
    rng = np.random.default_rng(5)
    n = 1 << 13
    a = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.03
    lo = O(((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.003).astype(np.complex64))
    x = FIBER(optical_signal(a), length=5, h=1.0, alpha=0.2, beta_2=-21.7, gamma=1.3)
    assert x.on_device and x._raw("signal").dtype == np.complex64
    ref = optical_signal(x._raw("signal").to_host())
    hlo = optical_signal(lo._raw("signal").to_host())
    assert x.on_device and lo.on_device
    before = dict(_lib.TRANSFERS)
    y = (x * np.float32(1.5) + lo)[:, :n - 37]
    mid = dict(_lib.TRANSFERS)
    assert mid == before and y.on_device and y.shape == (2, n - 37) and y._raw("signal").dtype == np.complex64
    z = (x * 1.5 - lo)[1, 5:n // 2]                              # a Python float is a float64 array in the reference: complex128 from here
    assert _lib.TRANSFERS == before and z.on_device and z.shape == (n // 2 - 5,) and z._raw("signal").dtype == np.complex128
    v = PD(BPF(y, BW=20e9), BW=7.5e9, r=1.0, rng="device")
    assert _lib.TRANSFERS["d2h"] == before["d2h"] and v.on_device
    # the products to their bound; from the device's own products on, sums and cuts are NumPy's bits
    y1, z1 = x * np.float32(1.5), x * 1.5
    assert product_ok(oc.describe(y1, NULL), oc.describe(ref * np.float32(1.5), NULL), ref, np.float32(1.5), "chain complex64")
    assert product_ok(oc.describe(z1, NULL), oc.describe(ref * 1.5, NULL), ref, 1.5, "chain complex128")
    assert same(y.signal, (optical_signal(y1.signal) + hlo)[:, :n - 37].signal)
    assert same(z.signal, (optical_signal(z1.signal) - hlo)[1, 5:n // 2].signal)


def test_each_operation_twice_gives_identical_bytes():
    rng = np.random.default_rng(9)
    n = 65535
    for dtype in (np.float64, np.complex128, np.complex64):
        x, y, r = O(*field(rng, (2, n), dtype, True)), O(*field(rng, (2, n), dtype, True)), O(*field(rng, (n,), dtype, False))
        ops = [lambda: x + y, lambda: x - r, lambda: x * y, lambda: r * x, lambda: 2.5 - x, lambda: -x, lambda: x.conj(), lambda: x / (2 - 1j), lambda: x ** 2,
               lambda: x ** 3, lambda: x[:, ::-3], lambda: x[1], lambda: x.normalize("amplitude")]
        for i, f in enumerate(ops):
            p, q = f(), f()
            assert same(p.signal, q.signal) and same(p.noise, q.noise), (np.dtype(dtype).name, i)
        assert same(x.power(), x.power()) and same(x.sum().signal, x.sum().signal) and same(x == y, x == y)


def test_the_example_prints_equal_transfer_counters():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "optical_algebra.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "transfers during the algebra: h2d +0, d2h +0; results on the GPU: True" in out.stdout
