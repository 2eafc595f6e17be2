"""The electrical_signal algebra on the MI355X: every fixture again with the operands uploaded first, a sweep against live NumPy / SciPy at tile
and grid edges, values at the edges of float64, phase() and filter() on their hard inputs, a chain without host transfers, determinism.

Bounds.  eps = 2^-52; "u" below is a distance in units of eps |want| (of the modulus for complex values), which is never less than the distance
in ulps.
* Real-typed + - * neg [] > == floor, abs of reals, conj, real, imag, real ** 0.5 and ** -1 (sqrt and the reciprocal, correctly rounded on the
  device as in NumPy), and the quotient by a REAL scalar of a complex signal (NumPy's Smith loop restated operation by operation, every one
  correctly rounded): NumPy's bits.
* Complex products and the three-term noise, x ** 2 with its noise 2 s n + n^2 included: elementwise |d| <= 8 eps (|s1||s2| resp.
  |s1||n2| + |n1||s2| + |n1||n2|).  Complex ** 3 is two such products: elementwise |d| <= 2 x 8 eps |s + n|^3.
* The quotient by a COMPLEX scalar and complex ** -1 (NumPy's reciprocal loop) restate NumPy's loops in correctly rounded operations
  (documented error 0): 0 + 1 u for NumPy's own rounding, should its build fuse a multiply-add.
* abs of complex, general ** of reals and the angle rest on the device's hypot, pow and atan2.  "HIP math API" of the HIP documentation for
  ROCm 7.2 (reference/math_api, table "Double precision mathematical functions") lists a maximum error of 1 ulp for each of hypot, pow and
  atan2: 1 + 1 (NumPy's own rounding) = 2 u.
* Complex ** 0.5 is t = sqrt((|re| + hypot) / 2) and im / 2t: relative error of t <= (1 (hypot) + 1/2 (the sum)) / 2 + 1/2 (sqrt) = 1.25 eps, of
  the quotient 1.25 + 1/2 = 1.75 eps, + 1 for NumPy = 2.75 u.  normalize('amplitude') of a complex signal divides by max hypot: 2 + 1 = 3 u.
* power, sum, filter and what is divided by a power (normalize('power')): 1e-12 of the peak.
* phase(): NumPy and the device each against the exact restatement (NumPy's angles, its integer wrap counts, times 2 pi in longdouble); the
  device may be no further from it than NumPy is, plus the atan2 distance (2 eps pi, the largest angle).
Every measured distance is recorded (tools/margins_digest.py folds the records into profiles/signal_ops_margins.txt).  In filter() with real
signal, noise and taps the noise rides as the imaginary part of the signal's field: the 1e-12 is of the peak of both together, and a noise
far below 1e-12 of the signal loses digits on that path (the test noise is within a factor 10^3 of the signal)."""
import os

import numpy as np
import pytest
import scipy.signal as sg

import margins
import signal_cases as sc
from opticomlib_amd import NULL, _lib, binary_sequence, electrical_signal, gv
from test_signal_algebra_cpu import CASES, expected, load_group, load_namespace, same

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 65535, 1 << 20, (1 << 20) + 1, 1 << 21)
ULP = {"hypot": 2.0, "pow": 2.0, "atan2": 2.0, "cquot": 1.0, "csqrt": 2.75, "cnorm": 3.0}
SCALARS = {"2": 2, "2.5": 2.5, "3+2j": 3 + 2j, "-0.0": -0.0}


def dev(x):
    up = lambda a: _lib.DeviceArray.from_host(np.ascontiguousarray(a))       # noqa: E731
    return electrical_signal.from_device(up(x.signal), NULL if x.noise is NULL else up(x.noise))


def E(s, n=None, on=True):
    x = electrical_signal(s) if n is None else electrical_signal(s, n)
    return dev(x) if on else x


def ulps(got, want, what, bound):
    """Largest |got - want| in units of eps |want| (of the modulus for complex values); recorded, then held to `bound`."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(want[fin]), np.finfo(np.float64).tiny) * EPS
        d = float(np.max(np.abs(got[fin] - want[fin]) / scale)) if fin.any() else 0.0
    return margins.within(got, want, bound=bound, what=f"{what} [ulp]", measured=d)


def peak(got, want, what, bound=1e-12, pk=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
    fin = np.isfinite(want)
    if not fin.all():                            # (-inf dBm of a zero power: the value itself, nothing to measure)
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
        if not fin.any():
            return True
    pk = float(np.max(np.abs(want[fin]))) if pk is None else pk
    return margins.within(got, want, bound=bound, what=what, measured=float(np.max(np.abs(got[fin] - want[fin]))) / (pk or 1.0))


def parts(x):
    """(|signal|, |noise| or 0) of an operand: a signal, an array or a scalar."""
    if isinstance(x, electrical_signal):
        return np.abs(x.signal), (0.0 if x.noise is NULL else np.abs(x.noise))
    return np.abs(np.asarray(x)), 0.0


def product_ok(got, want, a, b, what):
    """|d| <= 8 eps |s1||s2| for the signal and 8 eps (|s1||n2| + |n1||s2| + |n1||n2|) for the noise, elementwise."""
    (s1, n1), (s2, n2) = parts(a), parts(b)
    ok = True
    for key, m in (("signal", s1 * s2), ("noise", s1 * n2 + n1 * s2 + n1 * n2)):
        if key in want:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape
            d = np.abs(got[key] - want[key])
            bound = 8 * EPS * m
            worst = float(np.max(d / np.maximum(bound, np.finfo(np.float64).tiny)))
            ok &= margins.within(got[key], want[key], bound=1.0, what=f"{what} {key} [|d| / (8 eps terms)]", measured=worst)
    return ok


def cube_ok(got, want, x, what):
    """Complex ** 3 = (z z) z: two products, elementwise |d| <= 2 x 8 eps |z|^3 with z = signal + noise."""
    z = np.abs(np.asarray(x.signal + x.noise))
    assert got.dtype == want.dtype and got.shape == want.shape
    worst = float(np.max(np.abs(got - want) / np.maximum(16 * EPS * z ** 3, np.finfo(np.float64).tiny)))
    return margins.within(got, want, bound=1.0, what=f"{what} [|d| / (16 eps |z|^3)]", measured=worst)


def split_id(name, v):
    for i, ch in enumerate(name):
        if ch in "+-*" and i > 0 and (name[:i] in v or name[:i] in SCALARS) and (name[i + 1:] in v or name[i + 1:] in SCALARS):
            return name[:i], ch, name[i + 1:]
    raise AssertionError(name)


def phase_ok(z, got, what):
    """NumPy and the device each against the exact restatement: the angles NumPy takes, its integer wrap counts, times 2 pi in longdouble.
    The device may be no further from it than NumPy is, plus the atan2 distance (2 ulp of pi, the largest angle)."""
    ang = np.angle(z)
    want = np.unwrap(ang)
    turns = np.rint((want - ang) / (2 * np.pi)).astype(np.int64)
    exact = ang.astype(np.longdouble) + turns.astype(np.longdouble) * (2 * np.longdouble(np.pi))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    d_np = float(np.max(np.abs(want[fin] - exact[fin]))) if fin.any() else 0.0
    d_dev = float(np.max(np.abs(got[fin] - exact[fin]))) if fin.any() else 0.0
    slack = ULP["atan2"] * EPS * np.pi
    margins.record(f"{what} numpy vs exact [rad]", None, d_np, d_np + slack)
    return margins.within(got, want, bound=d_np + slack, what=f"{what} device vs exact [rad]", measured=d_dev)


def check_values(group, name, got, want, v):
    """The bound that belongs to the case (module docstring)."""
    what = f"{group}/{name}"
    if want.keys() != got.keys():
        return False
    kind = str(want["kind"])
    if kind == "error":
        return str(want["type"]) == str(got["type"]) and str(want["text"]) == str(got["text"])
    arrs = [k for k in want if k in ("signal", "noise", "data", "value")]
    if kind == "signal" and str(want["cls"]) != str(got["cls"]):
        return False
    cplx = any(want[k].dtype.kind == "c" for k in arrs)
    if group in ("binary", "reflected"):
        a, op, b = split_id(name, v)
        if op == "*" and cplx:
            return product_ok(got, want, v[a] if a in v else SCALARS[a], v[b] if b in v else SCALARS[b], what)
    elif group == "scalar" and "/" in name and "//" not in name and cplx:
        if name.split("/")[1] != "1+1j":                   # a real divisor: NumPy's bits
            return all(same(got[k], want[k]) for k in arrs)
        return all(ulps(got[k], want[k], what + " " + k, ULP["cquot"]) for k in arrs)
    elif group == "pow":
        x, p = v[name.split("**")[0]], name.split("**")[1]
        if cplx and p in ("2", "2.0"):
            return product_ok(got, want, x, x, what)
        if cplx and p == "3":
            return cube_ok(got["signal"], want["signal"], x, what)
        if cplx and p in ("-1", "0.5"):
            return ulps(got["signal"], want["signal"], what, ULP["cquot"] if p == "-1" else ULP["csqrt"])
        if p == "3":
            return ulps(got["signal"], want["signal"], what, ULP["pow"])
    elif group == "methods":
        if ".abs(" in name and name.startswith("xc"):
            return all(ulps(got[k], want[k], what + " " + k, ULP["hypot"]) for k in arrs)
        if ".normalize(amplitude)" in name and cplx:
            return all(ulps(got[k], want[k], what + " " + k, ULP["cnorm"]) for k in arrs)
        if ".power" in name or ".sum" in name or ".normalize(power)" in name:
            return all(peak(got[k], want[k], what + " " + k) for k in arrs)
        if ".phase" in name:
            x = v[name.split(".")[0]]
            return phase_ok(np.asarray(x.signal + x.noise), got["signal"], what)
    elif group == "filter":
        pk = max(float(np.max(np.abs(want[k]))) for k in arrs)
        return all(peak(got[k], want[k], what + " " + k, pk=pk) for k in arrs)
    elif group == "protocol" and name.startswith("np.abs(xc"):
        return all(ulps(got[k], want[k], what + " " + k, ULP["hypot"]) for k in arrs)
    return all(same(got[k], want[k]) for k in arrs)


@pytest.mark.parametrize("group", sc.GROUPS)
def test_fixtures_with_uploaded_operands(group):
    gv.default()
    fix, v, host = load_group(group), load_namespace(dev), load_namespace()
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        for x in v.values():
            assert not isinstance(x, electrical_signal) or x.on_device, cid          # no case brings an operand to the host
        d2h = _lib.TRANSFERS["d2h"]
        materialises = group == "protocol" and not name.startswith(("np.abs", "np.add"))
        try:
            with np.errstate(all="ignore"):
                r = fn(v)
        except Exception as e:                  # noqa: BLE001
            r = e
        if isinstance(r, electrical_signal) and not name.endswith(".sum") and not materialises:
            assert r.on_device and _lib.TRANSFERS["d2h"] == d2h, cid                 # the result lies on the device, nothing was read
        if isinstance(r, binary_sequence):
            assert hasattr(r._raw(), "ptr") and _lib.TRANSFERS["d2h"] == d2h, cid
        if materialises:
            v = load_namespace(dev)              # (np.asarray brought the operand to the host: upload it again)
        got = sc.describe(r, NULL)
        if not check_values(group, name, got, expected(fix, name), host):
            bad.append((cid, {k: (str(a) if a.ndim == 0 else a.dtype) for k, a in got.items()}))
    assert not bad, bad[:10]


def operands(n, rng, cplx, noise):
    mk = (lambda s: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * s) if cplx else (lambda s: rng.standard_normal(n) * s)
    return mk(1.0), (mk(0.05) if noise else None)


@pytest.mark.parametrize("n", SIZES)
def test_sweep_against_numpy(n):
    """Every operand placement (device / host signal, host array, scalar), noise on either, both or neither side, real and complex."""
    rng = np.random.default_rng(n)
    ok = True
    for cplx in (False, True):
        for na, nb in ((False, False), (True, False), (False, True), (True, True)):
            (sa, za), (sb, zb) = operands(n, rng, cplx, na), operands(n, rng, cplx and nb, nb)
            ha, hb = E(sa, za, on=False), E(sb, zb, on=False)
            for place in ("dev-dev", "dev-host", "host-dev", "dev-array", "dev-scalar"):
                a = E(sa, za) if place != "host-dev" else ha
                b = {"dev-dev": E(sb, zb), "dev-host": hb, "host-dev": E(sb, zb), "dev-array": sb, "dev-scalar": 1.75}[place]
                hb_ = {"dev-array": sb, "dev-scalar": 1.75}.get(place, hb)
                d2h = _lib.TRANSFERS["d2h"]
                res = [a + b, a - b, a * b, a > b]
                assert _lib.TRANSFERS["d2h"] == d2h and all(r.on_device for r in res[:3])
                want = [ha + hb_, ha - hb_, ha * hb_, ha > hb_]
                for r, w, op in zip(res[:3], want[:3], "+-*"):
                    assert (r.noise is NULL) == (w.noise is NULL), (place, op)
                    g_, w_ = sc.describe(r, NULL), sc.describe(w, NULL)
                    if op == "*" and r.signal.dtype.kind == "c":
                        ok &= product_ok(g_, w_, ha, hb_, f"sweep n={n} {place} *")
                    else:
                        assert all(same(g_[k], w_[k]) for k in w_), (n, place, op, cplx, na, nb)
                assert same(res[3].data, want[3].data), (n, place)
            x = E(sa, za)
            hx = ha
            d2h = _lib.TRANSFERS["d2h"]
            outs = {"neg": -x, "conj": x.conj(), "real": x.real, "imag": x.imag, "div": x / 3.0, "pow2": x ** 2, "abs_s": x.abs("signal"), "abs_all": x.abs(),
                    "step3": x[::3] if n > 2 else x[:], "rev2": x[::-2], "mid": x[n // 3: n - n // 5 if n > 4 else n]}
            outs.update({"div_c": x / (1.5 - 2j), "pow3": x ** 3, "pow-1": x ** -1, "pow0.5": x ** 0.5})
            if not cplx:
                outs.update({"floordiv": x // 0.3, "pow1.7": x ** 1.7, "pow-2.5": x ** -2.5})
            assert _lib.TRANSFERS["d2h"] == d2h and all(o.on_device for o in outs.values())
            with np.errstate(all="ignore"):
                ref = {"neg": -hx, "conj": hx.conj(), "real": hx.real, "imag": hx.imag, "div": hx / 3.0, "pow2": hx ** 2, "abs_s": hx.abs("signal"), "abs_all": hx.abs(),
                       "step3": hx[::3] if n > 2 else hx[:], "rev2": hx[::-2], "mid": hx[n // 3: n - n // 5 if n > 4 else n]}
                ref.update({"div_c": hx / (1.5 - 2j), "pow3": hx ** 3, "pow-1": hx ** -1, "pow0.5": hx ** 0.5})
                if not cplx:
                    ref.update({"floordiv": hx // 0.3, "pow1.7": hx ** 1.7, "pow-2.5": hx ** -2.5})
            for k, o in outs.items():
                w = ref[k]
                assert (o.noise is NULL) == (w.noise is NULL), k
                g_, w_ = sc.describe(o, NULL), sc.describe(w, NULL)
                tag = f"sweep n={n} {'c' if cplx else 'r'} {k}"
                if cplx and k == "pow2":
                    ok &= product_ok(g_, w_, hx, hx, tag)
                elif k == "div_c":
                    ok &= all(ulps(g_[q], w_[q], tag + " " + q, ULP["cquot"]) for q in ("signal", "noise") if q in w_)
                elif cplx and k == "pow3":
                    ok &= cube_ok(g_["signal"], w_["signal"], hx, tag)
                elif cplx and k in ("pow-1", "pow0.5"):
                    ok &= ulps(g_["signal"], w_["signal"], tag, ULP["cquot"] if k == "pow-1" else ULP["csqrt"])
                elif cplx and k.startswith("abs"):
                    ok &= ulps(g_["signal"], w_["signal"], tag, ULP["hypot"])
                elif k in ("pow3", "pow1.7", "pow-2.5"):
                    ok &= ulps(g_["signal"], w_["signal"], tag, ULP["pow"])
                else:                                       # NumPy's bits (the quotient of complex values by 3.0, real ** 0.5 and ** -1 among them)
                    assert all(same(g_[q], w_[q]) for q in w_), (n, cplx, k)
            # reductions, each twice: the same bits
            for of in ("signal", "noise", "all"):
                p1, p2 = x.power("W", of), x.power("W", of)
                assert p1 == p2 or (np.isnan(p1) and np.isnan(p2))
                ok &= peak(np.float64(p1), np.float64(hx.power("W", of)), f"sweep n={n} power {of}", pk=float(hx.power("W", "all")))
            s1, s2 = x.sum(), x.sum()
            assert same(s1.signal, s2.signal)
            ok &= peak(s1.signal, hx.sum().signal, f"sweep n={n} sum", pk=float(np.sum(np.abs(sa))))
            a1, a2 = x.normalize("amplitude"), x.normalize("amplitude")
            assert same(a1.signal, a2.signal)
            w = hx.normalize("amplitude")
            if cplx:
                ok &= ulps(a1.signal, w.signal, f"sweep n={n} normalize amplitude", ULP["cnorm"])
            else:
                assert same(a1.signal, w.signal)
            ok &= peak(x.normalize().signal, hx.normalize().signal, f"sweep n={n} normalize power")
            ok &= phase_ok(np.asarray(hx.signal + hx.noise), x.phase().signal, f"sweep n={n} {'c' if cplx else 'r'} phase")
    assert ok


def test_values_at_the_edges():
    tiny = np.finfo(np.float64).tiny
    s = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 5e-324, -5e-324, tiny / 4, 1.0, -1.0, 1e308, -1e308, 2.5])
    z = np.array([1.0, np.nan, 2.0, -0.0, -0.0, 5e-324, 3.0, tiny / 8, np.inf, -0.0, 1e308, 1e308, -2.5])
    x, y, hx, hy = E(s, z), E(z, s), E(s, z, on=False), E(z, s, on=False)
    with np.errstate(all="ignore"):
        for name, f in (("add", lambda a, b: a + b), ("sub", lambda a, b: a - b), ("rsub", lambda a, b: 2.0 - a), ("mul", lambda a, b: a * b), ("neg", lambda a, b: -a),
                        ("div", lambda a, b: a / -3.0), ("floordiv", lambda a, b: a // 0.7), ("pow2", lambda a, b: a ** 2), ("abs", lambda a, b: a.abs("noise")),
                        ("slice", lambda a, b: a[::-3]), ("scalar -0.0", lambda a, b: a + -0.0), ("times 0", lambda a, b: a * 0.0)):
            g, w = f(x, y), f(hx, hy)
            for k in ("signal", "noise"):
                gk, wk = getattr(g, k), getattr(w, k)
                assert (gk is NULL) == (wk is NULL), name
                if wk is not NULL:
                    assert same(gk, wk) and np.array_equal(np.signbit(gk), np.signbit(wk)), (name, k, gk, wk)
        assert same((x > y).data, (hx > hy).data) and same(x == y, hx == hy) and same((x < 0.5).data, (hx < 0.5).data)
        # ** of negative reals with a fractional exponent: NaN, as NumPy
        for p in (0.5, 1.5, -0.3, -1, 3):
            assert ulps((x ** p).signal, (hx ** p).signal, f"edges ** {p}", ULP["pow"])
    # complex values with zero, signed-zero, infinite and NaN parts: NumPy's bits where the operation restates NumPy's, its NaNs and infinities elsewhere
    parts_ = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5]
    cs = np.array([complex(a, b) for a in parts_ for b in parts_])
    cz = np.roll(cs, 3) * 0.5
    cz[np.isnan(cz)] = 0.25 - 1j
    cx, hcx, cy, hcy = E(cs, cz), E(cs, cz, on=False), E(cz), E(cz, on=False)
    with np.errstate(all="ignore"):
        for name, f in (("c add", lambda a, b: a + b), ("c sub", lambda a, b: a - b), ("c rsub", lambda a, b: (1 - 2j) - a), ("c mul", lambda a, b: a * b),
                        ("c scalar mul", lambda a, b: a * (0.0 + 1j)), ("c neg", lambda a, b: -a), ("c conj", lambda a, b: a.conj()), ("c real", lambda a, b: a.real),
                        ("c imag", lambda a, b: a.imag), ("c div real", lambda a, b: a / -3.0), ("c div complex", lambda a, b: a / (2 - 1j)),
                        ("c pow2", lambda a, b: a ** 2), ("c pow3", lambda a, b: b ** 3), ("c pow-1", lambda a, b: b ** -1), ("c pow-2", lambda a, b: b ** -2),
                        ("c pow0.5", lambda a, b: b ** 0.5), ("c abs", lambda a, b: a.abs("signal")), ("c abs all", lambda a, b: a.abs()), ("c slice", lambda a, b: a[::-2])):
            g, w = f(cx, cy), f(hcx, hcy)
            for k in ("signal", "noise"):
                gk, wk = getattr(g, k), getattr(w, k)
                assert (gk is NULL) == (wk is NULL), name
                if wk is NULL:
                    continue
                assert gk.dtype == wk.dtype and gk.shape == wk.shape, name
                if name in ("c pow3", "c pow-2", "c pow0.5", "c abs", "c abs all", "c div complex", "c pow-1"):
                    # the same NaNs and infinities; finite values to the bound of the operation
                    fin = np.isfinite(wk)
                    assert np.array_equal(np.isnan(gk.real), np.isnan(wk.real)) and np.array_equal(np.isnan(gk.imag), np.isnan(wk.imag)), (name, k, gk, wk)
                    assert np.array_equal(gk[~fin & ~np.isnan(wk)], wk[~fin & ~np.isnan(wk)]), (name, k, gk, wk)
                    bound = {"c pow3": 16.0, "c pow-2": 9.0, "c pow0.5": ULP["csqrt"], "c abs": ULP["hypot"], "c abs all": ULP["hypot"]}.get(name, ULP["cquot"])
                    assert ulps(np.where(fin, gk, 0), np.where(fin, wk, 0), f"edges {name} {k}", bound), (name, k)
                else:
                    assert same(gk, wk), (name, k, gk, wk)
        assert same((cx > cy).data, (hcx > hcy).data) and same(cx == cy, hcx == hcy) and same((cy == cy), (hcy == hcy))
    launches = dict(_lib.TRANSFERS)
    for zero in (0, 0.0, 0j, np.float64(0)):
        with pytest.raises(ZeroDivisionError, match="Can't divide electrical_signal by zero"):
            x / zero
        with pytest.raises(ZeroDivisionError):
            x // zero
    assert _lib.TRANSFERS == launches and x.on_device
    with pytest.raises(ValueError, match="invalid shape \\(0,\\)"):
        x[5:5]
    with pytest.raises(TypeError, match="float64 and complex128"):
        E(np.ones(4, np.complex64)) + 1
    with pytest.raises(ValueError, match="integer exponents below 100 and 0.5"):
        E(np.ones(4, np.complex128)) ** 1.5


def test_phase_on_hard_inputs():
    n = 1 << 20
    k = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(7)
    ok = True
    chirp = np.exp(1j * (2.9 * k / n) * k)                               # the step between neighbours grows to 5.8 rad: > 10^5 wraps
    assert np.count_nonzero(np.abs(np.diff(np.angle(chirp))) >= np.pi) > 10 ** 5
    steps = np.exp(1j * np.pi * np.cumsum(rng.integers(-1, 2, 4096)))     # steps of exactly +-pi (and none) between -1 and 1
    exact_pi = np.array([1.0, -1.0, 1.0, -1.0, -1.0, 1.0]) + 0j
    cases = {"chirp": (chirp, None), "constant": (np.full(1000, 0.3 - 0.4j), None), "pi steps": (steps, None), "exact pi": (exact_pi, None),
             "real signs": (np.array([1.0, -1.0, -2.0, 3.0, -0.0, 0.0, -1.0]), None),
             "noisy zero crossing": (np.linspace(1, -1, 4001) + 0j, (rng.standard_normal(4001) + 1j * rng.standard_normal(4001)) * 1e-3)}
    for name, (s, z) in cases.items():
        x = E(s, z)
        d2h = _lib.TRANSFERS["d2h"]
        p = x.phase()
        assert p.on_device and p.noise is NULL and _lib.TRANSFERS["d2h"] == d2h
        ok &= phase_ok(s if z is None else s + z, p.signal, "phase " + name)
    assert ok


def direct_at(x, h, idx):
    """'same' convolution of x with h at the outputs `idx` by the direct sum in longdouble."""
    n, taps = x.size, h.size
    ct = np.clongdouble if (np.iscomplexobj(x) or np.iscomplexobj(h)) else np.longdouble
    xl, hl, out = x.astype(ct), h.astype(ct), np.zeros(len(idx), ct)
    for q, i in enumerate(idx):
        j = i + (taps - 1) // 2                             # index in the full output
        lo, hi = max(0, j - taps + 1), min(n - 1, j)
        out[q] = np.sum(xl[lo:hi + 1] * hl[j - hi:j - lo + 1][::-1])
    return out.astype(np.complex128 if ct is np.clongdouble else np.float64)


def test_filter_against_scipy():
    rng = np.random.default_rng(11)
    ok, kept = True, 0
    for n in (100, 4096, 100000):
        for taps in (1, 2, 8, 129, n + 37):
            for ch in (False, True):
                for cx in (False, True):
                    for noise in (False, True):
                        (s, z) = operands(n, rng, cx, noise)
                        h = rng.standard_normal(taps) + (1j * rng.standard_normal(taps) if ch else 0)
                        h = h / max(1.0, np.sqrt(taps))
                        want_s = sg.fftconvolve(s, h, mode="same")
                        want_n = None if z is None else sg.fftconvolve(z, h, mode="same")
                        # SciPy itself within 1e-12 of the direct sum, in longdouble at 48 outputs (the ends among them), signal and noise;
                        # an input for which it is not is dropped
                        idx = np.unique(np.concatenate([[0, n - 1, n // 2], rng.integers(0, n, 45)]))
                        if any(float(np.max(np.abs(w[idx] - direct_at(a, h, idx)))) / float(np.max(np.abs(w))) >= 1e-12
                               for a, w in ((s, want_s), (z, want_n)) if a is not None):
                            continue
                        kept += 1
                        x = E(s, z)
                        d2h = _lib.TRANSFERS["d2h"]
                        y = x.filter(h)
                        assert y.on_device and _lib.TRANSFERS["d2h"] == d2h and (y.noise is NULL) == (z is None)
                        pk = max(float(np.max(np.abs(want_s))), 0.0 if z is None else float(np.max(np.abs(want_n))))
                        tag = f"filter n={n} taps={taps} h{'c' if ch else 'r'} x{'c' if cx else 'r'}{' noise' if noise else ''}"
                        ok &= peak(y.signal, want_s, tag + " signal", pk=pk)
                        if z is not None:
                            ok &= peak(y.noise, want_n, tag + " noise", pk=pk)
    assert kept >= 100                  # (of 120 inputs: SciPy's own accuracy must not empty the test)
    lo, hi = _lib.supported_log2n(_lib.C128, direct=True)
    with pytest.raises(ValueError, match=f"exceed the device path \\(2\\^{hi} points\\)"):
        E(np.ones(1 << hi)).filter(np.ones(3))
    assert ok


def test_chain_on_a_pd_output_without_host_transfers():
    from opticomlib_amd import PD, optical_signal
    gv(sps=16, R=10e9)
    rng = np.random.default_rng(3)
    field = (rng.standard_normal(1 << 14) + 1j * rng.standard_normal(1 << 14)) * 0.03
    x = PD(optical_signal(field), BW=5e9, r=1.0, rng="device")
    assert x.on_device
    h = np.hanning(33) / np.hanning(33).sum()
    ref = electrical_signal(x._raw("signal").to_host(), NULL if x._raw("noise") is NULL else x._raw("noise").to_host())

    def chain(s):
        y = (s - s.power() ** 0.5) * 3.5          # 1, 2 (power reads one scalar inside the library)
        y = y + y.abs("signal")                   # 3, 4
        y = (-y)[10:-10:2]                        # 5, 6
        y = y.filter(h) / 2.0                     # 7, 8
        y = y ** 2 - 1e-6                         # 9, 10
        return y, y > 0.0

    before = dict(_lib.TRANSFERS)
    y, bits = chain(x)
    assert _lib.TRANSFERS["d2h"] == before["d2h"] and y.on_device and hasattr(bits._raw(), "ptr")
    assert _lib.TRANSFERS["h2d"] - before["h2d"] == 1          # the taps
    wy, wbits = chain(ref)
    pk = max(float(np.max(np.abs(wy.signal))), float(np.max(np.abs(wy.noise))) if wy.noise is not NULL else 0.0)
    assert peak(y.signal, wy.signal, "chain signal", pk=pk)
    if wy.noise is not NULL:
        assert peak(y.noise, wy.noise, "chain noise", pk=pk)
    # equal bits wherever the host's sample (signal + noise) lies further from the threshold than the value bound allows the device's to move
    clear = np.abs(np.asarray(wy.signal + wy.noise)) > 2e-12 * pk
    assert clear.mean() > 0.99 and np.array_equal(bits.data[clear], wbits.data[clear])


def test_two_gpus_are_a_value_error():
    if _lib.device_count() < 2:
        x = E(np.ones(8))
        fake = electrical_signal.from_device(_lib.DeviceArray((8,), np.float64, 0))
        fake._raw("signal").device = 1               # (one GPU here: the check reads the arrays' device numbers before anything is launched)
        try:
            with pytest.raises(ValueError, match="different GPUs"):
                x + fake
        finally:
            fake._raw("signal").device = 0
        return
    a = E(np.ones(8))
    b = electrical_signal.from_device(_lib.DeviceArray.from_host(np.ones(8), None, 1))
    with pytest.raises(ValueError, match="different GPUs"):
        a * b


def test_the_device_is_the_one_the_signal_lies_on():
    """The ssfm_signal_* entry points take no device number: host memory is refused before any launch, with the pointer named."""
    lib = _lib.load()
    host = np.ones(64)
    out = _lib.DeviceArray((64,), np.float64)
    assert lib.ssfm_signal_unary(0, 1, 64, _lib._ptr(host), None, 0, 0.0, 0.0, 0, out, None) == 1
    assert b"is not device memory" in lib.ssfm_last_error()
    assert lib.ssfm_signal_split(_lib._ptr(host), 32, out, None) == 1
    x = E(np.arange(64.0))
    assert lib.ssfm_signal_binary(0, 1, 64, x._raw("signal"), None, 64, 0, _lib._ptr(host), None, 64, 0, 0.0, 0.0, out, None) == 1
    assert b"different devices" in lib.ssfm_last_error()
    assert same((-x).signal, -np.arange(64.0))              # the library goes on working after a refusal


def test_an_operand_of_another_class_stays_on_the_device():
    """A device-resident signal of the base class (or of a sibling class) is used where it lies: nothing is read, it stays on the device, and
    the result has the class of the left operand."""
    class mine(electrical_signal):
        pass

    class other(electrical_signal):
        pass
    a = mine.from_device(_lib.DeviceArray.from_host(np.arange(8.0)), _lib.DeviceArray.from_host(np.ones(8)))
    for b in (E(np.arange(8.0) * 2, np.ones(8) * 3), other.from_device(_lib.DeviceArray.from_host(np.arange(8.0) * 2))):
        before = dict(_lib.TRANSFERS)
        res = [a + b, a - b, a * b, b * a, a > b]
        assert _lib.TRANSFERS == before and a.on_device and b.on_device
        assert [type(r) for r in res[:4]] == [mine, mine, mine, type(b)] and all(r.on_device for r in res[:4])
        assert same((a * b).signal, np.arange(8.0) * (np.arange(8.0) * 2))
    for r in (a + 1, 2 * a, a[1:], -a, a / 2, a ** 2, a ** 3, a.conj(), a.real, a.abs("signal"), a.normalize(), a.filter([1.0]), np.arange(8.0) * a, a.phase()):
        assert type(r) is mine and r.on_device


def test_the_example_prints_zero_device_to_host_copies():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "signal_algebra.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "device-to-host copies between PD and the bits: 0; result on the GPU: True" in out.stdout


@pytest.mark.parametrize("cplx", (False, True), ids=("float64", "complex128"))
@pytest.mark.parametrize("n", (1, 2, 513, 524291))
def test_the_signal_and_field_entry_points_share_their_kernels(n, cplx):
    """ssfm_signal_reduce / ssfm_signal_slice are ssfm_field_reduce / ssfm_field_slice of one row: the same kernels on the same grid, so the
    same bits.  524291 is odd and just past 1024 workgroups x 256 lanes x 2 values, where the reduction's grid stops growing.  The values
    against NumPy on the host copy: slices exactly, sum and power within 1e-12 of the peak, max |.| exactly for float64 and within the
    hypot bound for complex128 (module docstring)."""
    import ctypes
    rng = np.random.default_rng(n)
    dtype, code = (np.complex128, 1) if cplx else (np.float64, 2)            # the field entry points' code of the type (ssfm_amd.h)
    ok = True
    for noise in (False, True):
        s, z = operands(n, rng, cplx, noise)
        total = s if z is None else s + z
        ds, dz = _lib.DeviceArray.from_host(s), (None if z is None else _lib.DeviceArray.from_host(z))
        tag = f"shared n={n} {'c' if cplx else 'r'}{' noise' if noise else ''}"
        for kind, name in ((2, "sum"), (1, "maxabs")) + (((0, "power"),) if noise else ()):      # (a lone array's power goes another way)
            a, b = (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
            _lib.api.ssfm_signal_reduce(kind, 1, n, ds, dz, int(cplx), a)
            _lib.api.ssfm_field_reduce(kind, 1, n, ds, dz, int(cplx), b)
            k = 2 if name == "sum" else 1
            assert same(np.array(a[:k]), np.array(b[:k])), (tag, name)
            if name == "sum":
                got = np.complex128(complex(a[0], a[1])) if cplx else np.float64(a[0])
                ok &= peak(got, np.sum(total), f"{tag} sum", pk=float(np.sum(np.abs(total))))
            elif name == "power":
                ok &= peak(np.float64(a[0]), np.mean(np.abs(total) ** 2), f"{tag} power")
            elif cplx:
                ok &= ulps(np.float64(a[0]), np.max(np.abs(total)), f"{tag} max", ULP["hypot"])
            else:
                assert a[0] == np.max(np.abs(total)), (tag, name)
        for key in (slice(n // 3, None, 1), slice(None, None, 3), slice(None, None, -2), slice(n - 1, n), slice(None)):
            start, stop, step = key.indices(n)
            count = len(range(start, stop, step))
            room = lambda: (_lib.zeros_device((count,), dtype), _lib.zeros_device((count,), dtype) if noise else None)     # noqa: E731
            by_signal, by_field = room(), room()
            _lib.api.ssfm_signal_slice(1, n, ds, dz, int(cplx), start, step, count, *by_signal)
            _lib.api.ssfm_field_slice(code, 1, n, ds, dz, 0, 1, start, step, count, *by_field)
            for src, o_sig, o_fld in zip((s, z), by_signal, by_field):
                if src is not None:
                    g_sig, g_fld = o_sig.to_host(), o_fld.to_host()
                    assert np.array_equal(g_sig, g_fld) and same(g_sig, src[key]), (tag, key)
    assert ok
