"""The cases of the electrical_signal algebra, shared by the fixture generator (tests/golden/make_golden_signal.py, which runs them on the
reference's class) and by the tests (which run them on this package's class, on the host and with the operands uploaded).

A case is ``(id, function of the namespace)``; the namespace maps names to signals (``xr``: real, ``xrn``: real with noise, ``xc``, ``xcn``:
complex; ``y*``: a second set; ``one``: size 1 with noise; ``mis``: another size), host arrays (``ar``, ``ac``, ``a1``) and NumPy.
``outcome`` turns what a case returns, or raises, into arrays a ``.npz`` can hold.  Test infrastructure."""
import warnings

import numpy as np

N = 257                      # odd: the kernels' last-sample path runs in every case
SIGNALS = ("xr", "xrn", "xc", "xcn")
GROUPS = ("binary", "reflected", "scalar", "pow", "compare", "slice", "methods", "filter", "protocol")


def inputs():
    """name -> (signal, noise or None): seeded, positive and negative values, noise within a factor 10^3 of the signal."""
    rng = np.random.default_rng(1216)
    r = lambda n, s=1.0: rng.standard_normal(n) * s                                    # noqa: E731
    c = lambda n, s=1.0: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * s     # noqa: E731
    return {
        "xr": (r(N), None), "xrn": (r(N), r(N, 0.05)), "xc": (c(N), None), "xcn": (c(N), c(N, 0.05)),
        "yr": (r(N) + 0.5, None), "yrn": (r(N), r(N, 0.02)), "yc": (c(N), None), "ycn": (c(N), c(N, 0.02)),
        "one": (np.array([1.5]), np.array([0.25])), "mis": (r(100), None),
    }


def arrays():
    rng = np.random.default_rng(1780)
    return {"ar": rng.standard_normal(N), "ac": rng.standard_normal(N) + 1j * rng.standard_normal(N), "a1": np.array([2.0]),
            "h1": np.array([0.7]), "h2": np.array([0.5, -0.25]), "h8": rng.standard_normal(8), "h9": rng.standard_normal(9),
            "h300": rng.standard_normal(300) / 17, "hc": rng.standard_normal(9) + 1j * rng.standard_normal(9)}


def cases():
    out = []
    add = lambda group, name, fn: out.append((f"{group}/{name}", fn))                  # noqa: E731
    others = ("yr", "yrn", "yc", "ycn", "one", "mis", "ar", "ac", "a1")
    for a in SIGNALS:
        for b in others:
            add("binary", f"{a}+{b}", lambda v, a=a, b=b: v[a] + v[b])
            add("binary", f"{a}-{b}", lambda v, a=a, b=b: v[a] - v[b])
            add("binary", f"{a}*{b}", lambda v, a=a, b=b: v[a] * v[b])
        for name, k in (("2", 2), ("2.5", 2.5), ("3+2j", 3 + 2j), ("-0.0", -0.0)):
            add("binary", f"{a}+{name}", lambda v, a=a, k=k: v[a] + k)
            add("binary", f"{a}-{name}", lambda v, a=a, k=k: v[a] - k)
            add("binary", f"{a}*{name}", lambda v, a=a, k=k: v[a] * k)
            add("reflected", f"{name}+{a}", lambda v, a=a, k=k: k + v[a])
            add("reflected", f"{name}-{a}", lambda v, a=a, k=k: k - v[a])
            add("reflected", f"{name}*{a}", lambda v, a=a, k=k: k * v[a])
        for b in ("ar", "ac", "a1"):
            add("reflected", f"{b}+{a}", lambda v, a=a, b=b: v[b] + v[a])
            add("reflected", f"{b}-{a}", lambda v, a=a, b=b: v[b] - v[a])
            add("reflected", f"{b}*{a}", lambda v, a=a, b=b: v[b] * v[a])
        add("binary", f"one*{a}", lambda v, a=a: v["one"] * v[a])
        add("binary", f"one+{a}", lambda v, a=a: v["one"] + v[a])
        add("scalar", f"-{a}", lambda v, a=a: -v[a])
        for name, k in (("2", 2), ("2.5", 2.5), ("1+1j", 1 + 1j), ("0", 0), ("0.0", 0.0), ("str", "a"), ("f64", np.float64(3.0)), ("list", [2.0])):
            add("scalar", f"{a}/{name}", lambda v, a=a, k=k: v[a] / k)
        for name, k in (("2", 2), ("0.3", 0.3), ("1j", 1j), ("0", 0)):
            add("scalar", f"{a}//{name}", lambda v, a=a, k=k: v[a] // k)
        for name, k in (("0", 0), ("1", 1), ("2", 2), ("2.0", 2.0), ("0.5", 0.5), ("-1", -1), ("3", 3), ("1j", 1j), ("str", "2")):
            add("pow", f"{a}**{name}", lambda v, a=a, k=k: v[a] ** k)
        for b in ("yr", "yrn", "yc", "mis", "ar"):
            add("compare", f"{a}>{b}", lambda v, a=a, b=b: v[a] > v[b])
            add("compare", f"{a}<{b}", lambda v, a=a, b=b: v[a] < v[b])
            add("compare", f"{a}=={b}", lambda v, a=a, b=b: v[a] == v[b])
        add("compare", f"{a}>0.1", lambda v, a=a: v[a] > 0.1)
        add("compare", f"{a}<0.1", lambda v, a=a: v[a] < 0.1)
        add("compare", f"{a}==self", lambda v, a=a: v[a] == v[a])
        keys = {"all": slice(None), "head": slice(None, 100), "step3": slice(10, 200, 3), "rev": slice(None, None, -1), "rev2": slice(None, None, -2),
                "back": slice(250, 5, -2), "tail": slice(-10, None), "empty": slice(5, 5), "beyond": slice(300, None), "empty_rev": slice(5, 50, -1),
                "int3": 3, "int-1": -1, "int1000": 1000, "str": "a", "float": 2.5, "tuple": (1, 2)}
        for name, k in keys.items():
            add("slice", f"{a}[{name}]", lambda v, a=a, k=k: v[a][k])
        add("methods", f"{a}.conj", lambda v, a=a: v[a].conj())
        add("methods", f"{a}.real", lambda v, a=a: v[a].real)
        add("methods", f"{a}.imag", lambda v, a=a: v[a].imag)
        add("methods", f"{a}.sum", lambda v, a=a: v[a].sum())
        for of in ("signal", "noise", "all", "ALL", "bad"):
            add("methods", f"{a}.abs({of})", lambda v, a=a, of=of: v[a].abs(of))
            add("methods", f"{a}.power(W,{of})", lambda v, a=a, of=of: v[a].power("W", of))
            add("methods", f"{a}.power(dBm,{of})", lambda v, a=a, of=of: v[a].power("dBm", of))
        add("methods", f"{a}.abs(3)", lambda v, a=a: v[a].abs(3))
        add("methods", f"{a}.power()", lambda v, a=a: v[a].power())
        add("methods", f"{a}.power(V)", lambda v, a=a: v[a].power("V"))
        for by in ("power", "amplitude", "bad"):
            add("methods", f"{a}.normalize({by})", lambda v, a=a, by=by: v[a].normalize(by))
        add("methods", f"{a}.phase", lambda v, a=a: v[a].phase())
        for h in ("h1", "h2", "h8", "h9", "h300", "hc"):
            add("filter", f"{a}.filter({h})", lambda v, a=a, h=h: v[a].filter(v[h]))
        add("protocol", f"{a}.w", lambda v, a=a: v[a].w())
        add("protocol", f"{a}.w(shift)", lambda v, a=a: v[a].w(True))
        add("protocol", f"{a}.f", lambda v, a=a: v[a].f())
        add("protocol", f"{a}.t", lambda v, a=a: v[a].t)
        add("protocol", f"{a}.grid", lambda v, a=a: np.array([v[a].fs, v[a].sps, v[a].dt, v[a].size, len(v[a])]))
        add("protocol", f"{a}.shape", lambda v, a=a: np.array(v[a].shape))
        add("protocol", f"{a}.type", lambda v, a=a: np.array(v[a].type.__name__))
        add("protocol", f"{a}.iter", lambda v, a=a: np.array(list(iter(v[a]))))
        add("protocol", f"asarray({a})", lambda v, a=a: np.asarray(v[a]))
        add("protocol", f"asarray({a},c128)", lambda v, a=a: np.asarray(v[a], dtype=np.complex128))
        add("protocol", f"np.abs({a})", lambda v, a=a: np.abs(v[a]))
        add("protocol", f"np.exp({a})", lambda v, a=a: np.exp(v[a]))
        add("protocol", f"np.add(ar,{a})", lambda v, a=a: np.add(v["ar"], v[a]))
        add("protocol", f"np.maximum({a},ar)", lambda v, a=a: np.maximum(v[a].real, v["ar"]))
    return out


def namespace(cls, upload=None):
    """The cases' namespace with signals of class ``cls``; ``upload(signal object) -> signal object`` moves each one (to a GPU)."""
    v = dict(arrays())
    for name, (s, n) in inputs().items():
        x = cls(s) if n is None else cls(s, n)
        v[name] = upload(x) if upload else x
    return v


def outcome(fn, v, null):
    """What a case gives, as a dict of arrays (``describe``)."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            r = fn(v)
        except Exception as e:                  # noqa: BLE001  (the exception IS the recorded outcome)
            r = e
    return describe(r, null)


def describe(r, null):
    """A case's result, or the exception it raised, as a dict of arrays: kind 'signal' (class name, signal, noise when there is one), 'bits',
    'array', or 'error' (type name and text)."""
    if isinstance(r, Exception):
        return {"kind": np.array("error"), "type": np.array(type(r).__name__), "text": np.array(str(r))}
    name = type(r).__name__
    if name in ("electrical_signal", "optical_signal"):
        out = {"kind": np.array("signal"), "cls": np.array(name), "signal": np.asarray(r.signal)}
        if r.noise is not null:
            out["noise"] = np.asarray(r.noise)
        return out
    if name == "binary_sequence":
        return {"kind": np.array("bits"), "data": np.asarray(r.data)}
    return {"kind": np.array("array"), "value": np.asarray(r)}
