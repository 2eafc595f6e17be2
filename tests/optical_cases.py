"""The cases of the optical_signal algebra, shared by the fixture generator (tests/golden/make_golden_optical.py, which runs them on the
reference's class) and by the tests (which run them on this package's class, on the host and with the operands uploaded).

A case is ``(id, function of the namespace)``; the namespace maps names to fields (``x*`` / ``y*``: complex128, ``s*`` / ``t*``: complex64,
``r*``: real; ``1`` / ``2``: the polarisations; ``n``: with noise; ``col``: a ``(2, 1)`` value; ``one``: a ``(1,)`` value with noise; ``mis``:
another size), electrical signals (``el``, ``eln``), host arrays (``ac``, ``a2r``, ``a21``, ``af``, the taps ``h*``) and NumPy.  The binary
cases are one group per left operand, so that no fixture file passes the size limit of a committed file.

Left out on purpose: ``.abs(...)`` and ``.phase()`` (this package returns host arrays there, the reference signal objects; ``np.abs(x)``
is in), and ``normalize('power')`` of a two-polarisation field (the reference fails there with a ``TypeError`` whose text names its own
module).  ``power`` goes through ``np.asarray``: the reference wraps the two powers of a two-polarisation field in a signal object, this
package returns the ``(2,)`` array.  Test infrastructure."""
import numpy as np

from signal_cases import describe, outcome  # noqa: F401  (the same recording of results and exceptions)

N = 257                      # odd: row 1 of a (2, N) field starts off a 16-byte boundary in float64 and complex64
SIGNALS = ("x1n", "x2", "x2n", "s2n", "s1", "r2n")
OTHERS = ("y1n", "y2n", "t2n", "t1", "col", "one", "el", "eln", "mis", "ac", "a2r", "af")
SCALARS = {"2": 2, "2.5": 2.5, "3+2j": 3 + 2j, "f64": np.float64(1.5), "f32": np.float32(0.5), "-0.0": -0.0}
OPS = {"+": lambda a, b: a + b, "-": lambda a, b: a - b, "*": lambda a, b: a * b}
GROUPS = tuple(f"binary_{a}" for a in SIGNALS) + ("reflected", "scalar", "pow", "compare", "index", "methods", "filter", "protocol")
KEYS = {"all": slice(None), "head": slice(None, 100), "step3": slice(10, 200, 3), "rev": slice(None, None, -1), "rev2": slice(None, None, -2),
        "back": slice(250, 5, -2), "tail": slice(-10, None), "first": slice(0, 1), "last": slice(N - 1, None), "empty": slice(5, 5),
        "beyond": slice(300, None), "int0": 0, "int1": 1, "int-1": -1, "int2": 2, "int256": N - 1, "int1000": 1000,
        "0,10:20": (0, slice(10, 20)), "1,::-3": (1, slice(None, None, -3)), "-1,:": (-1, slice(None)), "0,5:5": (0, slice(5, 5)),
        "-1,5": (-1, 5), "0,0": (0, 0), "1,1": (1, 1), "1,256": (1, N - 1), ":,5:50:2": (slice(None), slice(5, 50, 2)),
        ":,::-1": (slice(None), slice(None, None, -1)), ":,3": (slice(None), 3), ":,0": (slice(None), 0), ":,-1": (slice(None), -1),
        "2,5": (2, 5), "0,1000": (0, 1000), "0,1,2": (0, 1, 2), "str": "a", "float": 2.5, "0,str": (0, "a")}


def inputs():
    """name -> (signal, noise or None): seeded, positive and negative values, noise within a factor 10^3 of the signal."""
    rng = np.random.default_rng(2103)
    c = lambda shape, s=1.0: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * s        # noqa: E731
    f = lambda shape, s=1.0: c(shape, s).astype(np.complex64)                                           # noqa: E731
    r = lambda shape, s=1.0: rng.standard_normal(shape) * s                                             # noqa: E731
    return {
        "x1n": (c(N), c(N, 0.05)), "x2": (c((2, N)), None), "x2n": (c((2, N)), c((2, N), 0.05)), "s2n": (f((2, N)), f((2, N), 0.05)),
        "s1": (f(N), None), "r2n": (r((2, N)), r((2, N), 0.05)),
        "y1n": (c(N), c(N, 0.02)), "y2n": (c((2, N)), c((2, N), 0.02)), "t2n": (f((2, N)), f((2, N), 0.02)), "t1": (f(N), None),
        "col": (np.array([[1.5 + 0j], [-0.5 + 2j]]), None), "one": (np.array([1.5]), np.array([0.25])), "mis": (c(100), None),
    }


def electrical():
    rng = np.random.default_rng(1022)
    return {"el": (rng.standard_normal(N), None), "eln": (rng.standard_normal(N) + 1j * rng.standard_normal(N), rng.standard_normal(N) * 0.03 + 0j)}


def arrays():
    rng = np.random.default_rng(2305)
    return {"ac": rng.standard_normal(N) + 1j * rng.standard_normal(N), "a2r": rng.standard_normal((2, N)), "a21": np.array([[2.0], [-0.5]]),
            "af": rng.standard_normal(N).astype(np.float32), "a1": np.array([2.0]),
            "h1": np.array([0.7]), "h9": rng.standard_normal(9), "hc": rng.standard_normal(9) + 1j * rng.standard_normal(9),
            "hf": rng.standard_normal(8).astype(np.float32)}


def cases():
    out = []
    add = lambda group, name, fn: out.append((f"{group}/{name}", fn))                  # noqa: E731
    for a in SIGNALS:
        for sym, op in OPS.items():
            for b in OTHERS:
                add(f"binary_{a}", f"{a}{sym}{b}", lambda v, a=a, b=b, op=op: op(v[a], v[b]))
            for name, k in SCALARS.items():
                add(f"binary_{a}", f"{a}{sym}{name}", lambda v, a=a, k=k, op=op: op(v[a], k))
        add("scalar", f"-{a}", lambda v, a=a: -v[a])
        for name, k in (("2", 2), ("2.5", 2.5), ("1+1j", 1 + 1j), ("0", 0), ("0.0", 0.0), ("str", "a"), ("f64", np.float64(3.0)), ("f32", np.float32(3.0)),
                        ("list", [2.0])):
            add("scalar", f"{a}/{name}", lambda v, a=a, k=k: v[a] / k)
        for name, k in (("2", 2), ("0.3", 0.3), ("1j", 1j), ("0", 0)):
            add("scalar", f"{a}//{name}", lambda v, a=a, k=k: v[a] // k)
        for name, k in (("0", 0), ("1", 1), ("2", 2), ("2.0", 2.0), ("0.5", 0.5), ("-1", -1), ("3", 3), ("1j", 1j), ("str", "2")):
            add("pow", f"{a}**{name}", lambda v, a=a, k=k: v[a] ** k)
        for b in ("y1n", "y2n", "t2n", "col", "mis", "ac", "eln"):
            add("compare", f"{a}=={b}", lambda v, a=a, b=b: v[a] == v[b])
        add("compare", f"{a}==self", lambda v, a=a: v[a] == v[a])
        add("compare", f"{a}==0.5", lambda v, a=a: v[a] == 0.5)
        add("compare", f"{a}>y1n", lambda v, a=a: v[a] > v["y1n"])
        add("compare", f"{a}<0.1", lambda v, a=a: v[a] < 0.1)
        for name, k in KEYS.items():
            add("index", f"{a}[{name}]", lambda v, a=a, k=k: v[a][k])
        add("methods", f"{a}.conj", lambda v, a=a: v[a].conj())
        add("methods", f"{a}.real", lambda v, a=a: v[a].real)
        add("methods", f"{a}.imag", lambda v, a=a: v[a].imag)
        add("methods", f"{a}.sum", lambda v, a=a: v[a].sum())
        for of in ("signal", "noise", "all", "ALL", "bad"):
            add("methods", f"{a}.power(W,{of})", lambda v, a=a, of=of: np.asarray(v[a].power("W", of)))
            add("methods", f"{a}.power(dBm,{of})", lambda v, a=a, of=of: np.asarray(v[a].power("dBm", of)))
        add("methods", f"{a}.power()", lambda v, a=a: np.asarray(v[a].power()))
        add("methods", f"{a}.power(V)", lambda v, a=a: np.asarray(v[a].power("V")))
        for by in ("power", "amplitude", "bad"):
            if by != "power" or "2" not in a:
                add("methods", f"{a}.normalize({by})", lambda v, a=a, by=by: v[a].normalize(by))
        for h in ("h1", "h9", "hc", "hf"):
            add("filter", f"{a}.filter({h})", lambda v, a=a, h=h: v[a].filter(v[h]))
        add("protocol", f"{a}.w", lambda v, a=a: v[a].w())
        add("protocol", f"{a}.w(shift)", lambda v, a=a: v[a].w(True))
        add("protocol", f"{a}.f", lambda v, a=a: v[a].f())
        add("protocol", f"{a}.t", lambda v, a=a: v[a].t)
        add("protocol", f"{a}.grid", lambda v, a=a: np.array([v[a].fs, v[a].sps, v[a].dt, v[a].size, len(v[a]), v[a].n_pol, v[a].ndim]))
        add("protocol", f"{a}.shape", lambda v, a=a: np.array(v[a].shape))
        add("protocol", f"{a}.type", lambda v, a=a: np.array(v[a].type.__name__))
        add("protocol", f"{a}.iter", lambda v, a=a: np.array(list(iter(v[a]))))
        add("protocol", f"asarray({a})", lambda v, a=a: np.asarray(v[a]))
        add("protocol", f"asarray({a},c128)", lambda v, a=a: np.asarray(v[a], dtype=np.complex128))
        add("protocol", f"np.abs({a})", lambda v, a=a: np.abs(v[a]))
        add("protocol", f"np.exp({a})", lambda v, a=a: np.exp(v[a]))
        add("protocol", f"np.add(ac,{a})", lambda v, a=a: np.add(v["ac"], v[a]))
        add("protocol", f"np.subtract(a2r,{a})", lambda v, a=a: np.subtract(v["a2r"], v[a]))
        add("protocol", f"np.multiply(af,{a})", lambda v, a=a: np.multiply(v["af"], v[a]))
    for a in ("x1n", "x2n", "s2n"):
        for sym, op in OPS.items():
            for name, k in (("2.5", 2.5), ("3+2j", 3 + 2j), ("f32", np.float32(0.5))):
                add("reflected", f"{name}{sym}{a}", lambda v, a=a, k=k, op=op: op(k, v[a]))
            for b in ("ac", "a2r", "a21", "a1"):
                add("reflected", f"{b}{sym}{a}", lambda v, a=a, b=b, op=op: op(v[b], v[a]))
    return out


def namespace(optical, electrical_cls, upload=None):
    """The cases' namespace with fields of class ``optical`` and signals of class ``electrical_cls``; ``upload(object) -> object`` moves each
    one (to a GPU)."""
    v = dict(arrays())
    for cls, items in ((optical, inputs()), (electrical_cls, electrical())):
        for name, (s, n) in items.items():
            x = cls(s) if n is None else cls(s, n)
            v[name] = upload(x) if upload else x
    return v
