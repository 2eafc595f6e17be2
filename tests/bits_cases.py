"""The cases of the binary_sequence algebra, shared by the fixture generator (tests/golden/make_golden_bits.py, which runs them on the
reference's class) and by the tests (which run them on this package's class, on the host and with the operands uploaded).

A case is ``(id, function of the namespace)``; the namespace maps names to sequences (``a``, ``b``: 257 bits; ``c``: 300; ``one1`` / ``one0``:
one bit; ``mis``: another length; ``w``: a 7-bit word), host operands (``s``: a string; ``l``: a list; ``arr``: an int64 array; ``bad``: an
array holding a 2; ``h33``: 33 filter taps) and ``gv`` (the class's own global variables, ``sps = 8`` for ``dac``).  The strings hold ones
only: under NumPy 2 the reference's ``str2array`` reads every character of a bit string as True (its docstring says ``'101'`` is 1, 0, 1), and
a fixture must not record that; tests/test_bits_cpu.py holds the zeros of a string operand to this package's own constructor.
``outcome`` turns what a case returns, or raises, into arrays a ``.npz`` can hold.  Test infrastructure."""
import warnings

import numpy as np

N = 257                      # odd: a head, 16 vectors and a one-byte tail on the device
GROUPS = ("logic", "concat", "mul", "slice", "count", "dac", "protocol")
HOST_RESULT = ("protocol",)  # the groups whose results are host objects whatever the operands (==, other ufuncs, conversions)
SEQUENCES = ("a", "b", "c", "one1", "one0", "mis", "w")


def inputs():
    """name -> uint8 bits: seeded, both values present."""
    rng = np.random.default_rng(402)
    bits = lambda n: rng.integers(0, 2, n).astype(np.uint8)                            # noqa: E731
    return {"a": bits(N), "b": bits(N), "c": bits(300), "one1": np.array([1], np.uint8), "one0": np.array([0], np.uint8), "mis": bits(100),
            "w": np.array([1, 0, 1, 1, 0, 0, 1], np.uint8)}


def arrays():
    rng = np.random.default_rng(1009)
    arr = rng.integers(0, 2, N)
    bad = arr.copy()
    bad[5] = 2
    return {"s": "1" * N, "l": [int(v) for v in rng.integers(0, 2, N)], "arr": arr, "bad": bad,
            "h33": rng.standard_normal(33)}


def cases():
    out = []
    add = lambda group, name, fn: out.append((f"{group}/{name}", fn))                  # noqa: E731
    ops = {"&": lambda x, y: x & y, "|": lambda x, y: x | y, "^": lambda x, y: x ^ y, "!=": lambda x, y: x != y}
    for sym, op in ops.items():
        for o in ("b", "s", "l", "arr", "one1", "one0", "mis", "bad"):
            add("logic", f"a{sym}{o}", lambda v, op=op, o=o: op(v["a"], v[o]))
        for name, k in (("0", 0), ("1", 1), ("True", True), ("2", 2), ("0.5", 0.5)):
            add("logic", f"a{sym}{name}", lambda v, op=op, k=k: op(v["a"], k))
        add("logic", f"one1{sym}a", lambda v, op=op: op(v["one1"], v["a"]))
        add("logic", f"one0{sym}one1", lambda v, op=op: op(v["one0"], v["one1"]))
        if sym != "!=":                                         # (the reflected forms; `list != a` would be Python's own swap to a.__ne__)
            for o in ("s", "l"):
                add("logic", f"{o}{sym}a", lambda v, op=op, o=o: op(v[o], v["a"]))
            add("logic", f"1{sym}a", lambda v, op=op: op(1, v["a"]))
            add("logic", f"0{sym}a", lambda v, op=op: op(0, v["a"]))
    for x in ("a", "one1", "w"):
        add("logic", f"~{x}", lambda v, x=x: ~v[x])
        add("logic", f"{x}.flip", lambda v, x=x: v[x].flip())
    add("logic", "~~a", lambda v: ~~v["a"])

    for o in ("b", "c", "s", "l", "arr", "one1", "w", "bad"):
        add("concat", f"a+{o}", lambda v, o=o: v["a"] + v[o])
        add("concat", f"{o}+a", lambda v, o=o: v[o] + v["a"])
    for name, k in (("0", 0), ("1", 1), ("2", 2), ("str111", "1 1, 1")):
        add("concat", f"a+{name}", lambda v, k=k: v["a"] + k)
        add("concat", f"{name}+a", lambda v, k=k: k + v["a"])
    add("concat", "w+w+w", lambda v: v["w"] + v["w"] + v["w"])
    add("concat", "frame", lambda v: v["w"] + v["a"] * 3)
    add("concat", "np.add(arr,a)", lambda v: np.add(v["arr"], v["a"]))

    for name, k in (("0", 0), ("1", 1), ("True", True), ("False", False), ("2", 2), ("3", 3), ("16", 16), ("2.0", 2.0), ("-1", -1), ("1.0", 1.0)):
        add("mul", f"a*{name}", lambda v, k=k: v["a"] * k)
        add("mul", f"{name}*a", lambda v, k=k: k * v["a"])
    for o in ("b", "s", "l", "arr", "one1", "one0", "mis", "bad"):
        add("mul", f"a*{o}", lambda v, o=o: v["a"] * v[o])
    for o in ("l", "arr", "s"):
        add("mul", f"{o}*a", lambda v, o=o: v[o] * v["a"])
    add("mul", "w*5", lambda v: v["w"] * 5)
    add("mul", "one1*40", lambda v: v["one1"] * 40)
    add("mul", "np.multiply(arr,a)", lambda v: np.multiply(v["arr"], v["a"]))

    keys = {"all": slice(None), "head": slice(None, 100), "from3": slice(3, None), "from16": slice(16, None), "step3": slice(10, 200, 3),
            "rev": slice(None, None, -1), "rev2": slice(None, None, -2), "back": slice(250, 5, -2), "tail": slice(-10, None), "neg": slice(-5, 2, -2),
            "empty": slice(5, 5), "beyond": slice(300, None), "clipped": slice(-1000, 1000), "empty_rev": slice(5, 50, -1), "int3": 3, "int0": 0,
            "int-1": -1, "int-257": -257, "int257": 257, "int-258": -258}
    for name, k in keys.items():
        add("slice", f"a[{name}]", lambda v, k=k: v["a"][k])
    add("slice", "a[3:][::-1][:7]", lambda v: v["a"][3:][::-1][:7])
    add("slice", "one1[0]", lambda v: v["one1"][0])

    for x in SEQUENCES:
        add("count", f"{x}.ones", lambda v, x=x: v[x].ones)
        add("count", f"{x}.zeros", lambda v, x=x: v[x].zeros)
        add("count", f"{x}.size", lambda v, x=x: v[x].size)
        add("count", f"len({x})", lambda v, x=x: len(v[x]))
    for o in ("b", "a", "s", "l", "arr", "one1", "one0", "mis", "c", "bad"):
        add("count", f"a.hamming({o})", lambda v, o=o: v["a"].hamming_distance(v[o]))
    add("count", "one1.hamming(a)", lambda v: v["one1"].hamming_distance(v["a"]))
    add("count", "one0.hamming(a)", lambda v: v["one0"].hamming_distance(v["a"]))
    add("count", "a.hamming(1)", lambda v: v["a"].hamming_distance(1))
    add("count", "(a!=b).ones", lambda v: (v["a"] != v["b"]).ones)
    add("count", "(~a).ones", lambda v: (~v["a"]).ones)

    for x in ("a", "w", "one1", "c"):
        add("dac", f"{x}.dac(h33)", lambda v, x=x: v[x].dac(v["h33"]))
    add("dac", "(w+a).dac(h33)", lambda v: (v["w"] + v["a"]).dac(v["h33"]))

    add("protocol", "asarray(a)", lambda v: np.asarray(v["a"]))
    add("protocol", "a.to_numpy()", lambda v: v["a"].to_numpy())
    add("protocol", "a.to_numpy(float)", lambda v: v["a"].to_numpy(dtype=np.float64))
    add("protocol", "a.type", lambda v: np.array(v["a"].type.__name__))
    add("protocol", "list(w)", lambda v: np.array(list(v["w"]), dtype=np.int64))
    return out


def namespace(cls, gv, upload=None):
    """The cases' namespace with sequences of class ``cls``; ``upload(sequence) -> sequence`` moves each one (to a GPU)."""
    v = dict(arrays())
    for name, bits in inputs().items():
        x = cls(bits)
        v[name] = upload(x) if upload else x
    gv(sps=8)
    return v


def outcome(fn, v):
    """What a case gives, as a dict of arrays (``describe``)."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            r = fn(v)
        except Exception as e:                  # noqa: BLE001  (the exception IS the recorded outcome)
            r = e
    return describe(r)


def describe(r):
    """A case's result, or the exception it raised, as a dict of arrays: kind 'bits', 'int' (any integer scalar, NumPy's or Python's),
    'signal' (signal + noise of an electrical_signal), 'array', or 'error' (type name and text)."""
    if isinstance(r, Exception):
        return {"kind": np.array("error"), "type": np.array(type(r).__name__), "text": np.array(str(r))}
    name = type(r).__name__
    if name == "binary_sequence":
        return {"kind": np.array("bits"), "data": np.asarray(r.data)}
    if name == "electrical_signal":
        return {"kind": np.array("signal"), "value": np.asarray(r.signal + r.noise)}
    if isinstance(r, (int, np.integer)) and not isinstance(r, (bool, np.bool_)):
        return {"kind": np.array("int"), "value": np.array(int(r), dtype=np.int64)}
    return {"kind": np.array("array"), "value": np.asarray(r)}
