"""The electrical_signal algebra without a GPU: the host path against every fixture recorded from the reference (values equal -- it is the same
NumPy --, result class, noise present or NULL, exception type and text), the new entry points of the C ABI (which take no device number: the signal's memory names it), and that a host-only signal never
loads a device."""
import os
import subprocess

import numpy as np
import pytest

import signal_cases as sc
from opticomlib_amd import NULL, _lib, binary_sequence, electrical_signal, gv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("ssfm_signal_binary", "ssfm_signal_unary", "ssfm_signal_slice", "ssfm_signal_reduce", "ssfm_signal_phase", "ssfm_signal_pack",
               "ssfm_signal_split")
N_CASES = {"binary": 164, "reflected": 84, "scalar": 52, "pow": 36, "compare": 72, "slice": 64, "methods": 104, "filter": 24, "protocol": 56}
CASES = sc.cases()


def load_group(group):
    with np.load(os.path.join(GOLDEN, f"signal_{group}.npz")) as z:
        return {k: z[k] for k in z.files}


def load_namespace(upload=None):
    """The operands as the fixture holds them (not regenerated)."""
    with np.load(os.path.join(GOLDEN, "signal_inputs.npz")) as z:
        v = {k: z[k] for k in z.files if "/" not in k and k != "versions"}
        for name in {k.split("/")[0] for k in z.files if "/" in k}:
            x = electrical_signal(z[name + "/signal"], z[name + "/noise"] if name + "/noise" in z.files else NULL)
            v[name] = upload(x) if upload else x
    return v


def expected(fix, name):
    return {k.split("|", 1)[1]: a for k, a in fix.items() if k.split("|", 1)[0] == name}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


def test_there_are_fixtures():
    assert sum(N_CASES.values()) == len(CASES) == 656
    for g, count in N_CASES.items():
        assert len({k.split("|")[0] for k in load_group(g) if k != "versions"}) == count, g
    kinds = [str(a) for g in N_CASES for k, a in load_group(g).items() if k.endswith("|kind")]
    assert {k: kinds.count(k) for k in set(kinds)} == {"signal": 398, "error": 118, "bits": 40, "array": 100}


def test_the_fixture_inputs_are_the_cases_inputs():
    v, w = load_namespace(), sc.namespace(electrical_signal)
    assert v.keys() == w.keys()
    for k in v:
        if isinstance(v[k], electrical_signal):
            assert same(v[k].signal, w[k].signal) and (v[k].noise is NULL) == (w[k].noise is NULL)
            assert v[k].noise is NULL or same(v[k].noise, w[k].noise)
        else:
            assert same(v[k], w[k])


@pytest.mark.parametrize("group", sc.GROUPS)
def test_host_path_matches_the_reference(group):
    gv.default()
    fix, v = load_group(group), load_namespace()
    before = dict(_lib.TRANSFERS)
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        want, got = expected(fix, name), sc.outcome(fn, v, NULL)
        if want.keys() != got.keys() or any(not same(want[k], got[k]) for k in want):
            bad.append((cid, {k: (str(a) if a.ndim == 0 else a.dtype) for k, a in want.items()}, {k: (str(a) if a.ndim == 0 else a.dtype) for k, a in got.items()}))
    assert not bad, bad[:10]
    assert _lib.TRANSFERS == before                 # a host-only signal never loads a device
    assert all(not x.on_device for x in v.values() if isinstance(x, electrical_signal))


def test_the_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and f"SSFM_API int {s}(int device" not in hdr and s in _lib.SYMBOLS and s in names, s
    assert {n for n in names if n.startswith("ssfm_signal_")} == set(NEW_SYMBOLS)
    assert "#define SSFM_ABI_VERSION 3" in hdr
    assert "typing.py:1308-1419 (electrical_signal's" in hdr
    mk = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()
    assert "signal_ops.hip" in mk and "signal_ops.o: FLAGS += -ffp-contract=off" in mk


def test_results_keep_the_class_and_signals_are_unhashable():
    class mine(electrical_signal):
        pass
    x = mine(np.arange(4.0), np.ones(4))
    for r in (x + 1, 2 * x, x - x, x[1:], -x, x / 2, x // 2, x ** 2, x ** 3, x.conj(), x.real, x.abs("signal"), x.normalize(), x.filter([1.0]), np.arange(4.0) * x):
        assert type(r) is mine
    assert x.type is mine and isinstance(x > 1, binary_sequence)
    with pytest.raises(TypeError, match="unhashable"):
        hash(x)


def test_lt_is_the_references_subtraction():
    """`a < b` is `b - a > 0` (typing.py:1387-1389): with a NaN on either side both orders are False."""
    a, b = electrical_signal([1.0, np.nan, 3.0]), electrical_signal([2.0, 2.0, np.nan])
    assert list((a < b).data) == [1, 0, 0] and list((a > b).data) == [0, 0, 0]


PUBLIC = ["abs", "conj", "dt", "f", "filter", "from_device", "fs", "imag", "ndim", "noise", "normalize", "on_device", "phase", "power", "psd", "real",
          "shape", "signal", "size", "sps", "sum", "t", "to_numpy", "type", "w"]
DUNDERS = {"__add__", "__array__", "__array_ufunc__", "__call__", "__eq__", "__floordiv__", "__getitem__", "__gt__", "__hash__", "__init__", "__iter__",
           "__len__", "__lt__", "__mul__", "__neg__", "__pow__", "__radd__", "__repr__", "__rmul__", "__rsub__", "__sub__", "__truediv__"}
SHARED = ("signal", "noise", "_raw", "on_device", "shape", "ndim", "size", "type", "fs", "sps", "dt", "t", "__len__", "__hash__", "__iter__", "__array__",
          "to_numpy", "w", "f", "__call__", "psd", "_device_arrays", "__add__", "__radd__", "__sub__", "__rsub__", "__rmul__", "__eq__", "__neg__", "conj",
          "real", "imag", "sum", "filter", "__truediv__", "__floordiv__", "__pow__", "__array_ufunc__")


def test_the_two_signal_classes_share_one_base_and_keep_their_surface():
    """electrical_signal and optical_signal are siblings under one private base: neither is the other's subclass, the public names and the
    protocols of each are the lists below (written down from the classes as they were while they were unrelated), and every member the base
    holds is one object for both, so that an edit cannot fork them again."""
    from opticomlib_amd import optical_signal
    assert not issubclass(optical_signal, electrical_signal) and not issubclass(electrical_signal, optical_signal)
    public = lambda cls: sorted(n for n in dir(cls) if not n.startswith("_"))                            # noqa: E731
    assert public(optical_signal) == PUBLIC                                              # (`n_pol` and `execution_time` are instance attributes)
    assert public(electrical_signal) == sorted(PUBLIC + ["MAX_EYE_TRACES", "plot_eye"])
    x = optical_signal(np.arange(4.0))
    assert sorted(vars(x)) == ["_noise", "_signal", "execution_time", "n_pol"] and not hasattr(electrical_signal(np.arange(4.0)), "n_pol")
    housekeeping = {"__dict__", "__doc__", "__module__", "__weakref__", "__firstlineno__", "__static_attributes__"}
    for cls in (electrical_signal, optical_signal):
        own = {n for n in dir(cls) if n.startswith("__") and n.endswith("__") and any(n in k.__dict__ for k in cls.__mro__[:-1])}
        assert own - housekeeping == DUNDERS, cls
        assert cls.__hash__ is None
    for m in SHARED:
        assert getattr(electrical_signal, m) is getattr(optical_signal, m), m
    assert "_signal_base" not in dir(__import__("opticomlib_amd"))
