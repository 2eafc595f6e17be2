"""The optical_signal algebra without a GPU: the host path against every fixture recorded from the reference (values equal -- it is the same
NumPy --, result class, n_pol and shape, dtype, noise present or NULL, exception type and text), the new entry points of the C ABI, and that
host-only operands never load a device."""
import os
import subprocess

import numpy as np
import pytest

import optical_cases as oc
from opticomlib_amd import NULL, _lib, electrical_signal, gv, optical_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("ssfm_field_binary", "ssfm_field_unary", "ssfm_field_slice", "ssfm_field_reduce")
N_CASES = {"binary_x1n": 54, "binary_x2": 54, "binary_x2n": 54, "binary_s2n": 54, "binary_s1": 54, "binary_r2n": 54, "reflected": 63, "scalar": 84,
           "pow": 54, "compare": 66, "index": 216, "methods": 110, "filter": 24, "protocol": 90}
CASES = oc.cases()


def load_group(group):
    with np.load(os.path.join(GOLDEN, f"optical_{group}.npz")) as z:
        return {k: z[k] for k in z.files}


def load_namespace(upload=None):
    """The operands as the fixture holds them (not regenerated)."""
    with np.load(os.path.join(GOLDEN, "optical_inputs.npz")) as z:
        v = {k: z[k] for k in z.files if "/" not in k and k != "versions"}
        for name in {k.split("/")[0] for k in z.files if "/" in k}:
            cls = electrical_signal if name.startswith("el:") else optical_signal
            x = cls(z[name + "/signal"], z[name + "/noise"] if name + "/noise" in z.files else NULL)
            v[name.split(":")[-1]] = upload(x) if upload else x
    return v


def expected(fix, name):
    return {k.split("|", 1)[1]: a for k, a in fix.items() if k.split("|", 1)[0] == name}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


def test_there_are_fixtures():
    assert tuple(N_CASES) == oc.GROUPS and sum(N_CASES.values()) == len(CASES) == 1031
    for g, count in N_CASES.items():
        assert len({k.split("|")[0] for k in load_group(g) if k != "versions"}) == count, g
        assert os.path.getsize(os.path.join(GOLDEN, f"optical_{g}.npz")) < (1 << 20), g
    kinds = [str(a) for g in N_CASES for k, a in load_group(g).items() if k.endswith("|kind")]
    assert {k: kinds.count(k) for k in set(kinds)} == {"signal": 627, "error": 235, "array": 169}


def test_the_fixture_inputs_are_the_cases_inputs():
    v, w = load_namespace(), oc.namespace(optical_signal, electrical_signal)
    assert v.keys() == w.keys()
    for k in v:
        if isinstance(v[k], (optical_signal, electrical_signal)):
            assert type(v[k]) is type(w[k]) and same(v[k].signal, w[k].signal) and (v[k].noise is NULL) == (w[k].noise is NULL)
            assert v[k].noise is NULL or same(v[k].noise, w[k].noise)
        else:
            assert same(v[k], w[k])


@pytest.mark.parametrize("group", oc.GROUPS)
def test_host_path_matches_the_reference(group):
    gv.default()
    fix, v = load_group(group), load_namespace()
    before = dict(_lib.TRANSFERS)
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        want, got = expected(fix, name), oc.outcome(fn, v, NULL)
        if want.keys() != got.keys() or any(not same(want[k], got[k]) for k in want):
            bad.append((cid, {k: (str(a) if a.ndim == 0 else (a.dtype, a.shape)) for k, a in want.items()},
                        {k: (str(a) if a.ndim == 0 else (a.dtype, a.shape)) for k, a in got.items()}))
    assert not bad, (len(bad), bad[:10])
    assert _lib.TRANSFERS == before                 # host-only operands never load a device
    assert all(not x.on_device for x in v.values() if isinstance(x, (optical_signal, electrical_signal)))


def test_n_pol_follows_the_shape_of_the_result():
    v = load_namespace()
    assert (v["x1n"] + v["y2n"]).n_pol == 2 and (v["x1n"] * v["col"]).shape == (2, oc.N) and (v["x2n"] * v["el"]).n_pol == 2
    assert v["x2n"][1].n_pol == 1 and v["x2n"][:, 5:9].n_pol == 2 and v["x2n"][0, 5:9].shape == (4,) and v["x2n"][:, 3].shape == (2,)
    assert isinstance(v["x2"][0, 0:1], optical_signal) and (v["one"] * v["col"]).shape == (2, 1)


def test_the_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and f"SSFM_API int {s}(int device" not in hdr and s in _lib.SYMBOLS and s in names, s
    assert "#define SSFM_ABI_VERSION 3" in hdr
    assert "typing.py:1308-1419" in hdr and ":2261-2305" in hdr


def test_fields_are_unhashable_and_ordering_is_not_implemented():
    x = optical_signal(np.arange(4.0) + 0j)
    with pytest.raises(TypeError, match="unhashable"):
        hash(x)
    with pytest.raises(NotImplementedError, match="The > operator is not implemented for optical_signal objects."):
        x > 1
    with pytest.raises(NotImplementedError, match="The < operator is not implemented for optical_signal objects."):
        x < x
