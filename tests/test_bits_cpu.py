"""The binary_sequence algebra without a GPU: the host path against every fixture recorded from the reference (bits and integers equal, ``dac``
to 1e-12 of the peak -- ``filter``'s bound: the same ``fftconvolve`` --, the exception's type, and its text where this class words it), the new
entry points of the C ABI, and that a host-only sequence never loads a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bits_cases as bc
from opticomlib_amd import _lib, binary_sequence, electrical_signal, gv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("ssfm_bits_binary", "ssfm_bits_not", "ssfm_bits_slice", "ssfm_bits_tile", "ssfm_bits_concat", "ssfm_bits_count")
N_CASES = {"logic": 79, "concat": 27, "mul": 34, "slice": 22, "count": 43, "dac": 5, "protocol": 5}
CASES = bc.cases()
# the reference's constructor and this package's word the same refusal differently (this package's words are held by earlier tests)
NOT_BITS = {"The array must contain only 0's and 1's!": "Binary sequence must contain only 0 and 1 values."}


def load_group(group):
    with np.load(os.path.join(GOLDEN, f"bits_{group}.npz")) as z:
        return {k: z[k] for k in z.files}


def load_namespace(upload=None):
    """The operands as the fixture holds them (not regenerated)."""
    v = {}
    with np.load(os.path.join(GOLDEN, "bits_inputs.npz")) as z:
        for k in z.files:
            if k in bc.SEQUENCES:
                x = binary_sequence(z[k])
                v[k] = upload(x) if upload else x
            elif k == "s":
                v[k] = str(z[k])
            elif k == "l":
                v[k] = [int(b) for b in z[k]]
            elif k != "versions":
                v[k] = z[k]
    gv(sps=8)
    return v


def expected(fix, name):
    return {k.rsplit("|", 1)[1]: a for k, a in fix.items() if k.rsplit("|", 1)[0] == name}


def mismatch(want, got):
    """None when the outcome `got` is the fixture's `want`, else a description."""
    kind = str(want["kind"])
    if str(got["kind"]) != kind:
        return f"kind {got['kind']} ({got.get('text', '')}), expected {kind} ({want.get('text', '')})"
    if kind == "error":
        if str(got["type"]) != str(want["type"]):
            return f"{got['type']}: {got['text']}, expected {want['type']}: {want['text']}"
        text = str(want["text"])
        if "broadcast" in text:                  # NumPy's words in the reference, this class's here: both name the two shapes
            shapes = text[text.index("shapes") + 7:].strip()
            return None if "broadcast" in str(got["text"]) and str(got["text"]).endswith(shapes) else f"text {got['text']}, expected the shapes {shapes}"
        return None if str(got["text"]) == NOT_BITS.get(text, text) else f"text {got['text']!r}, expected {NOT_BITS.get(text, text)!r}"
    if kind == "signal":
        a, b = want["value"], got["value"]
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{b.dtype} {b.shape}, expected {a.dtype} {a.shape}"
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        return None if err <= 1e-12 else f"error {err:.3e} of the peak"
    key = "data" if kind == "bits" else "value"
    a, b = want[key], got[key]
    return None if a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) else f"{b.dtype} {b.shape}, expected {a.dtype} {a.shape}"


def test_there_are_fixtures():
    assert sum(N_CASES.values()) == len(CASES) == 215
    for g, count in N_CASES.items():
        assert len({k.rsplit("|", 1)[0] for k in load_group(g) if k != "versions"}) == count, g
    kinds = [str(a) for g in N_CASES for k, a in load_group(g).items() if k.endswith("|kind")]
    assert {k: kinds.count(k) for k in set(kinds)} == {"bits": 129, "error": 31, "int": 45, "signal": 5, "array": 5}


def test_the_fixture_inputs_are_the_cases_inputs():
    v, w = load_namespace(), bc.namespace(binary_sequence, gv)
    assert v.keys() == w.keys()
    for k in v:
        if isinstance(v[k], binary_sequence):
            assert np.array_equal(v[k].data, w[k].data) and v[k].data.dtype == np.uint8 and v[k].size <= 300
        elif isinstance(v[k], (str, list)):
            assert v[k] == w[k]
        else:
            assert np.array_equal(v[k], w[k]) and v[k].dtype == w[k].dtype


@pytest.mark.parametrize("group", bc.GROUPS)
def test_host_path_matches_the_reference(group):
    fix, v = load_group(group), load_namespace()
    before = dict(_lib.TRANSFERS)
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        got = bc.outcome(fn, v)
        why = mismatch(expected(fix, name), got)
        if why:
            bad.append((cid, why))
        if str(got["kind"]) == "int":
            r = fn(v)
            assert type(r) is int, (cid, type(r))               # Python integers, not NumPy scalars
    gv.default()
    assert not bad, bad[:10]
    assert _lib.TRANSFERS == before                 # a host-only sequence never loads a device
    assert all(not x.on_device for x in v.values() if isinstance(x, binary_sequence))


def test_host_algebra_never_loads_the_library():
    """In a process of its own: after every kind of operation on host sequences the shared library has not been loaded, let alone a device
    opened (this process may have loaded it for another test file)."""
    code = ("import numpy as np\n"
            "from opticomlib_amd import _lib, binary_sequence as B, gv\n"
            "a, b = B('1100'), B([1, 0, 1, 0])\n"
            "r = (~a, a & b, a | '1111', 1 ^ a, a != b, a + b, np.array([1, 0]) + a, a * 3, np.array([1, 0, 1, 1]) * a, a[::-1], a[1], a.flip())\n"
            "assert (a.ones, a.zeros, a.hamming_distance(b), (B([]) & 1).size, len(str(a)) > 0) == (2, 2, 2, 0, True)\n"
            "gv(sps=4); assert a.dac(np.ones(4)).size == 16\n"
            "assert _lib._lib is None and _lib.TRANSFERS == {'h2d': 0, 'd2h': 0}\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_the_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and f"SSFM_API int {s}(int device" not in hdr and s in _lib.SYMBOLS and s in names, s
    assert {n for n in names if n.startswith("ssfm_bits_")} == set(NEW_SYMBOLS)
    assert "#define SSFM_ABI_VERSION 3" in hdr
    assert "enum { SSFM_BITS_AND = 0, SSFM_BITS_OR = 1, SSFM_BITS_XOR = 2 };" in hdr
    assert (_lib.BITS_AND, _lib.BITS_OR, _lib.BITS_XOR) == (0, 1, 2)
    mk = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()
    assert "bits.hip" in mk
    src = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "bits.hip")).read()
    assert "float" not in src.replace("nothing in this file is a float", "") and "double" not in src      # integers only


def test_ne_is_a_mask_and_eq_stays_a_host_bool_array():
    a, b = binary_sequence("1100"), binary_sequence("1010")
    ne, eq = a != b, a == b
    assert isinstance(ne, binary_sequence) and list(ne.data) == [0, 1, 1, 0] and a.hamming_distance(b) == ne.ones == 2
    assert isinstance(eq, np.ndarray) and eq.dtype == bool and list(eq) == [True, False, False, True] and not (a == b).all()
    with pytest.raises(TypeError, match="unhashable"):
        hash(a)


def test_mul_takes_the_references_branches():
    a = binary_sequence("101")
    assert list((a * 2).data) == [1, 0, 1, 1, 0, 1] and list((2 * a).data) == [1, 0, 1, 1, 0, 1]
    assert list((a * 1).data) == [1, 0, 1] and list((a * True).data) == [1, 0, 1] and list((a * 0).data) == [0, 0, 0]
    assert list((a * binary_sequence("110")).data) == [1, 0, 0]
    for k in (2.0, -1, np.int64(2)):             # not an `int` above 1: the constructor refuses the value
        with pytest.raises(ValueError, match="only 0 and 1"):
            a * k


def test_frames_print_and_protocols():
    pre, word = binary_sequence("1110010"), binary_sequence([1, 0, 0, 1])
    frame = pre + word * 3
    assert frame.size == 19 and str(np.asarray(frame).dtype) == "uint8" and frame.ones == 10 and frame.zeros == 9 and frame.sizeof == 19
    assert list(("10" + word).data) == [1, 0, 1, 0, 0, 1] and list((np.array([1, 1]) + word).data) == [1, 1, 1, 0, 0, 1]
    assert list((np.array([1, 1, 0, 0]) * word).data) == [1, 0, 0, 0]
    assert list(np.bitwise_and(np.array([1, 1, 0, 0]), word)) == [1, 0, 0, 0]          # another ufunc: NumPy's own result
    assert frame.print("frame") is frame and "ones  :  10" in str(frame) and "frame" in frame.__str__("frame")
    assert frame.to_numpy(dtype=float).dtype == np.float64 and [b for b in word] == [1, 0, 0, 1]
    assert frame.flip().ones == 9 and isinstance(frame[2:5], binary_sequence) and frame[0] == 1 and type(frame[0]) is int
    gv(sps=4)
    y = word.dac(np.ones(4))
    gv.default()
    assert isinstance(y, electrical_signal) and y.size == 16 and not y.on_device


def test_prbs_is_devices_prbs(monkeypatch):
    """The static method hands its arguments to ``devices.PRBS`` (whose bits are tested against the reference's) and imports it when called."""
    from opticomlib_amd import devices
    calls = []
    monkeypatch.setattr(devices, "PRBS", lambda *a: calls.append(a) or "seq")
    assert binary_sequence.prbs(7, 20, 5, True) == "seq" and binary_sequence.prbs(9) == "seq"
    assert calls == [(7, 20, 5, True), (9, None, None, False)]
