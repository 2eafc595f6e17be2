"""CPU-side checks of the data-aided receiver (opticomlib_amd/lab.py, csrc/sync.hip): the NumPy restatement tests/sync_numpy.py reproduces the
reference's fixtures, the C ABI holds the new entry points, the module imports without the instrument libraries, and the argument errors
come before the library is loaded."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sync_numpy as sn
from opticomlib_amd import _lib
from opticomlib_amd.typing import binary_sequence, electrical_signal, gv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNC_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sync_*.npz")))
EYE_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "eyev2_*.npz")))
NEW_SYMBOLS = ("ssfm_load_template", "ssfm_sync_peak", "ssfm_eye_levels_known", "ssfm_eye_split_known")
EMPTY = "Signal must be scalar or 1D array for electrical_signal, invalid shape (0,)"


def name_of(path):
    return os.path.basename(path)[:-4]


def load_case(path):
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    for k in ("sps", "nslots", "i"):
        if k in g:
            g[k] = int(g[k])
    for k in ("raises", "message"):
        if k in g:
            g[k] = str(g[k])
    return g


def test_the_fixtures_cover_what_the_issue_asks():
    names = {name_of(p) for p in SYNC_GOLDEN + EYE_GOLDEN}
    assert {"sync_sps8_inside", "sync_sps16_inside", "sync_sps8_first_lag", "sync_sps16_last_lag", "sync_sps8_inverted", "sync_sps8_exact_length",
            "eyev2_gauss_sps8", "eyev2_gauss_sps16_clean", "eyev2_nrz_sps32_nslots64"} <= names
    for p in SYNC_GOLDEN + EYE_GOLDEN:
        assert os.path.getsize(p) < (1 << 20), p


@pytest.mark.parametrize("path", SYNC_GOLDEN, ids=name_of)
def test_restatement_reproduces_the_reference_sync(path):
    g = load_case(path)
    if g["raises"] and g["message"] != EMPTY:
        with pytest.raises(ValueError, match=re.escape(g["message"])):
            sn.sync(g["rx"], g["tx"], g["sps"])
        return
    r = sn.sync(g["rx"], g["tx"], g["sps"])
    if g["raises"]:                                             # the reference's constructor refused the empty slice
        assert g["raises"] == "ValueError" and r["signal"].size == 0
        l = g["tx"].size * g["sps"]
        assert r["i"] == l or g["rx"].size == l
        return
    assert r["i"] == g["i"]
    np.testing.assert_array_equal(r["signal"], g["signal"])
    assert bool(g["noise_is_null"])
    # the direct longdouble sums agree with SciPy's FFT correlation far inside the margin the peak has
    d = sn.correlation_direct(g["rx"], g["tx"], g["sps"])
    assert int(np.argmax(d)) == g["i"]
    assert np.max(np.abs(d - r["corr"])) <= 1e-12 * np.max(np.abs(d))


@pytest.mark.parametrize("path", EYE_GOLDEN, ids=name_of)
def test_restatement_reproduces_the_reference_eye(path):
    g = load_case(path)
    x = g["x"] + g["noise"] if g["noise"].size else g["x"]
    r = sn.get_eye_v2(x, g["tx"], g["sps"], g["nslots"])
    span = float(g["mu1"] - g["mu0"])
    for k in ("mu0", "mu1", "s0", "s1"):
        assert abs(r[k] - float(g[k])) <= 1e-12 * span, (k, r[k], float(g[k]))
    assert abs(r["threshold"] - float(g["threshold"])) <= span / 499 * (1 + 1e-9)
    for k in ("i", "t_left", "t_right", "t_dist", "t_opt", "t_span0", "t_span1"):
        assert r[k] == float(g[k]), k
    for k in ("y", "ones", "zeros"):
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)
    assert r["t0"].size == int(g["t0_size"]) and r["t1"].size == int(g["t1_size"])
    np.testing.assert_allclose([r["er"], r["eye_h"]], [float(g["er"]), float(g["eye_h"])], rtol=1e-11)


def test_restatement_raises_as_the_reference_does():
    with pytest.raises(BufferError):
        sn.sync(np.ones(15), np.ones(2), 8)
    with pytest.raises(IndexError):
        sn.get_eye_v2(np.arange(64.0), np.ones(3), 8)
    with pytest.raises(np.linalg.LinAlgError):
        sn.get_eye_v2(np.full(64, 0.5), np.array([0, 1] * 4), 8)


def test_abi_holds_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    vers = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "exports.map")).read()
    assert "ssfm_*;" in vers                                    # the version script exports the C ABI by its prefix
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and s in _lib.SYMBOLS and s in names, s
    assert "lab.SYNC and lab.GET_EYE_v2" in hdr
    assert "sync.hip" in open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()
    assert _lib.load().ssfm_abi_version() == 3


def test_lab_imports_without_the_instrument_libraries():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('pyvisa', 'h5py', 'serial'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "import opticomlib_amd.lab as lab\n"
            "import opticomlib_amd as oa\n"
            "assert oa.lab is lab and callable(lab.SYNC) and callable(lab.GET_EYE_v2)\n"
            "assert not {'pyvisa', 'h5py', 'serial'} & set(sys.modules)\n"
            "from opticomlib_amd import _lib\n"
            "assert _lib._lib is None\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    from opticomlib_amd import lab

    def no_load():
        raise AssertionError("the library was loaded before the argument check")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_lib", None)
    gv(sps=8, R=1e9)
    word = np.array([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    rx = np.zeros(8 * 8 * 2)
    with pytest.raises(TypeError, match='The "signal_rx" must be of type `electrical_signal` or `np.ndarray`.'):
        lab.SYNC(list(rx), word, 8)
    with pytest.raises(TypeError, match='The "slots_tx" must be of type `binary_sequence` or `np.ndarray`.'):
        lab.SYNC(rx, list(word), 8)
    with pytest.raises(ValueError, match='"sps" must be provided to perform synchronization.'):
        lab.SYNC(rx, word)
    with pytest.raises(TypeError):
        lab.SYNC(rx, word, 8.0)
    with pytest.raises(TypeError, match="complex"):
        lab.SYNC(rx.astype(complex), word, 8)
    with pytest.raises(TypeError, match="complex"):
        lab.SYNC(electrical_signal(rx.astype(complex)), binary_sequence(word))
    with pytest.raises(BufferError, match="The length of the received vector must be greater than the transmitted vector!!"):
        lab.SYNC(rx[:63], word, 8)
    with pytest.raises(BufferError):
        lab.SYNC(electrical_signal(rx[:63]), binary_sequence(word))
    with pytest.raises(ValueError, match="only 0 and 1"):
        lab.SYNC(rx, np.array([0, 2, 1]), 8)
    with pytest.raises(IndexError, match="boolean index did not match indexed array along axis 0; size of axis is 128 but size of corresponding boolean axis is 64"):
        lab.GET_EYE_v2(electrical_signal(rx), word)
    with pytest.raises(IndexError):
        lab.GET_EYE_v2(rx, "1010")
    with pytest.raises(ValueError, match="only 0 and 1"):
        lab.GET_EYE_v2(rx, np.arange(16))


def test_a_get_eye_eye_has_no_known_slot_attributes():
    from opticomlib_amd.typing import eye
    e = eye(sps=8, dt=1.0, y=np.zeros(16), _nslots=2, t_opt=0.0, i=4, mu0=0.0, mu1=1.0, s0=0.1, s1=0.1, threshold=0.5)
    for k in ("ones", "zeros", "t0", "t1"):
        assert not hasattr(e, k), k
    assert repr(e) == "eye(sps=8, t_opt=0.0, i=4, mu0=0, mu1=1, s0=0.1, s1=0.1, threshold=0.5)"
    v2 = eye(sps=4, dt=1.0, y=np.zeros(8), ones=np.arange(4.0), zeros=np.arange(4.0), _nslots=2, _n0=1, _n1=1)
    np.testing.assert_array_equal(v2.t0, [-0.5, -0.25, 0.0, 0.25])
    np.testing.assert_array_equal(v2.ones, np.arange(4.0))
    assert v2.t1 is v2.t1 and v2.t.size == 8
