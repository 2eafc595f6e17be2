"""Welch's PSD without a GPU: the new entry points of the C ABI, the host's segment layout against SciPy's, and get_psd's argument rules
(the reference's default nperseg with its 2-D quirk, SciPy 1.15's checks and warning, the output dtype and the window scale)."""
import os
import subprocess
import warnings

import numpy as np
import pytest
import scipy.signal as sg

from opticomlib_amd import utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssfm_welch", "ssfm_welch_frames", "ssfm_welch_accumulate", "ssfm_welch_finish")
NPERSEGS = (1, 2, 3, 15, 16, 17, 1000, 2047, 2048, 8192, 8193, 16384)


def test_get_psd_is_exported():
    import opticomlib_amd as oa
    assert "get_psd" in oa.__all__ and oa.get_psd is utils.get_psd
    assert callable(oa.electrical_signal.psd) and callable(oa.optical_signal.psd)


def test_the_new_entry_points_are_declared_bound_and_exported():
    from opticomlib_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and s in _lib.SYMBOLS and s in names, s
    assert "#define SSFM_ABI_VERSION 3" in hdr
    assert "utils.py:2048-2079 (get_psd" in hdr


@pytest.mark.parametrize("nperseg", NPERSEGS)
def test_layout_is_scipys(nperseg):
    """nseg / noverlap / step against the segment times of scipy.signal.spectrogram, which shares Welch's segmenting."""
    for n in sorted({nperseg, nperseg + 1, nperseg + nperseg // 2, 2 * nperseg - 1, 3 * nperseg + 7, 5 * nperseg + nperseg // 3 + 1}):
        lay = utils._welch_layout(n, nperseg)
        t = sg.spectrogram(np.zeros(n), fs=1.0, window="hann", nperseg=nperseg, noverlap=nperseg // 2, detrend=False)[1]
        assert lay["nseg"] == t.size, (n, nperseg)
        assert lay["noverlap"] == nperseg // 2 and lay["step"] == nperseg - nperseg // 2
        # the last segment ends inside the input, and one more would not
        assert (lay["nseg"] - 1) * lay["step"] + nperseg <= n < lay["nseg"] * lay["step"] + nperseg
        want = 2 if nperseg < 16 else (1 if nperseg <= 8192 and nperseg & (nperseg - 1) == 0 else 3)
        assert lay["route"] == want, (nperseg, lay)


def test_layout_when_n_equals_nperseg():
    for nperseg in NPERSEGS:
        assert utils._welch_layout(nperseg, nperseg)["nseg"] == 1


def test_default_nperseg_is_the_references_rule():
    assert utils._default_nperseg(np.zeros(10000)) == 2048
    assert utils._default_nperseg(np.zeros(1000)) == 1000
    assert utils._default_nperseg(np.zeros((2, 1 << 20), np.complex64)) == 2            # len() of a dual-polarisation field: its rows
    # ... and SciPy indeed returns (2, 2) for it
    assert sg.welch(np.ones((2, 64), np.complex64), nperseg=2, return_onesided=False, detrend=False)[1].shape == (2, 2)


def test_invalid_nperseg_matches_scipy():
    for bad in (0, -1, -2048):
        with pytest.raises(ValueError, match="^nperseg must be a positive integer$"):
            utils.get_psd(np.ones(100), 1.0, bad)
        with pytest.raises(ValueError, match="^nperseg must be a positive integer$"):
            sg.welch(np.ones(100), nperseg=bad)
    assert utils._validate_nperseg(2.5, 100) == 2 and utils._validate_nperseg(np.float64(7.9), 100) == 7 and utils._validate_nperseg(1, 100) == 1


def test_long_nperseg_warns_like_scipy():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert utils._validate_nperseg(2048, 1000) == 1000
    assert [str(m.message) for m in w] == ["nperseg = 2048 is greater than input length  = 1000, using nperseg = 1000"]
    assert w[0].category is UserWarning


def test_non_numeric_input_is_a_type_error():
    for bad in ("abc", object(), 3.0, ["a", "b"]):
        with pytest.raises(TypeError, match="signal must be array_like or have a .signal attribute"):
            utils.get_psd(bad, 1.0)


def test_empty_input_gives_empty_arrays():
    f, p = utils.get_psd(np.zeros(0), 1.0, 16)
    rf, rp = sg.welch(np.zeros(0), nperseg=16, return_onesided=False, detrend=False)
    assert f.shape == rf.shape and p.shape == rp.shape


def test_output_dtype_is_scipys():
    for dt in (np.bool_, np.int8, np.int16, np.int32, np.int64, np.uint8, np.float16, np.float32, np.float64, np.complex64, np.complex128):
        x = (np.arange(64) % 3).astype(dt)
        want = sg.welch(x, nperseg=16, scaling="spectrum", return_onesided=False, detrend=False)[1].dtype
        assert (want == np.float32) == utils._out_f32(np.dtype(dt)), dt


@pytest.mark.parametrize("nperseg", NPERSEGS)
def test_window_scale_is_scipys(nperseg):
    w = sg.get_window("hann", nperseg)
    assert utils._hann_scale(nperseg) == 1.0 / w.sum() ** 2
