"""Welch's PSD on the MI355X: get_psd against the reference's fixtures (tests/golden/psd_*.npz) and against live SciPy over every route, the
device residency of its input, determinism, no host fallback, duck typing, and the signals' .psd() plots."""
import glob
import os
import warnings

import numpy as np
import pytest
import scipy.signal as sg

import opticomlib_amd as oa
from opticomlib_amd import _lib, utils
from opticomlib_amd.typing import electrical_signal, gv, optical_signal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "psd_*.npz")))
NPERSEGS = (1, 2, 3, 15, 16, 17, 1000, 2047, 2048, 8192, 8193, 16384)
DTYPES = (np.float32, np.float64, np.complex64, np.complex128)


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def scipy_psd(x, fs, nperseg):
    """SciPy in float64 on the same (widened) values, fftshifted."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    f, p = sg.welch(x, fs=fs, nperseg=nperseg, scaling="spectrum", return_onesided=False, detrend=False)
    return np.fft.fftshift(f), np.fft.fftshift(p, axes=-1)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(b)))


def test_there_are_fixtures():
    assert len(FIXTURES) >= 8


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_matches_the_reference_fixture(path):
    g = dict(np.load(path))
    x = np.exp(1j * g["phase"].astype(np.float64)) if "phase" in g else g["x"]
    nperseg = None if int(g["nperseg"]) < 0 else int(g["nperseg"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        f, psd = oa.get_psd(x, float(g["fs"]), nperseg)
    msgs = [str(m.message) for m in w if issubclass(m.category, UserWarning)]
    assert msgs == ([str(g["warning"])] if str(g["warning"]) else []), msgs
    np.testing.assert_array_equal(f, g["f"])
    assert f.dtype == g["f"].dtype and psd.dtype == g["psd"].dtype and psd.shape == g["psd"].shape
    tol = 1e-5 if psd.dtype == np.float32 else 1e-12
    assert rel(psd, g["psd"]) <= tol, rel(psd, g["psd"])


def _input(dtype, rows, n, seed):
    rng = np.random.default_rng(seed)
    shape = (n,) if rows == 1 else (rows, n)
    x = rng.standard_normal(shape) + 0.5 * np.cos(np.arange(n) * 0.3)
    if np.issubdtype(dtype, np.complexfloating):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def _lengths(nperseg):
    return sorted({nperseg, nperseg + 1, 3 * nperseg + 5, 11 * nperseg // 2 + 3})


@pytest.mark.parametrize("nperseg", NPERSEGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_sweep_against_scipy(nperseg, dtype):
    for rows in (1, 2):
        for k, n in enumerate(_lengths(nperseg)):
            x = _input(dtype, rows, n, 1000 * nperseg + 10 * k + rows)
            f, psd = oa.get_psd(x, 3.0, nperseg)
            rf, rp = scipy_psd(x, 3.0, nperseg)
            np.testing.assert_array_equal(f, rf)
            f32 = np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))
            assert psd.dtype == (np.float32 if f32 else np.float64) and psd.shape == rp.shape
            assert rel(psd, rp) <= (1e-7 if f32 else 1e-12), (nperseg, dtype, rows, n, rel(psd, rp))


def test_a_big_dual_pol_field_at_8192():
    x = _input(np.complex64, 2, 1 << 22, 7)
    f, psd = oa.get_psd(x, 1.0, 8192)
    rf, rp = scipy_psd(x, 1.0, 8192)
    np.testing.assert_array_equal(f, rf)
    assert psd.shape == (2, 8192) and rel(psd, rp) <= 1e-7


def test_the_chirp_route_in_several_chunks():
    """nperseg = 17 on 2 x 2^20 samples: 233 016 segments, more than one chunk (a plan holds at most 65 535 rows)."""
    x = _input(np.complex128, 2, 1 << 20, 17)
    assert 2 * utils._welch_layout(1 << 20, 17)["nseg"] > 2 * utils._MAX_PLAN_BATCH
    f, psd = oa.get_psd(x, 1.0, 17)
    assert rel(psd, scipy_psd(x, 1.0, 17)[1]) <= 1e-12


def test_leading_shape_is_rows():
    x = _input(np.complex128, 1, 3 * 4 * 700, 3).reshape(3, 4, 700)
    f, psd = oa.get_psd(x, 1.0, 64)
    assert psd.shape == (3, 4, 64)
    assert rel(psd, scipy_psd(x, 1.0, 64)[1]) <= 1e-12


def test_integer_input():
    x = (np.arange(5000) % 7).astype(np.int64)
    f, psd = oa.get_psd(x, 1.0, 256)
    assert psd.dtype == np.float64 and rel(psd, scipy_psd(x, 1.0, 256)[1]) <= 1e-12


def test_device_fields_stay_on_the_device():
    gv(sps=16, R=10e9, N=4096)
    laser = oa.LASER(0, lw=1e6, rng="device")
    rng = np.random.default_rng(5)
    field = optical_signal(((rng.standard_normal((2, 1 << 16)) + 1j * rng.standard_normal((2, 1 << 16))) * 0.02).astype(np.complex64))
    fib = oa.FIBER(field, length=5, alpha=0.2, beta_2=-20, gamma=1.3)
    for sig in (laser, fib):
        raw = sig._raw("signal")
        assert isinstance(raw, _lib.DeviceArray)
        h2d, d2h = _lib.TRANSFERS["h2d"], _lib.TRANSFERS["d2h"]
        f, psd = oa.get_psd(sig, gv.fs, 8192)
        assert _lib.TRANSFERS["h2d"] == h2d and _lib.TRANSFERS["d2h"] - d2h <= 1
        assert isinstance(sig._raw("signal"), _lib.DeviceArray)
        f2, psd2 = oa.get_psd(raw.to_host(), gv.fs, 8192)
        np.testing.assert_array_equal(psd, psd2)
        np.testing.assert_array_equal(f, f2)


def test_device_field_on_the_chirp_route_stays_on_the_device():
    gv(sps=16, R=10e9, N=1024)
    laser = oa.LASER(3, lw=5e6, rng="device")
    h2d, d2h = _lib.TRANSFERS["h2d"], _lib.TRANSFERS["d2h"]
    f, psd = oa.get_psd(laser, gv.fs, 3000)
    assert _lib.TRANSFERS["h2d"] == h2d and _lib.TRANSFERS["d2h"] - d2h <= 1
    assert rel(psd, scipy_psd(laser.signal, gv.fs, 3000)[1]) <= 1e-12


@pytest.mark.parametrize("nperseg", (2, 1024, 8192, 3000))
def test_two_calls_give_the_same_bits(nperseg):
    x = _input(np.complex128, 2, 100_000, 11)
    a = oa.get_psd(x, 1.0, nperseg)[1]
    b = oa.get_psd(x, 1.0, nperseg)[1]
    np.testing.assert_array_equal(a, b)


def test_no_host_fallback(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("scipy.signal.welch must not be called")
    monkeypatch.setattr(sg, "welch", boom)
    import scipy.signal
    monkeypatch.setattr(scipy.signal, "welch", boom)
    x = _input(np.float64, 1, 20000, 2)
    for nperseg in (5, 512, 1500):
        f, psd = oa.get_psd(x, 1.0, nperseg)
        assert psd.shape == (nperseg,) and np.all(np.isfinite(psd))


def test_duck_typing_and_the_reference_example():
    fs = 10e9
    t = np.arange(0, 1000e-9, 1 / fs)
    sig = np.sin(2 * np.pi * 1e9 * t)
    f, psd = oa.get_psd(sig, fs)
    k = int(np.argmax(psd))
    assert abs(abs(f[k]) - 1e9) < 50e6 and abs(psd[k] - 0.25) < 0.05       # the reference test's checks (utils_test.py:12)

    class MockSignal:
        def __init__(self, s):
            self.signal = s
    f2, psd2 = oa.get_psd(MockSignal(sig), fs)
    np.testing.assert_array_equal(f, f2)
    np.testing.assert_array_equal(psd, psd2)
    f3, psd3 = oa.get_psd(list(sig[:300]), fs)                              # a list: array_like
    np.testing.assert_array_equal(psd3, oa.get_psd(sig[:300], fs)[1])


def test_signal_objects_use_the_signal_only():
    rng = np.random.default_rng(9)
    s, nz = rng.standard_normal(4096), rng.standard_normal(4096)
    np.testing.assert_array_equal(oa.get_psd(electrical_signal(s, nz), 1.0)[1], oa.get_psd(s, 1.0)[1])
    dual = (rng.standard_normal((2, 4096)) + 1j * rng.standard_normal((2, 4096))).astype(np.complex64)
    f, psd = oa.get_psd(optical_signal(dual), 1.0)                           # default nperseg = len(sig) = 2
    assert psd.shape == (2, 2) and rel(psd, scipy_psd(dual, 1.0, 2)[1]) <= 1e-7


# ----------------------------------------------------------------------------------------------- .psd()
def _lines():
    import matplotlib.pyplot as plt
    return plt.gca().get_lines()


def _dbm(p):
    with np.errstate(divide="ignore"):
        return 10 * np.log10(p) + 30


@pytest.fixture
def agg():
    mpl = pytest.importorskip("matplotlib")
    mpl.use("Agg")
    import matplotlib.pyplot as plt
    plt.close("all")
    yield plt
    plt.close("all")


def test_electrical_psd_plot(agg):
    gv(sps=16, R=10e9, N=512)
    rng = np.random.default_rng(1)
    x = electrical_signal(rng.standard_normal(10000))
    assert x.psd('--b', n=98, xlabel='Freq', ylabel='Spectra', grid=False, hold=True) is x      # the reference test (typing_test.py:737)
    agg.close("all")
    assert x.psd() is x
    (line,) = _lines()
    n = min(x.size, gv.t.size)
    f, p = scipy_psd(x.signal[:n], gv.fs * 1e-9, 2048)
    np.testing.assert_array_equal(line.get_xdata(), f)
    assert np.max(np.abs(line.get_ydata() - _dbm(p))) < 1e-9
    agg.close("all")
    x.psd(yscale='linear')
    (line,) = _lines()
    assert rel(line.get_ydata(), p * 1e3) <= 1e-12
    with pytest.raises(TypeError, match='`yscale` must be one of the following values \\("linear", "dbm"\\)'):
        x.psd(yscale='db')


def test_optical_psd_plot(agg):
    gv(sps=16, R=10e9, N=1024)
    rng = np.random.default_rng(2)
    dual = (rng.standard_normal((2, 20000)) + 1j * rng.standard_normal((2, 20000))) * 0.1
    x = optical_signal(dual)
    n = min(x.size, gv.t.size)
    f, p = scipy_psd(dual[:, :n], gv.fs * 1e-9, 2048)
    for mode, want in (("x", [p[0]]), ("y", [p[1]]), ("both", [p[0], p[1]])):
        agg.close("all")
        assert x.psd(mode=mode) is x
        lines = _lines()
        assert len(lines) == len(want)
        for line, w in zip(lines, want):
            np.testing.assert_array_equal(line.get_xdata(), f)
            assert np.max(np.abs(line.get_ydata() - _dbm(w))) < 1e-9
    agg.close("all")
    x.psd(mode='both', yscale='linear', label='sig')
    lines = _lines()
    assert [l.get_label() for l in lines] == ['sig X', 'sig Y']
    assert rel(lines[1].get_ydata(), p[1] * 1e3) <= 1e-12
    assert x.psd('--r', mode='x', n=98, xlabel='Freq', ylabel='Spectra', grid=True, hold=True) is x             # typing_test.py:1277
    assert x.psd('--b', mode='both', n=98, xlabel='Freq', ylabel='Spectra', grid=False, hold=True) is x
    with pytest.raises(TypeError, match='argument `mode` should be \\("x", "y" or "both"\\)'):
        x.psd(mode='z')
    with pytest.raises(TypeError, match='`yscale` must be one of the following values'):
        x.psd(yscale='dB')


def test_psd_plot_of_a_device_field(agg):
    gv(sps=16, R=10e9, N=256)
    rng = np.random.default_rng(3)
    field = optical_signal(((rng.standard_normal((2, 8192)) + 1j * rng.standard_normal((2, 8192))) * 0.02).astype(np.complex64))
    y = oa.FIBER(field, length=2, alpha=0.2, beta_2=-20, gamma=1.3)
    assert isinstance(y._raw("signal"), _lib.DeviceArray)
    h2d, d2h = _lib.TRANSFERS["h2d"], _lib.TRANSFERS["d2h"]
    y.psd(mode='y')
    assert _lib.TRANSFERS["h2d"] == h2d and _lib.TRANSFERS["d2h"] == d2h
    (line,) = _lines()
    n = min(y.size, gv.t.size)                                               # 4096 of 8192 samples: a row stride, not a copy
    f, p = scipy_psd(y.signal[:, :n], gv.fs * 1e-9, 2048)
    assert np.max(np.abs(line.get_ydata() - _dbm(p[1]))) < 5e-5                 # the float32 result in dBm, rounded in float32: ~2e-6 per ulp
