"""The OOK receiver on the MI355X (csrc/eye.hip): GET_EYE / SAMPLER / ook.DSP / BER_analizer against the reference's fixtures and,
exactly, against the NumPy restatement tests/eye_numpy.py (the same deterministic two-means)."""
import glob
import os

import numpy as np
import pytest
import scipy.signal as sg

import eye_numpy as en
import opticomlib_amd as oa
from opticomlib_amd import _lib, ook
from opticomlib_amd.typing import binary_sequence, electrical_signal, gv
from test_eye_cpu import GOLDEN, check_eye, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


DISCRETE = ("t_left", "t_right", "t_opt", "i", "y_left", "y_right", "t_span0", "t_span1")


def assert_same_as_restatement(e, r):
    span = r["mu1"] - r["mu0"]
    for k in DISCRETE:
        assert getattr(e, k) == r[k], (k, getattr(e, k), r[k])
    for k in ("mu0", "mu1", "s0", "s1"):
        assert abs(getattr(e, k) - r[k]) <= 1e-12 * abs(span), (k, getattr(e, k), r[k])
    for k in ("top_int", "bot_int"):                           # sample values of the resampled signal: the transforms differ in the last bits
        np.testing.assert_allclose(getattr(e, k), r[k], rtol=0, atol=1e-12 * abs(span), err_msg=k)
    if r["threshold"] is None:
        assert e.threshold is None
    else:
        assert abs(e.threshold - r["threshold"]) <= abs(span) / 499 * (1 + 1e-9)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_device_against_the_reference(path):
    g = load_case(path)
    gv(sps=g["sps"], R=float(g["R"]))
    x = electrical_signal(g["x"])
    if g["what"] == "eye":
        e = oa.GET_EYE(x, nslots=g["nslots"], sps_resamp=g["sps_resamp"])
        check_eye(e, g)
        return
    bw = None if np.isnan(g["BW"]) else float(g["BW"])
    rx, e, rth = ook.DSP(x, BW=bw)
    check_eye(e, g)
    span = float(g["mu1"] - g["mu0"])
    assert abs(rth - g["rth"]) <= span / 999 * (1 + 1e-9)
    np.testing.assert_array_equal(rx.data, g["rx"])
    assert ook.BER_analizer("counter", Tx=binary_sequence(g["tx"]), Rx=rx) == g["ber_counter"]
    # and against the restatement on the same (filtered) signal
    xr = g["x"] if bw is None else oa.LPF(electrical_signal(g["x"]), bw).signal       # the device's own filter output
    bits, r, rth_r = en.dsp(xr, g["sps"])
    assert_same_as_restatement(e, r)
    np.testing.assert_array_equal(rx.data, bits)


def random_eye(seed):
    rng = np.random.default_rng(seed)
    sps = int(rng.choice([8, 16, 32, 64]))
    nbits = int(rng.integers(60, 1500))
    lo, hi = sorted(rng.uniform(-1, 2, 2))
    hi += 0.2
    bits = rng.integers(0, 2, nbits)
    x = np.repeat(lo + (hi - lo) * bits, sps).astype(float)
    width = rng.uniform(0.05, 0.4) * sps
    k = np.arange(-3 * sps, 3 * sps + 1)
    h = np.exp(-0.5 * (k / width) ** 2)
    x = np.convolve(x, h / h.sum(), mode="same")
    x += rng.normal(0, rng.uniform(0.01, 0.12) * (hi - lo), x.size)
    x = x[: x.size - int(rng.integers(0, sps))]                                       # odd lengths
    nslots = int(rng.choice([4096, 2 * int(rng.integers(8, 400))]))
    resamp = [None, 32, 64, 128][int(rng.integers(0, 4))]
    return x, sps, nslots, resamp


@pytest.mark.parametrize("seed", range(20))
def test_device_against_the_restatement(seed):
    x, sps, nslots, resamp = random_eye(seed)
    gv(sps=sps, R=1e9)
    e = oa.GET_EYE(x, nslots=nslots, sps_resamp=resamp)
    r = en.get_eye(x, sps, nslots, resamp)
    assert_same_as_restatement(e, r)
    np.testing.assert_allclose(e.y, r["y"], rtol=0, atol=1e-12 * np.max(np.abs(r["y"])))


def test_results_are_identical_across_calls():
    x, sps, nslots, resamp = random_eye(101)
    gv(sps=sps, R=1e9)
    a, b = oa.GET_EYE(x, nslots, 128), oa.GET_EYE(x, nslots, 128)
    for k in DISCRETE + ("mu0", "mu1", "s0", "s1", "threshold", "er", "eye_h"):
        assert getattr(a, k) == getattr(b, k), k
    np.testing.assert_array_equal(a.y, b.y)


def test_round_trips_are_counted_and_fixed():
    """Every blocking host wait of a call on a device-resident signal: 4 without resampling, 9 with it (an open eye)."""
    x, sps, nslots, resamp = random_eye(3)
    gv(sps=sps, R=1e9)
    d = oa.devices._wrap_out(electrical_signal, _lib.DeviceArray.from_host(x, np.float64), oa.NULL)
    assert oa.GET_EYE(d, nslots).round_trips == 4
    assert oa.GET_EYE(d, nslots, 128).round_trips == 9


@pytest.mark.parametrize("n", [1, 2, 7, 2048, 2049, 100_003, 1 << 20, 1 << 21])
def test_sort_is_np_sort_bit_for_bit(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, np.inf, -np.inf, 1.0, 1.0, -1.0, 0.0, -0.0])
    x[rng.integers(0, n, min(n, special.size))] = special[: min(n, special.size)]
    x[: n // 3] = np.round(x[: n // 3])                                               # duplicates
    d = _lib.DeviceArray.from_host(x, np.float64)
    _lib._check(_lib.load().ssfm_device_sort_f64(0, _lib._VP(d.ptr), n), "ssfm_device_sort_f64")
    got = d.to_host()
    want = np.sort(x, kind="stable")
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("n,m", [(4096, 8192), (4096, 1000), (3000, 8191), (3001, 6000), (4097, 4097), (1 << 19, 1 << 20), (8192, 4096)])
def test_resample_is_scipy(n, m):
    x = np.random.default_rng(n + m).standard_normal(n)
    d = _lib.DeviceArray.from_host(x, np.float64)
    y = oa.devices._resample_device(d, m, 0).to_host()
    ref = sg.resample(x, m)
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12 * np.max(np.abs(ref)))


def test_sampler():
    gv(sps=4, R=1e9)
    dac = oa.DAC("010", pulse_shape="nrz", Vpp=1)
    for instant in (0, 2):
        np.testing.assert_allclose(oa.SAMPLER(dac, instant=instant).signal, [0, 1, 0], atol=1e-15)
    gv(sps=16, R=1e9)
    x = np.random.default_rng(3).standard_normal(16 * 37 + 5)
    nz = np.random.default_rng(4).standard_normal(x.size)
    for instant in (0, 7, 15, -3):
        s = oa.SAMPLER(electrical_signal(x, nz), instant)
        np.testing.assert_array_equal(s.signal, x[instant::16])
        np.testing.assert_array_equal(s.noise, nz[instant::16])


def test_example_link_end_to_end():
    """PRBS-11 -> DAC -> MZM(LASER) -> FIBER -> PD -> ook.DSP -> BER_analizer, all on the device; the bits and the error count equal the
    restatement's on the downloaded PD output."""
    gv(sps=32, R=10e9, N=2047)
    tx = oa.PRBS(order=11)
    Vpi = 5.0
    drive = oa.DAC(tx, Vpp=Vpi, offset=-Vpi / 2, pulse_shape="gaussian")
    field = oa.MZM(oa.LASER(P0=1), drive, bias=-Vpi / 2, Vpi=Vpi, loss_dB=3, ER_dB=20)
    pd = oa.PD(oa.FIBER(field, length=20, alpha=0.2, beta_2=-20, gamma=2), BW=0.75 * gv.R, r=1.0, include_noise="all", rng="device")
    rx, e, rth = ook.DSP(pd)
    ber = ook.BER_analizer("counter", Tx=tx, Rx=rx)
    assert isinstance(rx._raw(), _lib.DeviceArray)
    v = np.asarray(pd.signal + pd.noise)
    bits, r, rth_r = en.dsp(v, 32)
    assert_same_as_restatement(e, r)
    assert abs(rth - rth_r) <= 1e-12 * (r["mu1"] - r["mu0"])                         # a point of linspace(mu0, mu1, 1000)
    np.testing.assert_array_equal(rx.data, bits)
    assert ber == np.count_nonzero(bits != tx.data[: bits.size]) / bits.size
    assert 1e-4 < e.mu1 < 1e-1


def test_foreign_types():
    import foreign_types as ft
    x, sps, nslots, resamp = random_eye(7)
    ft.gv.set(sps, 1e9)
    gv(sps=4, R=1e9)                                                                  # our own gv deliberately different
    e = oa.GET_EYE(ft.electrical_signal(x), nslots=nslots, sps_resamp=resamp)
    r = en.get_eye(x, sps, nslots, resamp)
    assert_same_as_restatement(e, r)
    s = oa.SAMPLER(ft.electrical_signal(x), 3)
    assert type(s) is ft.electrical_signal
    np.testing.assert_array_equal(s.signal, x[3::sps])
    rx, e2, rth = ook.DSP(ft.electrical_signal(x))
    bits, r2, _ = en.dsp(x, sps)
    np.testing.assert_array_equal(rx.data, bits)
    e3 = oa.GET_EYE(x, nslots=nslots, sps_resamp=resamp, _grid=ft.gv)                # a NumPy array
    assert e3.t_opt == r["t_opt"] and e3.mu1 == e.mu1
