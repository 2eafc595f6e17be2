"""PM and ADC on the MI355X against the reference's fixtures (tests/golden/pm_cases.npz, adc_cases.npz)."""
import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib
from opticomlib_amd.typing import electrical_signal, gv, optical_signal
from test_fbg_cpu import load

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_pm_matches_the_fixture():
    g = load("pm_cases")
    gv(sps=16, R=10e9)
    out = oa.PM(optical_signal(g["signal"], g["noise"]), electrical_signal(g["v"], g["vn"]), Vpi=3.3)
    assert isinstance(out._raw("signal"), _lib.DeviceArray)
    assert rel(out.signal, g["out_signal"]) < 1e-14 and rel(out.noise, g["out_noise"]) < 1e-14
    assert rel(oa.PM(optical_signal(g["signal"]), 2.5, Vpi=5).signal, g["out_scalar"]) < 1e-14
    out2 = oa.PM(optical_signal(g["signal2"]), g["v"], Vpi=4.0)
    assert out2.shape == g["signal2"].shape and rel(out2.signal, g["out2"]) < 1e-14
    with pytest.raises(TypeError, match="`op_input` must be of type 'optical_signal'."):
        oa.PM(g["signal"], 1.0)


def test_pm_takes_a_device_drive():
    g = load("pm_cases")
    gv(sps=16, R=10e9)
    v = electrical_signal.from_device(_lib.DeviceArray.from_host(g["v"], np.float64, 0), _lib.DeviceArray.from_host(g["vn"], np.float64, 0))
    out = oa.PM(optical_signal(g["signal"], g["noise"]), v, Vpi=3.3)
    assert rel(out.signal, g["out_signal"]) < 1e-14


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("tag", ["nofs", "fs"])
@pytest.mark.parametrize("otype", ["n", "v"])
def test_adc_matches_the_fixture(bits, tag, otype):
    g = load("adc_cases")
    gv(sps=16, R=10e9)
    fs = None if tag == "nofs" else float(g["fs"]) / 2
    x = electrical_signal(g["signal"], g["noise"])
    out = oa.ADC(x, fs=fs, n=bits, otype=otype)
    assert isinstance(out._raw("signal"), _lib.DeviceArray)
    want = g[f"n{bits}_{tag}_{otype}"]
    got = out.signal
    if otype == "n":
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.max(np.abs(want)))


def test_adc_otype_error():
    with pytest.raises(ValueError, match="`otype` must be 'v' or 'n'."):
        oa.ADC(electrical_signal(np.arange(10.0)), otype="x")
