"""The PPM receiver on the MI355X (csrc/ppm.hip): opticomlib_amd.ppm against the reference's fixtures (tests/golden/ppm_*.npz) and, where the
reference's KMeans draws make the fixture unreachable, against the NumPy restatement tests/ppm_numpy.py."""
import numpy as np
import pytest

import opticomlib_amd as oa
import ppm_numpy as pn
from opticomlib_amd import _lib, ppm
from opticomlib_amd.typing import binary_sequence, electrical_signal, gv
from test_ppm_cpu import DSP_THR, load, ms

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def on_device(seq):
    return isinstance(seq._raw(), _lib.DeviceArray)


def dev_bits(a):
    return binary_sequence.from_device(_lib.DeviceArray.from_host(np.asarray(a, np.uint8), np.uint8, 0))


def signal(d, key=""):
    return electrical_signal(d["sig" + key], d["noise" + key])


def test_encoder_and_decoder_equal_the_fixtures_on_the_device():
    g = load("ppm_codec")
    for M in ms(g, "enc_"):
        enc = ppm.PPM_ENCODER(dev_bits(g[f"bits_{M}"]), M)
        assert on_device(enc)
        np.testing.assert_array_equal(enc.data, g[f"enc_{M}"], err_msg=str(M))
        dec = ppm.PPM_DECODER(dev_bits(g[f"dec_in_{M}"]), M)
        assert on_device(dec)
        np.testing.assert_array_equal(dec.data, g[f"dec_out_{M}"], err_msg=str(M))
        np.testing.assert_array_equal(ppm.PPM_DECODER(enc, M).data, g[f"bits_{M}"][: g[f"bits_{M}"].size // int(np.log2(M)) * int(np.log2(M))])


def test_the_reference_suite_cases_of_encoder_decoder_hdd_sdd():
    for inp in ("00011011", [0, 0, 0, 1, 1, 0, 1, 1], (0, 0, 0, 1, 1, 0, 1, 1), np.array([0, 0, 0, 1, 1, 0, 1, 1]), binary_sequence("00011011")):
        np.testing.assert_array_equal(ppm.PPM_ENCODER(inp, 4).data, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
        np.testing.assert_array_equal(ppm.PPM_ENCODER(inp, 256).data, np.insert(np.zeros(255), 27, 1))
    np.testing.assert_array_equal(ppm.PPM_DECODER("0100000100101000", 4).data, [0, 1, 1, 1, 1, 0, 0, 0])
    np.testing.assert_array_equal(ppm.PPM_DECODER(np.insert(np.zeros(127), 13, 1), 128).data, [0, 0, 0, 1, 1, 0, 1])
    assert ppm.PPM_DECODER("0000", 4).size == 0
    inputs = ["1010 0110 0000 0001", [1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
    for inp, m, total in ((inputs[0], 4, 4), (inputs[1], 8, 2), (np.array(inputs[1]), 16, 1)):
        assert ppm.HDD(inp, m).data.sum() == total
    with pytest.raises(ValueError):
        ppm.HDD("1010 0110 1", 4)
    x = np.kron([0.1, 1.2, 0.1, 0.2, 0.1, 0.9, 1.0, 1.1, 0.1, 0.1, 0.1, 0.2], np.ones(16))
    gv(sps=16, R=1e9)
    np.testing.assert_array_equal(ppm.SDD(x, 4).data, [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1])


def test_hdd_is_seed_for_seed_the_reference():
    g = load("ppm_hdd")
    for M in ms(g, "in_"):
        inp = g[f"in_{M}"].copy()
        np.random.seed(int(g[f"seed_{M}"]))
        out = ppm.HDD(dev_bits(inp), M)
        assert on_device(out)
        np.testing.assert_array_equal(out.data, g[f"out_{M}"], err_msg=str(M))
        np.random.seed(int(g[f"seed_{M}"]))
        np.testing.assert_array_equal(ppm.HDD(inp, M).data, g[f"out_{M}"])                # host input: uploaded
        np.testing.assert_array_equal(inp, g[f"in_{M}"])                                   # and not written


def test_sdd_and_soft_dsp_are_exact():
    g = load("ppm_sdd")
    for M in ms(g, "out_"):
        gv(sps=int(g[f"sps_{M}"]), R=1e9)
        out = ppm.SDD(electrical_signal(g[f"sig_{M}"], g[f"noise_{M}"]), M)
        assert on_device(out)
        np.testing.assert_array_equal(out.data, g[f"out_{M}"], err_msg=str(M))
    gv(sps=4, R=1e9)
    np.testing.assert_array_equal(ppm.SDD(g["ties_x"], 4).data, g["ties_out"])                 # first index on ties, NaN the maximum
    d = load("ppm_dsp_soft")
    gv(sps=int(d["sps"]), R=1e9)
    rx = ppm.DSP(signal(d), int(d["M"]), decision="soft")
    assert on_device(rx)
    np.testing.assert_array_equal(rx.data, d["rx"])
    with pytest.raises(TypeError):
        ppm.SDD(electrical_signal(g["ties_x"] + 0j), 4)


@pytest.mark.parametrize("name", DSP_THR)
def test_hard_dsp_with_a_given_threshold_is_seed_for_seed_exact(name):
    d = load(name)
    gv(sps=int(d["sps"]), R=1e9)
    np.random.seed(int(d["seed"]))
    rx = ppm.DSP(signal(d), int(d["M"]), decision="hard", threshold=float(d["rth"]))
    assert on_device(rx) and rx.rth == float(d["rth"])
    np.testing.assert_array_equal(rx.data, d["rx"])


def test_hard_dsp_with_an_estimated_threshold():
    d = load("ppm_dsp_hard_est")
    M, sps = int(d["M"]), int(d["sps"])
    gv(sps=sps, R=1e9)
    np.random.seed(int(d["seed"]))
    rx = ppm.DSP(signal(d), M, decision="hard")
    span = float(d["mu1"] - d["mu0"])
    assert abs(rx.rth - float(d["rth"])) <= span / 499 * (1 + 1e-9), (rx.rth, float(d["rth"]))     # one KDE grid step (test_eye_cpu)
    np.random.seed(int(d["seed"]))
    np.testing.assert_array_equal(rx.data, pn.dsp_hard(d["sig"] + d["noise"], M, sps, rx.rth))      # this GET_EYE takes no draws
    assert rx.eye_obj is not None


@pytest.mark.parametrize("rng", ["numpy", "device"])
def test_the_reference_link_decodes_without_errors(rng):
    gv(sps=64, R=1e9)
    M = 4
    bits = oa.PRBS(order=11)[:-1]
    x = oa.DAC(ppm.PPM_ENCODER(bits, M), pulse_shape="gaussian")
    np.random.seed(7)
    x = electrical_signal(np.real(np.asarray(x.signal)), np.random.normal(0, 0.05, x.size))
    for decision in ("soft", "hard"):
        rx = ppm.DSP(x, M, decision=decision, rng=rng)
        np.testing.assert_array_equal(rx.data, bits.data, err_msg=decision)
        assert ppm.BER_analizer("counter", Tx=bits, Rx=rx) == 0.0
    with pytest.raises(ValueError):
        ppm.DSP(x, M=5)
    with pytest.raises(ValueError):
        ppm.DSP(x, M=8, decision="hi")


def test_device_rng_gives_one_on_slot_repeatably_and_uniformly():
    M, nsym = 16, 100_000
    empty = np.zeros(nsym * M, np.uint8)
    full = np.ones(8 * nsym, np.uint8)                     # M = 8, every slot ON: keep one of 8
    oa.device_rng_seed(1234)
    a = ppm.HDD(dev_bits(empty), M, rng="device").data.reshape(-1, M)
    b = ppm.HDD(dev_bits(full), 8, rng="device").data.reshape(-1, 8)
    oa.device_rng_seed(1234)
    np.testing.assert_array_equal(ppm.HDD(dev_bits(empty), M, rng="device").data.reshape(-1, M), a)
    assert (a.sum(axis=1) == 1).all() and (b.sum(axis=1) == 1).all()
    for sym, m in ((a, M), (b, 8)):
        counts = np.bincount(sym.argmax(axis=1), minlength=m)
        e = nsym / m
        chi2 = ((counts - e) ** 2 / e).sum()
        assert chi2 < 3 * m, (chi2, counts)                # dof m - 1; a loose bound (P(chi2_15 > 48) ~ 2e-5)
    c = ppm.HDD(dev_bits(empty), M, rng="device").data.reshape(-1, M)
    assert (c != a).any()                                   # the next call takes the next stream


def test_sixteen_million_slots():
    M, sps = 256, 2
    nsym = (1 << 24) // M
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, nsym * 8).astype(np.uint8)
    slots = ppm.PPM_ENCODER(dev_bits(bits), M)
    gv(sps=sps, R=1e9)
    x = electrical_signal(np.repeat(slots.data, sps).astype(np.float64))     # 2^25 samples
    rx = ppm.DSP(x, M, decision="soft")
    assert rx.size == bits.size
    assert ppm.BER_analizer("counter", Tx=dev_bits(bits), Rx=rx) == 0.0
    rx = ppm.DSP(x, M, decision="hard", threshold=0.5, rng="device")
    assert ppm.BER_analizer("counter", Tx=dev_bits(bits), Rx=rx) == 0.0
