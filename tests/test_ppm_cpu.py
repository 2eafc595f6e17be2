"""The PPM receiver without a GPU: the NumPy restatement tests/ppm_numpy.py against the reference's fixtures (tests/golden/ppm_*.npz, written
by make_golden_ppm.py) -- HDD's draw order bit for bit -- the host scalars of opticomlib_amd.ppm / ook against the reference's values, and the
new entry points of the C ABI."""
import os
import subprocess

import numpy as np
import pytest

import ppm_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("ssfm_ppm_encode", "ssfm_ppm_decode", "ssfm_ppm_decide", "ssfm_ppm_faulty", "ssfm_ppm_resolve")
DSP_THR = ("ppm_dsp_hard_thr", "ppm_dsp_hard_thr_m64")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def ms(g, prefix):
    return sorted(int(k[len(prefix):]) for k in g if k.startswith(prefix))


def test_restatement_reproduces_the_codec_fixtures():
    g = load("ppm_codec")
    for M in ms(g, "enc_"):
        np.testing.assert_array_equal(pn.encode(g[f"bits_{M}"], M), g[f"enc_{M}"], err_msg=str(M))
        np.testing.assert_array_equal(pn.decode(g[f"dec_in_{M}"], M), g[f"dec_out_{M}"], err_msg=str(M))
        s = g[f"dec_in_{M}"].reshape(-1, M).sum(axis=1)
        assert (s == 0).any() and (s > 1).any()                              # the decoder cases hold empty and double symbols


def test_restatement_reproduces_every_hdd_fixture_bit_for_bit():
    g = load("ppm_hdd")
    for M in ms(g, "in_"):
        cnt = g[f"in_{M}"].reshape(-1, M).sum(axis=1)
        assert (cnt == 0).sum() >= 10 and (cnt > 1).sum() >= 10, M            # many faulty symbols of both kinds
        np.random.seed(int(g[f"seed_{M}"]))
        np.testing.assert_array_equal(pn.hdd(g[f"in_{M}"], M), g[f"out_{M}"], err_msg=str(M))
        assert (g[f"out_{M}"].reshape(-1, M).sum(axis=1) == 1).all()


def test_restatement_reproduces_sdd_and_the_given_threshold_dsp():
    g = load("ppm_sdd")
    for M in ms(g, "out_"):
        np.testing.assert_array_equal(pn.sdd(g[f"sig_{M}"] + g[f"noise_{M}"], M, int(g[f"sps_{M}"])), g[f"out_{M}"], err_msg=str(M))
    np.testing.assert_array_equal(pn.sdd(g["ties_x"], 4, 4), g["ties_out"])
    d = load("ppm_dsp_soft")
    M, sps = int(d["M"]), int(d["sps"])
    np.testing.assert_array_equal(pn.decode(pn.sdd(d["sig"] + d["noise"], M, sps), M), d["rx"])
    for name in DSP_THR:
        d = load(name)
        np.random.seed(int(d["seed"]))
        np.testing.assert_array_equal(pn.dsp_hard(d["sig"] + d["noise"], int(d["M"]), int(d["sps"]), float(d["rth"])), d["rx"], err_msg=name)


def test_estimated_threshold_fixture_is_consistent():
    d = load("ppm_dsp_hard_est")
    from opticomlib_amd import ppm
    from opticomlib_amd.typing import eye
    e = eye(mu0=float(d["mu0"]), mu1=float(d["mu1"]), s0=float(d["s0"]), s1=float(d["s1"]))
    rth = float(d["threshold"]) if not np.isnan(d["threshold"]) else ppm.THRESHOLD_EST(e, int(d["M"]))
    assert rth == float(d["rth"])
    np.testing.assert_array_equal(pn.slot_samples(d["sig"] + d["noise"], int(d["sps"])) > d["rth"], d["decisions"].astype(bool))


def test_threshold_est_values_of_the_reference_suite():
    from opticomlib_amd import ppm
    from opticomlib_amd.typing import eye
    mu0, mu1, s = [0.1, 0.2, 0.3, 0.4], [0.9, 1.0, 1.1, 1.2], [0.1, 0.2, 0.3, 0.4]
    out = [0.514014014014014, 0.6532532532532533, 0.8085085085085084, 0.9693693693693693]
    for i in range(4):
        assert ppm.THRESHOLD_EST(eye(mu0=mu0[i], mu1=mu1[i], s0=s[i], s1=s[i]), 4) == out[i]
    with pytest.raises(ValueError):
        ppm.THRESHOLD_EST(eye(mu0=0.1, mu1=0.9, s0=0.1, s1=0.1), 5)
    with pytest.raises(TypeError):
        ppm.THRESHOLD_EST({"mu0": 0.1}, 4)


def test_theory_ber_values_of_the_reference_docstrings():
    from opticomlib_amd import ook, ppm
    assert ppm.theory_BER(mu1=1, s0=0.1, s1=0.1, M=8, decision="hard") == 8.515885763544466e-07
    assert ppm.theory_BER(mu1=1, s0=0.1, s1=0.1, M=8, decision="soft") == 3.074810247686141e-12
    assert ook.theory_BER(mu1=1, s0=0.1, s1=0.1) == 2.8674468224390994e-07
    assert ppm.theory_BER(1, 0.1, 0.1, 4, "hard") < 1e-6
    assert ppm.theory_BER(1, 0.1, 0.1, 4, "soft") < 1e-11
    assert ppm.theory_BER(1, 0.1, 0.1, 4, "hard") > ppm.theory_BER(1, 0.1, 0.1, 4, "soft")
    assert (ppm.theory_BER([1, 1], [0.1, 0.1], [0.1, 0.1], 4, "hard") < 1e-6).all()
    with pytest.raises(ValueError):
        ppm.theory_BER(1, 0.1, 0.1, 5, "hard")
    with pytest.raises(ValueError):
        ppm.theory_BER(1, 0.1, 0.1, 4, "medium")


def test_estimator_and_theory_match_the_fixtures():
    from opticomlib_amd import ook, ppm
    from opticomlib_amd.typing import eye
    g = load("ppm_ber")
    for a, decision in enumerate(("hard", "soft")):
        for i, (mu0, mu1, s0, s1) in enumerate(g["eyes"]):
            for j, M in enumerate(g["Ms"]):
                v = ppm.BER_analizer("estimator", eye_obj=eye(mu0=mu0, mu1=mu1, s0=s0, s1=s1), M=int(M), decision=decision)
                np.testing.assert_allclose(v, g["estimator"][a, i, j], rtol=1e-12, atol=0)
        for j, M in enumerate(g["Ms"]):
            np.testing.assert_allclose(ppm.theory_BER(g["mu1"], g["s"], 1.3 * g["s"], int(M), decision), g["theory"][a, j], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ook.theory_BER(g["mu1"], g["s"], 1.3 * g["s"]), g["theory_ook"], rtol=1e-12, atol=0)


def test_ber_analizer_exceptions_of_the_reference_suite():
    from opticomlib_amd import ppm
    from opticomlib_amd.typing import eye
    e = eye(mu0=0.0, mu1=1.0, s0=0.1, s1=0.1)
    with pytest.raises(ValueError):
        ppm.BER_analizer(mode="hi")
    with pytest.raises(KeyError):
        ppm.BER_analizer("counter")
    with pytest.raises(KeyError):
        ppm.BER_analizer("estimator")
    with pytest.raises(ValueError):
        ppm.BER_analizer("estimator", eye_obj=e, M=5)
    with pytest.raises(ValueError):
        ppm.BER_analizer("estimator", eye_obj=e, M=4, decision="hi")
    assert ppm.BER_analizer("estimator", eye_obj=e, M=4) < 1e-11


def test_argument_errors_come_before_any_device_work():
    from opticomlib_amd import ppm
    with pytest.raises(TypeError):
        ppm.DSP(input=2, M=5)
    with pytest.raises(ValueError):
        ppm.DSP(input=[1, 2, 3], M=5)
    with pytest.raises(ValueError):
        ppm.SDD(np.zeros(64), 5)
    with pytest.raises(TypeError):
        ppm.PPM_ENCODER(3.5, 4)
    with pytest.raises(TypeError):
        ppm.HDD({1, 0}, 4)
    with pytest.raises(ValueError):
        ppm.HDD(binary_sequence_of("1010 0110"), 3)
    with pytest.raises(ValueError):
        ppm.HDD(np.array([], dtype=np.uint8), 3)


def binary_sequence_of(s):
    from opticomlib_amd.typing import binary_sequence
    return binary_sequence(s)


def test_the_receiver_is_exported():
    import opticomlib_amd as oa
    from opticomlib_amd import ppm
    assert "ppm" in oa.__all__
    assert set(ppm.__all__) == {"PPM_ENCODER", "PPM_DECODER", "HDD", "SDD", "THRESHOLD_EST", "DSP", "BER_analizer", "theory_BER"}
    assert callable(oa.ook.theory_BER)


def test_the_new_entry_points_are_declared_bound_and_exported():
    from opticomlib_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and s in _lib.SYMBOLS and s in names, s
    assert "#define SSFM_ABI_VERSION 3" in hdr
    assert "ppm.hip" in open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()


def test_philox_restatement_known_answers():
    # Random123's published known-answer vectors for philox4x32_10 (the generator of ppm.HDD's rng="device")
    assert [int(w) for w in pn.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(w) for w in pn.philox4x32_10(f, f, f, f, f, f)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
