"""The OOK receiver without a GPU: the NumPy restatement (tests/eye_numpy.py) against the reference's fixtures (tests/golden/eye_*.npz),
the host-scalar parts of opticomlib_amd.ook, and the new entry points of the C ABI.

Tolerances against the fixtures: exact on t_left / t_right / t_opt / i, the received bits and the error count; 1e-9 of mu1 - mu0 on the
moments; one grid step on threshold and rth.  The reference's KMeans (sklearn, tol = 1e-4 of the variance) stops short of the two-means'
fixed point that the deterministic Lloyd reaches (with tol = 0 sklearn lands on it exactly): the split vm, and with it top_int / bot_int,
moves by up to about 1e-4 of the eye's height (bound: 3e-4), and y_left / y_right (snapped to the dense set of sample values) by up to 1e-3 of it.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

import eye_numpy as en

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "eye_*.npz")))
GOLDEN_DSP = [p for p in GOLDEN if os.path.basename(p).startswith("eye_dsp_")]
NEW_SYMBOLS = ("ssfm_device_sort_f64", "ssfm_eye_prepare", "ssfm_eye_resample_stage", "ssfm_eye_estimate", "ssfm_eye_levels", "ssfm_device_sample",
               "ssfm_device_count_diff")


def load_case(path):
    g = dict(np.load(path))
    g["what"], g["sps"] = str(g["what"]), int(g["sps"])
    g["nslots"], g["sps_resamp"] = int(g["nslots"]), (None if int(g["sps_resamp"]) < 0 else int(g["sps_resamp"]))
    return g


def check_eye(e, g):
    """e: the attributes (dict or eye object) under test; g: a fixture."""
    get = (lambda k: e[k]) if isinstance(e, dict) else (lambda k: getattr(e, k))
    span = float(g["mu1"] - g["mu0"])
    for k in ("t_left", "t_right", "t_opt", "i"):
        assert get(k) == g[k], (k, get(k), g[k])
    for k in ("y_left", "y_right"):
        v = get(k)
        if np.isnan(g[k]):
            assert v is None, (k, v)
        else:                                           # within 2e-3 of the span: see the module docstring
            assert abs(v - g[k]) <= 2e-3 * span, (k, v, g[k])
    for k in ("mu0", "mu1", "s0", "s1"):
        assert abs(get(k) - g[k]) <= 1e-9 * span, (k, get(k), g[k])
    for k in ("top_int", "bot_int"):
        np.testing.assert_allclose(np.ravel(get(k)), g[k], rtol=0, atol=3e-4 * span, err_msg=k)
    th = get("threshold")
    if np.isnan(g["threshold"]):
        assert th is None
    else:
        assert abs(th - g["threshold"]) <= span / 499 * (1 + 1e-9), (th, g["threshold"])


def restated(g):
    x = g["x_filt"] if "x_filt" in g else g["x"]
    if g["what"] == "eye":
        return en.get_eye(x, g["sps"], g["nslots"], g["sps_resamp"]), None, None
    bits, e, rth = en.dsp(x, g["sps"])
    return e, bits, rth


def test_the_fixtures_cover_the_cases():
    names = {os.path.basename(p)[:-4] for p in GOLDEN}
    assert len(names) >= 9 and len(GOLDEN_DSP) >= 3
    cases = [load_case(p) for p in GOLDEN]
    assert {g["sps"] for g in cases} >= {16, 64} and {g["sps_resamp"] for g in cases} >= {None, 128}
    assert any(g["x"].size & (g["x"].size - 1) for g in cases)                         # not a power of two
    assert any(g["what"] == "eye" and g["x"].size // g["sps"] < g["nslots"] for g in cases)
    assert any("x_filt" in g for g in cases) and any(g["what"] == "dsp" and "x_filt" not in g for g in cases)
    assert any(g["what"] == "link" and 1e-4 < g["mu1"] < 1e-1 for g in cases)           # PD currents
    assert any(np.isnan(g["y_left"]) for g in cases)                                     # the fallback branch


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_reproduces_the_reference(path):
    g = load_case(path)
    e, bits, rth = restated(g)
    check_eye(e, g)
    if bits is not None:
        span = float(g["mu1"] - g["mu0"])
        assert abs(rth - g["rth"]) <= span / 999 * (1 + 1e-9)
        np.testing.assert_array_equal(bits, g["rx"])
        n = bits.size
        assert np.count_nonzero(g["tx"][:n] != bits) / n == g["ber_counter"]


@pytest.mark.parametrize("path", GOLDEN_DSP, ids=lambda p: os.path.basename(p)[:-4])
def test_threshold_and_estimator_match_the_reference(path):
    from opticomlib_amd import ook
    from opticomlib_amd.typing import eye
    g = load_case(path)
    e = eye(mu0=float(g["mu0"]), mu1=float(g["mu1"]), s0=float(g["s0"]), s1=float(g["s1"]))
    assert ook.THRESHOLD_EST(e) == g["rth"]
    np.testing.assert_allclose(ook.BER_analizer("estimator", eye_obj=e), g["ber_estimator"], rtol=1e-12, atol=0)


def test_threshold_est_cases_of_the_reference_suite():
    from opticomlib_amd import ook

    class MockEye:
        def __init__(self, mu0, mu1, s0, s1):
            self.mu0, self.mu1, self.s0, self.s1 = mu0, mu1, s0, s1

    assert abs(ook.THRESHOLD_EST(MockEye(0, 1, 0.1, 0.1)) - 0.5) <= 0.01
    th = ook.THRESHOLD_EST(MockEye(0, 1, 0.1, 0.2))
    assert 0.0 < th < 0.5
    with pytest.raises(TypeError):
        ook.BER_analizer("nonsense")


def test_the_receiver_is_exported():
    import opticomlib_amd as oa
    from opticomlib_amd import GET_EYE, SAMPLER, ook  # noqa: F401
    assert {"GET_EYE", "SAMPLER", "ook", "eye"} <= set(oa.__all__)
    assert callable(ook.DSP) and callable(ook.BER_analizer) and callable(ook.THRESHOLD_EST)


def test_the_new_entry_points_are_declared_bound_and_exported():
    from opticomlib_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and s in _lib.SYMBOLS and s in names, s
    assert "#define SSFM_ABI_VERSION 3" in hdr


def test_restatement_building_blocks():
    x = np.array([0.0, 1.0, 1.0 + 5e-11, 2.0, 3.0, 3.0 + 5e-11])
    # diffs at lag 3: [2, 2, 2 - 5e-11]: all within 1e-10 of the minimum -> int(mean([0, 1, 2])) = 1
    np.testing.assert_array_equal(en.shortest_int(x), [1.0, 3.0])
    with pytest.raises(ValueError):
        en.shortest_int(np.array([1.0]))
    assert en.find_nearest(np.array([0.0, 1.0, 2.0]), 0.5) == 0.0                       # ties to the lower value
    c = en.two_means_1d(np.r_[np.zeros(10), np.ones(10)])
    np.testing.assert_array_equal(c, [0.0, 1.0])


def test_restatement_counts_its_lloyd_updates():
    # (0, 10) -> (1, 10): one update, then the step that finds the centres unchanged
    c, u = en.two_means_1d(np.array([0.0, 1.0, 2.0, 10.0]), updates=True)
    np.testing.assert_array_equal(c, [1.0, 10.0])
    assert u == 1
    c, u = en.two_means_1d(np.r_[np.zeros(10), np.ones(10)], updates=True)
    assert u == 0
    x = np.random.default_rng(0).exponential(1.0, 1 << 20)                 # far outliers: many small moves of the upper centre
    c, u = en.two_means_1d(x, updates=True)
    np.testing.assert_array_equal(c, en.two_means_1d(x))
    assert u > 24
    t = np.tile(np.linspace(-1, 1, 8, endpoint=False), 4)
    cc, u2 = en.two_means_2d(t, np.arange(t.size, dtype=float), updates=True)
    np.testing.assert_array_equal(cc, en.two_means_2d(t, np.arange(t.size, dtype=float)))
    assert u2 >= 1


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("resamp", [None, 32])
def test_restatement_refuses_non_finite_samples(bad, resamp):
    x = np.tile(np.r_[np.zeros(16), np.ones(16)], 32)
    x[7] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        en.get_eye(x, 16, 64, resamp)
    x[7] = 0.0
    assert en.get_eye(x, 16, 64, resamp)["_updates1"] >= 0                 # a finite signal goes through
