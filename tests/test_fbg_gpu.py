"""FBG on the MI355X (csrc/fbg.hip): H, step counts and filtered outputs against the reference's fixtures (tests/golden/fbg_*.npz), against
scipy.integrate.solve_ivp run here on the same ODE, and against the closed-form reflectivity of a uniform grating."""
import json

import numpy as np
import pytest
from scipy.integrate import solve_ivp

import opticomlib_amd as oa
from opticomlib_amd import _lib
from opticomlib_amd.typing import electrical_signal, gv, optical_signal
from test_fbg_cpu import C, load

pytestmark = pytest.mark.gpu

CASES = ["fbg_uniform_kl2", "fbg_uniform_kl16", "fbg_rcos", "fbg_gaussian", "fbg_parabolic", "fbg_chirped_rcos", "fbg_fc_dneff_n",
         "fbg_landa_kl_n", "fbg_landa_vdneff_l", "fbg_nofiltfilt", "fbg_npow2_3000"]


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def run_fixture(g, **extra):
    gv(fs=float(g["fs"]))
    noisy = g["noise"].size > 0
    x = optical_signal(g["signal"], g["noise"]) if noisy else optical_signal(g["signal"])
    return oa.FBG(x, print_params=False, retH=True, **json.loads(str(g["kwargs"])), **extra)


@pytest.mark.parametrize("name", CASES)
def test_H_steps_and_output_match_the_fixture(name):
    g = load(name)
    out, H = run_fixture(g)
    assert oa.FBG.last_steps == int(g["steps"]), (oa.FBG.last_steps, int(g["steps"]))
    assert oa.FBG.last_attempts == (int(g["nfev"]) - 2) // 6
    assert rel(H, g["H"]) < 1e-9
    assert rel(out.signal, g["out_signal"]) < 1e-9
    if g["noise"].size:
        assert rel(out.noise, g["out_noise"]) < 1e-9


def test_some_fixture_rejects_a_step():
    g = load("fbg_rcos")
    run_fixture(g)
    assert oa.FBG.last_attempts > oa.FBG.last_steps


def grating(n, fs, kL, F, apo, rng):
    """delta, s, k of a random grating (the reference's float64 expressions) and the apodization as a function of z."""
    gv(fs=fs)
    neff, lam_D = 1.45, C / gv.f0 * (1 + rng.uniform(-2e-5, 2e-5))
    vdneff = rng.uniform(3e-5, 2e-4)
    L = kL / (np.pi * vdneff / lam_D)
    w = np.fft.fftshift(np.fft.fftfreq(n, gv.dt) * 2 * np.pi)
    lam = 2 * np.pi * C / (w + 2 * np.pi * gv.f0)
    d = 2 * np.pi * neff * (1 / lam - 1 / lam_D) * L
    k = np.pi * vdneff / lam * L
    p = {"uniform": None, "gaussian": lambda z: np.exp(-4 * np.log(2) * (3 * z) ** 2), "parabolic": lambda z: 1 - (2 * z) ** 2}[apo]
    return dict(landa_D=lam_D, vdneff=vdneff, L=L), d, np.zeros(n), k, p


def scipy_H(d, s, k, F, p, rtol=1e-3, atol=1e-6, attempts=False):
    """(H, accepted steps) of solve_ivp(RK45, vectorized) on the coupled-mode equations of the arrays d, s, k; with ``attempts`` also
    the attempted steps ((nfev - 2) / 6: two evaluations for the initial step, six per attempt)."""
    n = d.size

    def rhs(z, y):
        R, S = y[:n], y[n:]
        kk, ss = (k * p(z), s * p(z)) if p else (k, s)
        sg = (d + ss - F * z)[:, None]
        kk = kk[:, None]
        return np.concatenate([1j * (sg * R + kk * S), -1j * (sg * S + kk * R)])
    y0 = np.concatenate([np.ones(n, complex), np.zeros(n, complex)])
    sol = solve_ivp(rhs, [0.5, -0.5], y0, method="RK45", vectorized=True, rtol=rtol, atol=atol)
    assert sol.status == 0, sol.message
    H, steps = sol.y[n:, -1] / sol.y[:n, -1], len(sol.t) - 1
    return (H, steps, (sol.nfev - 2) // 6) if attempts else (H, steps)


def test_random_gratings_match_scipy_solve_ivp():
    rng = np.random.default_rng(7)
    for trial in range(10):
        n = int(rng.choice([256, 1000, 2048, 4096]))
        kL, F, apo = float(rng.uniform(0.5, 12)), float(rng.choice([0.0, rng.uniform(-15, 15)])), str(rng.choice(["uniform", "gaussian", "parabolic"]))
        design, d, s, k, p = grating(n, float(rng.choice([50e9, 100e9, 200e9])), kL, F, apo, rng)
        x = optical_signal(np.ones(n, complex))
        _, H = oa.FBG(x, **design, F=F, apodization=apo, filtfilt=False, print_params=False, retH=True)
        Hs, steps = scipy_H(d, s, k, F, p)
        assert oa.FBG.last_steps == steps, (trial, oa.FBG.last_steps, steps)
        assert rel(H, Hs) < 1e-9, (trial, rel(H, Hs))


def test_uniform_grating_matches_the_closed_form():
    n = 4096
    gv(fs=100e9)
    for kL in (2.0, 16.0):
        x = optical_signal(np.ones(n, complex))
        _, H = oa.FBG(x, fc=gv.f0, vdneff=1e-4, kL=kL, filtfilt=False, print_params=False, retH=True, rtol=1e-10, atol=1e-12)
        lam_D = C / gv.f0
        L = kL / (np.pi * 1e-4 / lam_D)
        lam = 2 * np.pi * C / (x.w(shift=True) + 2 * np.pi * gv.f0)
        dl = 2 * np.pi * 1.45 * (1 / lam - 1 / lam_D) * L
        k = np.pi * 1e-4 / lam * L
        g = np.sqrt(k ** 2 - dl ** 2 + 0j)
        rho = -k * np.sinh(g) / (dl * np.sinh(g) + 1j * g * np.cosh(g))
        assert np.max(np.abs(H - rho)) < 1e-7, (kL, np.max(np.abs(H - rho)))


def test_custom_apodization_equals_the_built_in_and_waits_per_step():
    g = load("fbg_gaussian")
    out_b, H_b = run_fixture(g)
    steps, waits_b = oa.FBG.last_steps, oa.FBG.last_waits
    kw = json.loads(str(g["kwargs"]))
    kw["apodization"] = lambda z: np.exp(-4 * np.log(2) * (3 * z) ** 2)
    x = optical_signal(g["signal"])
    out_c, H_c = oa.FBG(x, print_params=False, retH=True, **kw)
    assert oa.FBG.last_steps == steps
    assert oa.FBG.last_waits >= oa.FBG.last_attempts > waits_b
    assert rel(H_c, H_b) < 1e-12 and rel(H_c, g["H"]) < 1e-9


def test_custom_apodization_error_propagates():
    gv(fs=100e9)

    def bad(z):
        raise RuntimeError("apodization failed")
    with pytest.raises(RuntimeError, match="apodization failed"):
        oa.FBG(optical_signal(np.ones(512, complex)), fc=gv.f0, vdneff=1e-4, kL=2, apodization=bad, print_params=False)


def test_the_reference_unit_tests():
    gv(sps=16, R=1e9)
    op = oa.LASER(P0=10)
    fbg = oa.FBG(op, fc=gv.f0, vdneff=1e-4, kL=2)
    assert isinstance(fbg, optical_signal) and fbg.size == op.size
    pm = oa.PM(op, el_input=0, Vpi=5)
    np.testing.assert_allclose(pm.signal, op.signal)
    pm = oa.PM(op, el_input=5, Vpi=5)
    np.testing.assert_allclose(pm.signal, op.signal * np.exp(1j * np.pi))
    t = np.linspace(0, 1, 100)
    adc = oa.ADC(electrical_signal(np.sin(2 * np.pi * t)), n=2, otype="n")
    assert np.unique(adc.signal).size <= 4 and adc.signal.min() >= 0 and adc.signal.max() <= 3


def test_outputs_stay_on_the_device_and_dual_polarisation_rows_share_H():
    g = load("fbg_uniform_kl2")
    gv(fs=float(g["fs"]))
    x = oa.DM(optical_signal(g["signal"], g["noise"]), D=0.0)              # a device-resident input
    assert isinstance(x._raw("signal"), _lib.DeviceArray)
    out = oa.FBG(x, print_params=False, **json.loads(str(g["kwargs"])))
    assert isinstance(out._raw("signal"), _lib.DeviceArray) and isinstance(out._raw("noise"), _lib.DeviceArray)
    assert out.execution_time > 0
    two = np.stack([g["signal"], g["signal"][::-1]])
    out2 = oa.FBG(optical_signal(two), print_params=False, **json.loads(str(g["kwargs"])))
    one_b = oa.FBG(optical_signal(g["signal"][::-1].copy()), print_params=False, **json.loads(str(g["kwargs"])))
    assert out2.shape == (2, g["signal"].size)
    assert rel(out2.signal[0], g["out_signal"]) < 1e-9
    assert rel(out2.signal[1], one_b.signal) < 1e-12
