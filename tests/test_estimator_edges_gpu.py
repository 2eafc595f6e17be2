"""The two chains of one-workgroup folds driven by a host loop, at their size limits and edges: GET_EYE's estimator (csrc/eye.hip
ssfm_eye_estimate / ssfm_eye_levels) against the float64 restatement tests/eye_numpy.py, and FBG's coupled-mode solve (csrc/fbg.hip
ssfm_fbg_solve / ssfm_fbg_delay) against scipy.integrate.solve_ivp and NumPy on the same arrays."""
import math

import numpy as np
import pytest

import eye_numpy as en
import opticomlib_amd as oa
from opticomlib_amd import _lib, ook
from opticomlib_amd.typing import electrical_signal, gv, optical_signal
from test_eye_gpu import DISCRETE, assert_same_as_restatement, random_eye
from test_fbg_gpu import scipy_H

pytestmark = pytest.mark.gpu

EYE_MAX = 1 << 21                 # devices._EYE_MAX_N
RED_REACH = 480 * 256             # eye.hip kRedBlocks * kThreads: one grid-stride pass of a reduction
CHUNK = 24                        # eye.hip kLloydChunk
LLOYD_MAX = 300


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


# ------------------------------------------------------------------------------------------------ GET_EYE
def assert_same(e, r, moment_scale=None):
    """assert_same_as_restatement, NaN-aware (an empty centre window gives NaN moments and no threshold on both sides).
    ``moment_scale``: the magnitude the moments' rounding scales with, when it is much larger than the eye's span (an offset eye)."""
    span = r["mu1"] - r["mu0"]
    if np.isfinite(span) and moment_scale is None:
        assert_same_as_restatement(e, r)
    else:
        span = span if np.isfinite(span) else 0.0                                     # one moment is NaN: the other must be equal
        for k in DISCRETE:
            assert getattr(e, k) == r[k], (k, getattr(e, k), r[k])
        for k in ("mu0", "mu1", "s0", "s1"):
            a, b = getattr(e, k), r[k]
            if np.isnan(b):
                assert np.isnan(a), (k, a)
            else:                                                   # 64 ulp of the level: the sums run in another order than NumPy's
                assert abs(a - b) <= 1e-12 * abs(span) + 64 * np.finfo(float).eps * (moment_scale or 0.0), (k, a, b)
        for k in ("top_int", "bot_int"):
            np.testing.assert_array_equal(getattr(e, k), r[k], err_msg=k)
        if r["threshold"] is None:
            assert e.threshold is None
        else:
            assert abs(e.threshold - r["threshold"]) <= abs(span) / 499 * (1 + 1e-9)
    assert e._y_center == r["y_center"]


def nrz(bits, sps, lo=0.0, hi=1.0, width=0.25, noise=0.0, rng=None):
    """Levels lo / hi, Gaussian-smoothed edges (``width`` in slots; 0: rectangular), Gaussian noise of ``noise`` times the swing."""
    x = np.repeat(np.asarray(bits, float), sps)
    if width:
        k = np.arange(-3 * sps, 3 * sps + 1)
        h = np.exp(-0.5 * (k / (width * sps)) ** 2)
        x = np.convolve(x, h / h.sum(), mode="same")
    if noise:
        x = x + rng.normal(0, noise, x.size)
    return lo + (hi - lo) * x


def eye_case(x, sps, nslots, resamp=None, **kw):
    gv(sps=sps, R=1e9)
    r = en.get_eye(x, sps, nslots, resamp)
    e = oa.GET_EYE(x, nslots=nslots, sps_resamp=resamp)
    assert_same(e, r, **kw)
    return e, r


@pytest.mark.parametrize("sps,resamp", [(256, None), (16, 256)], ids=["plain", "resampled"])
def test_eye_at_the_cap(sps, resamp):
    """2^21 samples exactly: 8192 slots at 256 samples, before or after the resampling."""
    rng = np.random.default_rng(sps)
    x = nrz(rng.integers(0, 2, 8192), sps, noise=0.08, rng=rng)
    e, r = eye_case(x, sps, 8192, resamp)
    assert e.y.size == EYE_MAX
    np.testing.assert_allclose(e.y, r["y"], rtol=0, atol=1e-12 * np.max(np.abs(r["y"])))


@pytest.mark.parametrize("sps,resamp", [(256, None), (16, 256)], ids=["plain", "resampled"])
def test_eye_one_pair_of_slots_beyond_the_cap_is_refused(sps, resamp):
    """8194 slots (the slot count must be even): 2^21 + 2 sps samples before, or 2^21 + 512 after, the resampling."""
    gv(sps=sps, R=1e9)
    x = nrz(np.random.default_rng(1).integers(0, 2, 8194), sps)
    with pytest.raises(ValueError, match=r"2\^21"):
        oa.GET_EYE(x, nslots=8194, sps_resamp=resamp)


@pytest.mark.parametrize("sps,nslots", [(16, 7678), (16, 7680), (16, 7682), (64, 1918), (64, 1920), (64, 1922), (2, 61438), (2, 61442)])
def test_eye_around_the_reach_of_one_reduction_pass(sps, nslots):
    """Lengths just below, at and just above kRedBlocks * kThreads = 122 880 samples, where the grid-stride loops take a second lap."""
    assert abs(sps * nslots - RED_REACH) <= 2 * sps
    rng = np.random.default_rng(nslots)
    x = nrz(rng.integers(0, 2, nslots), sps, noise=0.1, rng=rng)
    eye_case(x, sps, nslots)


def test_eye_smallest_call():
    """sps 2 and 2 slots: four samples."""
    x = np.array([0.0, 0.1, 1.0, 0.9])
    e, r = eye_case(x, 2, 2)
    assert e.y.size == 4


# --- the host loop of 24-step Lloyd chunks
def heavy_noise(kind, seed, amp, scale, sps=128, nslots=8192):
    """2^20 samples: an NRZ eye of amplitude ``amp`` (0: noise alone) plus heavy-tailed noise, whose two-means start from far outliers."""
    rng = np.random.default_rng(seed)
    x = nrz(rng.integers(0, 2, nslots), sps) * amp
    nz = rng.standard_t(3.0, x.size) if kind == "t3" else rng.exponential(1.0, x.size)
    return x + scale * nz


def chunks(updates):
    """Lloyd launches until the flag is set: one per update, plus the step that finds the centres unchanged (none at the cap of 300),
    in chunks of 24 with one look at the state after each."""
    return math.ceil(min(updates + 1, LLOYD_MAX) / CHUNK)


@pytest.mark.parametrize("case,need1,need2", [(("t3", 0, 0.0, 0.05), 48, 0), (("exp", 1, 0.0, 3.0), 24, 48)], ids=["1d-3-chunks", "2d-3-chunks"])
def test_round_trips_follow_the_lloyd_updates(case, need1, need2):
    """round_trips = 1 (prepare) [+ 5 (resampling)] + 2 (t-grid upload, first state read) + (chunks1 - 1) + (chunks2 - 1) + 1 (levels):
    every extra chunk of the 1-D two-means re-launches the stages after it and the first 2-D chunk, every extra 2-D chunk only the 2-D."""
    x = heavy_noise(*case)
    gv(sps=128, R=1e9)
    r = en.get_eye(x, 128, 8192)
    u1, u2 = r["_updates1"], r["_updates2"]
    assert u1 > need1 and u2 >= need2, (u1, u2)
    d = oa.devices._wrap_out(electrical_signal, _lib.DeviceArray.from_host(x, np.float64), oa.NULL)
    e = oa.GET_EYE(d, 8192)
    assert_same(e, r)
    assert e.round_trips == 1 + 2 + (chunks(u1) - 1) + (chunks(u2) - 1) + 1, (e.round_trips, u1, u2)


# --- degenerate eyes
def test_noise_free_two_level_eye_has_an_empty_band():
    rng = np.random.default_rng(5)
    x = nrz(rng.integers(0, 2, 600), 16, width=0)
    e, r = eye_case(x, 16, 600)
    assert r["y_left"] is None and e.y_left is None and e.t_opt == 0.0


def test_three_level_eye():
    rng = np.random.default_rng(6)
    x = nrz(rng.integers(0, 3, 900) / 2, 32, noise=0.03, rng=rng)
    eye_case(x, 32, 900)
    eye_case(x, 32, 900, 64)


def test_constant_signal_is_refused_on_both_sides():
    gv(sps=16, R=1e9)
    x = np.full(16 * 64, 0.25)
    with pytest.raises(ValueError):
        en.get_eye(x, 16, 64)
    with pytest.raises(ValueError):
        oa.GET_EYE(x, nslots=64)


def test_band_at_a_single_phase_gives_nan_moments_and_no_threshold():
    """Noise-free levels 0 and 1, and a 0.5 at one phase of some slots: the band's points share one t, both 2-D centres sit on it,
    t_dist = 0 and the centre window is empty."""
    sps, nslots = 16, 400
    rng = np.random.default_rng(8)
    x = nrz(rng.integers(0, 2, nslots), sps, width=0)
    x[5::sps * 2][: nslots // 4] = 0.5                                               # one phase of every other slot, in a quarter of them
    e, r = eye_case(x, sps, nslots)
    assert r["t_dist"] == 0 and e.t_dist == 0
    assert np.isnan(r["mu0"]) and np.isnan(e.mu0) and np.isnan(e.mu1)
    assert r["threshold"] is None and e.threshold is None


@pytest.mark.parametrize("lo,hi", [(1e6, 1e6 + 1e-3), (-3.0, -1.0)], ids=["offset-1e6", "negative"])
def test_offset_and_negative_eyes(lo, hi):
    """Cancellation in the moments (two-pass) and in the KDE's whitening; the threshold keeps the one-grid-step bound."""
    rng = np.random.default_rng(9)
    x = nrz(rng.integers(0, 2, 2000), 32, lo=lo, hi=hi, noise=0.06, rng=rng)
    eye_case(x, 32, 2000, moment_scale=max(abs(lo), abs(hi)))


# --- ties
def test_samples_at_the_1d_midpoint_join_cluster_0():
    """Noise-free slots at 0, 1 and 2 (30 / 40 / 30 %): every 1 lies exactly at (0 + 2) / 2, the midpoint of the first centres
    (min, max).  Ties to cluster 0 give centres (0.57, 2), vm > 1 and the 1s in the lower half, which they dominate: bot_int = (1, 1),
    y_center 1, mu0 = 0.  Ties to cluster 1 would give centres (0, 1.44), the 1s in the upper half: top_int = (1, 1), bot_int = (0, 0),
    y_center 0, and an empty bottom cluster (mu0 NaN, no threshold)."""
    rng = np.random.default_rng(10)
    x = np.repeat(rng.choice([0.0, 1.0, 2.0], 512, p=[0.3, 0.4, 0.3]), 16)
    e, r = eye_case(x, 16, 512)
    np.testing.assert_array_equal(e.bot_int, [1.0, 1.0])
    np.testing.assert_array_equal(e.top_int, [2.0, 2.0])
    assert e._y_center == 1.0 and e.mu0 == 0.0 and e.threshold is not None


def test_y_center_tie_is_resolved_by_the_fold_to_the_lower_value():
    """Levels 0 and 1 (y_center target 0.5) and one sample each of 0.75 and 0.25: equidistant members of the pre-resample set, placed in
    the ranges of workgroups 0 and 1 of the nearest-value reduction, so that only the fold of the partials sees the tie."""
    sps, nslots = 16, 512
    rng = np.random.default_rng(11)
    x = nrz(rng.integers(0, 2, nslots), sps, width=0)
    shift = -sps // 2 + 1                                                            # x0 = np.roll(x, shift): x0[i] = x[(i - shift) % n]
    x[(10 - shift) % x.size] = 0.75
    x[(300 - shift) % x.size] = 0.25
    e, r = eye_case(x, sps, nslots)
    assert r["y_center"] == 0.25 and e._y_center == 0.25


def test_signed_zeros_in_the_value_set():
    """Levels -1 and +1 and a few samples of +0.0 and -0.0: the y_center target is 0 and the band is the zeros, so y_center and y_left
    are a zero of the set (the sign NumPy's unsorted-stable np.unique keeps is not part of the comparison)."""
    rng = np.random.default_rng(12)
    x = nrz(rng.integers(0, 2, 512), 16, lo=-1.0, hi=1.0, width=0)
    pos = rng.choice(x.size, 80, replace=False)
    x[pos[:40]] = 0.0
    x[pos[40:]] = -0.0
    e, r = eye_case(x, 16, 512)
    assert e._y_center == 0.0 and e.y_left == 0.0


def test_integer_samples_make_kde_plateaus_and_the_first_argmin_wins():
    """Integer levels with rare ones: the KDE underflows to exactly 0 over a run of grid points, and the first of them is the threshold.
    Where the run starts is decided by which kernels underflow to 0 and which to a subnormal, and there scipy's gaussian_kde (another
    formula) and the device part by a couple of grid points; so the run is located with the device's formula restated in NumPy:
    sum_j exp(-(y_j / h - x / h)^2 / 2) over the central samples, h = sqrt(var, ddof 1) nc^(-1/5).  A sum of non-negative terms is 0 in
    any order exactly when every term is, so the run does not depend on the summation order."""
    sps, nslots = 64, 4096
    rng = np.random.default_rng(13)
    bits = (rng.random(nslots) < 0.003).astype(int)
    x = nrz(bits, sps, width=0) * 4                                                  # levels 0 and 4; Scott's bandwidth ~0.03
    x[(0 - (-sps // 2 + 1)) % x.size] = 1.0                                          # a 1 at t = -1 (outside the centre): y_center = 1
    gv(sps=sps, R=1e9)
    r = en.get_eye(x, sps, nslots)
    e = oa.GET_EYE(x, nslots=nslots)
    assert (r["mu0"], r["mu1"], r["y_center"]) == (0.0, 4.0, 1.0)
    grid = np.linspace(r["mu0"], r["mu1"], 500)
    yc = r["y"][(r["t_span0"] < r["t"]) & (r["t"] < r["t_span1"])]
    ih = 1.0 / (np.sqrt(np.var(yc, ddof=1)) * yc.size ** -0.2)
    kde = np.array([np.exp(-((yc * ih - g * ih) ** 2) / 2.0).sum() for g in grid])
    zero = np.nonzero(kde == 0.0)[0]
    assert zero.size > 20 and zero[-1] - zero[0] == zero.size - 1                  # one run of exact zeros
    assert e.threshold == grid[zero[0]]
    assert abs(e.threshold - r["threshold"]) <= 4 * (r["mu1"] - r["mu0"]) / 499    # scipy's run starts within a few points of it
    assert_same(e, dict(r, threshold=grid[zero[0]]))


# --- non-finite samples
@pytest.mark.parametrize("resamp", [None, 32])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_non_finite_samples_are_refused_and_the_device_recovers(bad, where, resamp):
    sps, nslots = 16, 256
    x, _, _, _ = random_eye(21)
    x = x[: sps * nslots].copy()
    x[{"first": 0, "middle": x.size // 2, "last": x.size - 1}[where]] = bad
    gv(sps=sps, R=1e9)
    with pytest.raises(ValueError, match="NaN|infinity"):
        en.get_eye(x, sps, nslots, resamp)
    with pytest.raises(ValueError, match="NaN|infinity"):
        oa.GET_EYE(x, nslots=nslots, sps_resamp=resamp)
    x[np.isnan(x) | np.isinf(x)] = 0.5
    eye_case(x, sps, nslots, resamp)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_non_finite_samples_are_refused_by_dsp(bad):
    x, sps, _, _ = random_eye(22)
    x = x.copy()
    x[x.size // 3] = bad
    gv(sps=sps, R=1e9)
    with pytest.raises(ValueError, match="NaN|infinity"):
        ook.DSP(electrical_signal(x))
    x[x.size // 3] = 0.5
    rx, e, rth = ook.DSP(electrical_signal(x))
    bits, r, _ = en.dsp(x, sps)
    assert_same(e, r)
    np.testing.assert_array_equal(rx.data, bits)


# ------------------------------------------------------------------------------------------------ FBG
APO = {"uniform": 0, "rcos": 1, "gaussian": 2, "parabolic": 3}
P = {"uniform": None,
     "rcos": lambda z: 1.0 if abs(z) <= 0 else 0.0 if abs(z) > 0.5 else 0.5 * (1 + np.cos(2 * np.pi * abs(z))),
     "gaussian": lambda z: np.exp(-4 * np.log(2) * (3 * z) ** 2),
     "parabolic": lambda z: 1 - (2 * z) ** 2}




def device_solve(d, s, k, F, apo, rtol=1e-3, atol=1e-6):
    n = d.size
    H = _lib.DeviceArray((n,), np.complex128, 0)
    info = (_lib._I64 * 3)()
    d, s, k = (np.ascontiguousarray(a, dtype=np.float64) for a in (d, s, k))
    rc = _lib.load().ssfm_fbg_solve(0, n, _lib._ptr(d), _lib._ptr(s), _lib._ptr(k), float(F), APO[apo], rtol, atol, None, None, _lib._VP(H.ptr), info)
    _lib._check(rc, "ssfm_fbg_solve")
    return H.to_host(), int(info[0]), int(info[1])


def crafted(n, kL=2.0, span=6.0, seed=0):
    """delta across +-span, a small random s, kappa = kL with a run of zeros in the middle quarter."""
    rng = np.random.default_rng(seed)
    d = np.linspace(-span, span, n) if n > 1 else np.array([0.3])
    s = rng.uniform(-0.2, 0.2, n)
    k = np.full(n, kL) * (1 + 0.1 * rng.standard_normal(n))
    zero = np.zeros(n, bool)
    zero[3 * n // 8: 3 * n // 8 + max(n // 16, 0)] = True
    k[zero] = 0.0
    return d, s, k, zero


def check_solve(d, s, k, F, apo, zero=None):
    H, steps, attempts = device_solve(d, s, k, F, apo)
    Hs, steps_s, attempts_s = scipy_H(d, s, k, F, P[apo], attempts=True)
    assert (steps, attempts) == (steps_s, attempts_s)
    assert np.max(np.abs(H - Hs)) <= 1e-9 * max(np.max(np.abs(Hs)), 1e-300)
    if zero is not None and zero.any():
        assert np.all(H[zero] == 0)
    return steps, attempts


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 18) + 3, (1 << 20) + 1])
def test_fbg_solve_sizes(n):
    """Up to 16 partials the fold adds one per thread; at 65 537 bins (257 partials) thread 0 adds two."""
    d, s, k, zero = crafted(n, seed=n)
    check_solve(d, s, k, 0.0, "uniform", zero)


def test_fbg_solve_apodizations_with_and_without_chirp():
    rejected = False
    for j, apo in enumerate(APO):
        for F in (0.0, 40.0):
            d, s, k, zero = crafted(3000, kL=16.0, span=60.0, seed=1)
            steps, attempts = check_solve(d, s, k, F, apo, zero)
            rejected |= attempts > steps
    assert rejected


def test_fbg_solve_at_its_cap():
    n = 1 << 22
    d, s, k, zero = crafted(n, kL=0.5, span=1.0, seed=4)
    check_solve(d, s, k, 0.0, "uniform", zero)
    with pytest.raises(_lib.SsfmError):
        device_solve(np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1), 0.0, "uniform")


@pytest.mark.parametrize("apply", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4097, (1 << 21) - 1, 1 << 21])
def test_fbg_delay(n, apply):
    rng = np.random.default_rng(n + apply)
    H = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    dt, tau = 1 / 400e9, 7.3e3                                                       # |w tau| up to ~9e3 rad: the phase wraps ~1400 times
    Hd = _lib.DeviceArray.from_host(H, np.complex128)
    Hn = _lib.DeviceArray((n,), np.complex128, 0)
    _lib._check(_lib.load().ssfm_fbg_delay(0, _lib._VP(Hd.ptr), _lib._VP(Hn.ptr), n, dt, tau, apply), "ssfm_fbg_delay")
    w = np.fft.fftshift(np.fft.fftfreq(n, dt)) * 2 * np.pi
    phase = -w * tau * 1e-12
    want = H * np.exp(1j * phase) if apply else H
    # Both sides form the phase with the same double operations in the same order (k / (n dt), x 2 pi, x tau, x 1e-12), so it is the
    # same double, and the complex product is the same expression.  What differs is cos / sin of the phase: the device's sincos against
    # NumPy's complex exp.  With an exact range reduction each is within ~1 ulp, so a few eps |H| would do.  A reduction by a
    # finite-precision 2 pi errs by ~eps |phase| in absolute terms, hence the (1 + |phase|) factor: |error| <= 8 eps (1 + |phase|) |H|.
    # That is ~1.6e-11 |H| at n = 2^21 (|phase| ~ 9e3); a shift by one bin, or a wrong phase, errs by O(|H|).
    bound = 8 * np.finfo(float).eps * (1 + np.abs(phase)) * np.abs(H)
    got_h, got_n = Hd.to_host(), Hn.to_host()
    assert np.all(np.abs(got_h - want) <= bound)
    assert np.all(np.abs(got_n - np.fft.ifftshift(want)) <= np.fft.ifftshift(bound))
    if apply:
        assert np.max(np.abs(phase)) > 100 * np.pi or n < 4097


@pytest.mark.parametrize("n", [(1 << 21) - 1, 1 << 21])
def test_fbg_end_to_end_at_the_filtering_cap(n):
    gv(fs=400e9)
    rng = np.random.default_rng(n)
    sig = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.1
    nz = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.01
    out, H = oa.FBG(optical_signal(sig, nz), fc=gv.f0, vdneff=1e-4, kL=2, print_params=False, retH=True)
    Hn = np.fft.ifftshift(H)
    for got, x in ((out.signal, sig), (out.noise, nz)):
        want = np.fft.ifft(np.fft.fft(x, axis=-1) * Hn, axis=-1)
        assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))


def test_fbg_beyond_the_filtering_cap_is_refused_before_the_solve():
    gv(fs=400e9)
    x = optical_signal(np.ones(1 << 12, complex))
    oa.FBG(x, fc=gv.f0, vdneff=1e-4, kL=2, print_params=False)
    before = (oa.FBG.last_steps, oa.FBG.last_attempts, oa.FBG.last_waits)
    big = optical_signal(np.ones((1 << 21) + 1, complex))
    with pytest.raises(ValueError, match=r"2\^21"):
        oa.FBG(big, fc=gv.f0, vdneff=1e-4, kL=2, print_params=False)
    assert (oa.FBG.last_steps, oa.FBG.last_attempts, oa.FBG.last_waits) == before
