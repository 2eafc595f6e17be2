"""GPU parity tests (``-m gpu``): the HIP path, called through the C ABI, against
(1) outputs captured from the imported reference (tests/golden/*.npz),
(2) the oracle on the same seeded inputs at sizes it finishes in seconds,
(3) size-independent properties at the full 2^20 x 2 benchmark size.

Stated tolerances: complex64, fixed h: max|d|/peak <= 2e-5 up to 100 steps,
<= 3e-4 at 1000 steps (the reference's own complex64 noise floor against float64 is 5e-6 /
8e-5); adaptive: the same bound at z = L with the step count within +-1; complex128: <= 1e-10.
Round 6: ONE continuous bound, `opticomlib_amd.accuracy.tol(steps)` (2e-5 up to 100 steps, the log-log
line to 3e-4 at 1000, proportional to the steps beyond) -- `TOL_100` / `TOL_1000` below are tol(100) /
tol(1000) and are only used for runs of at most 100 / of exactly 1000 steps.  Every comparison goes through
`margins.within`, which writes the error it measured beside its bound (profiles/r06_parity_margins.txt).
"""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, workloads
from opticomlib_amd.typing import NULL, gv, optical_signal
from cases import CASES, case_dt, case_input
from oracle import ssfm_numpy as orc

pytestmark = pytest.mark.gpu

from margins import relmax, steps_of, within
from opticomlib_amd.accuracy import TOL_C128, tol as tol_at

TOL_100 = tol_at(100)        # 2e-5: runs of up to 100 steps
TOL_1000 = tol_at(1000)      # 3e-4: runs of exactly 1000 steps (anything between states tol_at(steps))


def _npts(case):
    return case["inp"][2][-1] if "inp" in case else 0


def _signal(case):
    gv(**case["gv"])
    sig, noi = case_input(case)
    return optical_signal(sig) if noi is None else optical_signal(sig, noi)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


# ----------------------------------------------------------------------- FFT building block
@pytest.mark.parametrize("k", range(8, 23))
@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
def test_fft_against_numpy(k, prec):
    n = 1 << k
    cd = np.complex64 if prec == _lib.C64 else np.complex128
    rng = np.random.default_rng(k)
    x = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(cd)
    p = _lib.Plan(n, 2, prec)
    try:
        p.set_field(x)
        X = p.debug_fft()
        ref = np.fft.fft(x.astype(np.complex128), axis=-1)
        err = np.linalg.norm(X - ref) / np.linalg.norm(ref)
        assert err < (3e-7 if prec == _lib.C64 else 2e-15)
        p.set_field(x)
        p.apply_transfer(np.ones(n, dtype=cd))          # ifft(fft(x))
        y = p.get_field()
        err2 = np.linalg.norm(y - x) / np.linalg.norm(x)
        assert err2 < (5e-7 if prec == _lib.C64 else 2e-15)
    finally:
        p.close()


# ----------------------------------------------------------------------- golden vectors
POW2 = [n for n, c in CASES.items() if _npts(c)]          # every captured case: other lengths take the chirp-z path


@pytest.mark.parametrize("name", [n for n in POW2 if CASES[n]["func"] in ("FIBER", "DBP")])
def test_fiber_dbp_golden(golden_dir, name):
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x = _signal(case)
    fn = oa.FIBER if case["func"] == "FIBER" else oa.DBP
    kw = dict(case["kw"])
    nsteps_ref = len(g["z"]) - 1 if "z" in g else (steps_of(kw) or 1)      # (adaptive goldens without a z log are the single-step cases)
    tol = tol_at(nsteps_ref)
    if kw.get("return_steps"):
        z, A_z = fn(x, **kw)
        assert z.dtype == np.float64 and A_z.dtype == np.complex64
        assert A_z.shape == g["A_z"].shape
        np.testing.assert_array_equal(z, g["z"])
        assert within(A_z, g["A_z"], tol, steps=nsteps_ref, what="golden A_z, every step")
        return
    y = fn(x, **kw)
    assert isinstance(y, optical_signal) and y.noise is NULL
    assert y.signal.dtype == np.complex64 and y.signal.shape == g["out"].shape
    assert y.n_pol == (2 if g["out"].ndim == 2 else 1)
    assert y.execution_time > 0
    assert within(y.signal, g["out"], tol, steps=nsteps_ref, what="golden out")
    if "z" in g:
        z, A_z = fn(x, return_steps=True, **kw)
        if kw.get("h") is not None:
            np.testing.assert_array_equal(z, g["z"])            # float32 schedule reproduced exactly
        else:
            assert abs(len(z) - len(g["z"])) <= 1                 # adaptive: chaotic in the last bit
            m = min(len(z), len(g["z"])) - 1
            np.testing.assert_allclose(z[:m], g["z"][:m], rtol=2e-4)
        # (adaptive: the bound of the run's own step count; a +-1 mismatch is a different splitting of the last stretch and is
        # held to the same bound -- the goldens' adaptive runs are 29 ... 60 steps, far from where that matters)
        assert within(A_z[-1], g["out"], tol, steps=len(z) - 1, what="golden out, return_steps run")


def test_fiber_then_dbp_golden(golden_dir):
    case = CASES["fiber_then_dbp"]
    g = np.load(os.path.join(golden_dir, "fiber_then_dbp.npz"))
    x = _signal(case)
    mid = oa.FIBER(x, **case["kw"])
    out = oa.DBP(mid, **case["kw"])
    assert within(mid.signal, g["mid"], kw=case["kw"], what="golden FIBER leg")
    assert within(out.signal, g["out"], steps=2 * steps_of(case["kw"]), what="golden FIBER + DBP")
    # KAT-3: not the identity -- parity is against the reference's DBP output, not the input
    assert np.max(np.abs(out.signal - x.signal)) > 1e-3


@pytest.mark.parametrize("name", [n for n in POW2 if CASES[n]["func"] == "DM"])
def test_dm_golden(golden_dir, name):
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x = _signal(case)
    r = oa.DM(x, **case["kw"])
    if case["kw"].get("retH"):
        y, H = r
        assert H.dtype == np.complex128 and H.shape == g["H"].shape
        np.testing.assert_allclose(H, g["H"], rtol=0, atol=1e-15)     # H is generated on the device (sincos within 1 ulp)
    else:
        y = r
    assert y.signal.dtype == np.complex128 and y.n_pol == x.n_pol
    assert within(y.signal, g["out"], 1e-13)
    if "out_noise" in g:
        assert within(y.noise, g["out_noise"], 1e-13)
    else:
        assert y.noise is NULL


@pytest.mark.parametrize("name", [n for n in POW2 if CASES[n]["func"] == "TWIN"])
def test_c128_against_reference_twin(golden_dir, name):
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x = _signal(case)
    kw = case["kw"]
    y = oa.FIBER(x, precision="complex128", **kw)
    assert y.signal.dtype == np.complex128
    want = g["A_last"] * np.exp(-(kw["alpha"] / 4.343) * g["z"][-1] / 2)
    assert within(y.signal, want, TOL_C128)


# ----------------------------------------------------------------------- lengths that are not powers of two
@pytest.mark.parametrize("n,npol", [(3000, 1), (1000, 2), (257, 1), (64, 2), (12345, 2), (100003, 1), (2, 1), (3, 2)])
def test_any_length_fixed_step_against_oracle(n, npol):
    """Chirp-z path (complex128 arithmetic on a power-of-two plan): composite, prime, tiny and small power-of-two
    lengths against the oracle's complex64 run -- the difference is the reference's own float32 rounding."""
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(n)
    a = (rng.standard_normal((npol, n)) + 1j * rng.standard_normal((npol, n))) * 0.03
    a = a[0] if npol == 1 else a
    kw = dict(length=6, h=0.7, **workloads.SMF)                       # 9 steps, the last one short
    y = oa.FIBER(optical_signal(a), **kw)
    assert y.signal.dtype == np.complex64 and y.signal.shape == a.shape and y.n_pol == npol
    ref = orc.fiber_c64(a, gv.dt, **kw)
    assert within(y.signal, ref, kw=kw, what="oracle")
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    np.testing.assert_array_equal(z, zr)
    assert A_z.shape == Ar.shape and A_z.dtype == np.complex64 and within(A_z, Ar, kw=kw, what="oracle, every step")
    back = oa.DBP(y, **kw)                                             # device-resident input of odd length
    assert within(back.signal, orc.dbp_c64(ref, gv.dt, **kw), steps=2 * steps_of(kw), what="oracle FIBER + DBP")


@pytest.mark.parametrize("n,npol,steps", [(100003, 2, 40), (140001, 1, 120), (300007, 2, 12)])
def test_long_lines_hold_complex64_between_float64_passes(n, npol, steps, monkeypatch):
    """Round 6: a complex64 caller's fixed-step run of more than 65536 samples that are not a power of two keeps its chirp-z line (2^18 points and more) as
    complex64 BETWEEN the passes while every pass computes in float64 (ssfm_kernels.hpp time_body / freq_body, H) and goes out on the plan's two lanes: against
    the complex128 line of the same schedule (SSFM_CHIRP_HALF=0; 1e-13 from the float64 solution) the difference is the four roundings to complex64 per step --
    a few 1e-7, twenty times inside the bound; against the oracle it is the oracle's own float32 transforms.  One lane: the same bits."""
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(n)
    a = ((rng.standard_normal((npol, n)) + 1j * rng.standard_normal((npol, n))) * 0.03).astype(np.complex64)
    a = a[0] if npol == 1 else a
    kw = dict(length=steps * 0.25 - 0.1, h=0.25, **workloads.SMF)                     # (the last step short: two step sizes)
    for k in ("SSFM_CHIRP_HALF", "SSFM_LANES", "SSFM_E", "SSFM_EF"):            # (the knobs this comparison of two lines depends on are pinned: the complex64-storage passes
        monkeypatch.delenv(k, raising=False)                                    # exist for the plans' default points per thread)
    oa.devices.release_plans()
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert y.dtype == np.complex64 and y.shape == a.shape
    monkeypatch.setenv("SSFM_LANES", "1")
    assert np.array_equal(oa.FIBER(optical_signal(a), **kw).signal, y)
    monkeypatch.delenv("SSFM_LANES")
    monkeypatch.setenv("SSFM_CHIRP_HALF", "0")
    wide = oa.FIBER(optical_signal(a), **kw).signal
    monkeypatch.delenv("SSFM_CHIRP_HALF")
    assert not np.array_equal(wide, y)                                                # (the knob really chose the other line)
    assert within(y, wide, 2e-6, kw=kw, what="complex128 line of the same schedule")
    if n * steps <= 6e6:
        assert within(y, orc.fiber_c64(a, gv.dt, **kw), kw=kw, what="oracle")
        y128 = oa.FIBER(optical_signal(a), precision="complex128", **kw).signal      # a complex128 caller never takes it: the float64 restatement to 1e-10
        assert y128.dtype == np.complex128 and within(y128, orc.fiber_c128(a, gv.dt, **kw), TOL_C128, kw=kw, what="float64 restatement")


def test_long_lines_adaptive_run(monkeypatch):
    """... and the adaptive run of such a length (the reference's default, h=None): five passes per step with the caller's field at both ends of every step -- the
    line between them complex64, a table of n entries, nothing done by the passes queued behind the run's end.  Same z log as the complex128 line and as the oracle
    (float32 step arithmetic in both), the field within the bound of the oracle and 2e-6 of the complex128 line."""
    gv(**workloads.BENCH_GV)
    n = 100003
    rng = np.random.default_rng(n + 5)
    a = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.14
    # (noise in an eighth of the band, as a signal of two samples per symbol in a 16-sample grid would be: with the WHOLE band full -- 28 rad of dispersion per km at its edge --
    # the reference's own float32 z accumulation decides the length of the last, clamped step to 3e-6 km, and two correct runs end 3e-5 apart: tests/diag/adaptive_long_diag.py)
    spec = np.fft.fft(a, axis=-1)
    spec[:, n // 16: n - n // 16] = 0
    a = np.fft.ifft(spec, axis=-1).astype(np.complex64)
    kw = dict(length=12, phi_max=0.02, **workloads.SMF)
    for k in ("SSFM_CHIRP_HALF", "SSFM_E", "SSFM_EF"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()
    y = oa.FIBER(optical_signal(a), **kw).signal
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    monkeypatch.setenv("SSFM_CHIRP_HALF", "0")
    wide = oa.FIBER(optical_signal(a), **kw).signal
    zw, _ = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    monkeypatch.delenv("SSFM_CHIRP_HALF")
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    steps = len(zr) - 1
    assert steps >= 8 and len(z) == len(zw) == len(zr)
    np.testing.assert_allclose(z, zw, rtol=1e-6)
    np.testing.assert_allclose(z, zr, rtol=2e-4)
    assert not np.array_equal(y, wide) and within(y, wide, 2e-6, steps=steps, what="complex128 line, adaptive")
    # The oracle transforms this PRIME length in float32 (pocketfft's Bluestein): its own maxima, and with them its step sizes, move by up to 1.5e-4 of a step, and a
    # band full of noise turns that into several 1e-5 of the field.  The judge of both runs is the float64 solution of the reference's adaptive problem
    # (fuzz_cases.truth_adaptive_f64: float32 coefficients and step rule, float64 transforms): the HIP run is held to it by HALF the bound and takes ITS steps,
    # the oracle is wherever it is, and the two are held together by the sum.
    zt, truth = _fuzz_module().truth_adaptive_f64(a, gv.dt, kw)
    assert len(zt) == len(z)
    np.testing.assert_allclose(z, zt, rtol=3e-6)
    oracle_off = relmax(Ar[-1], truth)
    assert within(y, truth, 0.5 * tol_at(steps), steps=steps, what="float64 solution of the adaptive problem")
    assert within(y, Ar[-1], oracle_off + 0.5 * tol_at(steps), steps=steps, what=f"oracle adaptive (itself {oracle_off:.2e} from the float64 solution)")
    assert within(A_z[-1], y, 1e-6, steps=steps, what="return_steps, the same run a step at a time")
    # a complex128 caller's adaptive run of this length takes the lanes and the short table too, and keeps its complex128 line: the same field as round 5's form to 1e-12
    kw128 = dict(kw, length=4)
    y128 = oa.FIBER(optical_signal(a), precision="complex128", **kw128).signal
    monkeypatch.setenv("SSFM_CHIRP_HALF", "0")
    w128 = oa.FIBER(optical_signal(a), precision="complex128", **kw128).signal
    monkeypatch.delenv("SSFM_CHIRP_HALF")
    assert y128.dtype == np.complex128 and within(y128, w128, 1e-12, what="complex128 caller, adaptive: lanes and a table of n entries against round 5's form")


@pytest.mark.parametrize("n", [3000, 5001])
def test_any_length_adaptive_complex128_and_dm(n):
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(n + 1)
    a = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.07
    kw = dict(length=10, phi_max=0.02, **workloads.SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    assert abs(len(z) - len(zr)) <= 1 and abs(z[-1] - 10.0) < 1e-4
    m = min(len(z), len(zr)) - 1
    np.testing.assert_allclose(z[:m], zr[:m], rtol=2e-4)
    assert within(A_z[-1], Ar[-1], steps=len(z) - 1, what=f"oracle adaptive, return_steps ({len(z) - 1} vs {len(zr) - 1} steps)")
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert within(y, Ar[-1], steps=len(zr) - 1, what="oracle adaptive")
    # complex128 extension against the float64 restatement
    kwf = dict(length=5, h=0.5, **workloads.SMF)
    y128 = oa.FIBER(optical_signal(a), precision="complex128", **kwf).signal
    assert y128.dtype == np.complex128 and within(y128, orc.fiber_c128(a, gv.dt, **kwf), TOL_C128, kw=kwf, what="float64 restatement")
    # DM: signal and noise apart, H as the reference forms it
    nz = 0.1 * a[::-1].copy()
    d, H = oa.DM(optical_signal(a, nz), D=-150.0, retH=True)
    ds, dn = orc.dm_c128(a, gv.dt, -150.0, noise=nz)
    assert within(d.signal, ds, 1e-12) and within(d.noise, dn, 1e-12)
    np.testing.assert_allclose(H, np.fft.fftshift(orc.dm_transfer(n, gv.dt, -150.0)), rtol=0, atol=1e-15)


@pytest.mark.parametrize("n", [100, 500, 1016, 2032, 3000, 8176])
def test_any_length_run_driven_from_c_against_the_host_loop(n, monkeypatch):
    """Lengths that are not powers of two: the whole run queued from C (ssfm_chirp_propagate; adaptive: the step rule evaluated on the device in
    the caller's float32 arithmetic) against the loop that calls one entry point per kernel from Python and waits for every step's maximum
    (SSFM_CHIRP_LOOP=python).  The C loop takes five launches per step -- the middle of a step in one column launch, the step's two ends inside the
    first and the last -- so the product with exp(D~ h) and the chirp products are rounded in other places than in the host loop's nine: 1e-12 ("c5").  Up to
    2048 samples a fixed-step run is one launch (k_small_chirp; SSFM_CHIRP_SMALL=0 turns it off), with the two half rotations between steps merged
    into one: 1e-12 as well.  (Round 3's nine- and seven-launch forms of the C loop, bit-identical to the host loop, were removed in round 4.)"""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 14, seed=n, power_w=8e-3)[:, :n]
    x = optical_signal(a)
    for kw in (dict(length=6.0, h=0.37, **workloads.SMF), dict(length=8.0, phi_max=0.004, **workloads.SMF)):
        res = {}
        for name, env in (("python", {"SSFM_CHIRP_LOOP": "python"}), ("c5", {"SSFM_CHIRP_LOOP": "c", "SSFM_CHIRP_SMALL": "0", "SSFM_MEDIUM": "0"}),
                          ("c", {"SSFM_CHIRP_LOOP": "c", "SSFM_CHIRP_SMALL": "1", "SSFM_MEDIUM": "1"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            y = oa.FIBER(x, **kw).signal
            z, _ = oa.FIBER(x, return_steps=True, **kw) if name == "python" else (None, None)
            res[name] = (y, z)
        for name in ("c5", "c"):      # (c5: five launches per step; c: n <= 2048: the whole run in one launch)
            tol = 1e-12 * (1 if "h" in kw else 1e4)                 # (adaptive: a last-bit difference in a maximum moves a step size)
            if name == "c":
                tol = TOL_100      # (round 4: a complex64 caller's run of up to 65536 samples is ONE launch on a complex64 line -- the reference's own arithmetic class)
            assert within(res[name][0], res["python"][0], tol, steps=len(res["python"][1]) - 1, what=f"the run driven from C ({name}) against the host loop"), name
        assert len(res["python"][1]) > 10
        if n <= 2048:
            # the complex128 line in one launch (precision="complex128") against the complex128 host loop: 1e-12 as before
            monkeypatch.setenv("SSFM_CHIRP_LOOP", "python")
            r128 = oa.FIBER(x, precision="complex128", **kw).signal
            monkeypatch.setenv("SSFM_CHIRP_LOOP", "c"); monkeypatch.setenv("SSFM_CHIRP_SMALL", "1")
            y128 = oa.FIBER(x, precision="complex128", **kw).signal
            assert y128.dtype == np.complex128 and within(y128, r128, 1e-12 * (1 if "h" in kw else 1e4))
            # ... and the complex64 line against the oracle (the reference's complex64 run of the same field)
            y64 = oa.FIBER(x, **kw).signal
            zo, Ao = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
            assert y64.dtype == np.complex64 and within(y64, Ao[-1], steps=len(zo) - 1, what="oracle, complex64 one-launch line")
    # one polarisation (a single row: the one-launch adaptive engine has nobody to exchange maxima with)
    x1, kw = optical_signal(a[0]), dict(length=8.0, phi_max=0.004, **workloads.SMF)
    monkeypatch.setenv("SSFM_CHIRP_LOOP", "python")
    ref = oa.FIBER(x1, **kw).signal
    monkeypatch.setenv("SSFM_CHIRP_LOOP", "c")
    assert within(oa.FIBER(x1, **kw).signal, ref, TOL_100, what="one polarisation, adaptive: the run driven from C against the host loop")  # (the complex64 line, see above)
    monkeypatch.setenv("SSFM_CHIRP_SMALL", "0"); monkeypatch.setenv("SSFM_MEDIUM", "0")
    assert within(oa.FIBER(x1, **kw).signal, ref, 1e-8)  # (the complex128 line queued from C)


@pytest.mark.parametrize("precision", ["complex64", "complex128"])
@pytest.mark.parametrize("n", [100, 200, 500, 1016, 2032])
def test_any_length_one_launch_line_of_every_length_against_oracle(n, precision, monkeypatch):
    """The one-workgroup chirp-z kernels (k_small_chirp, k_small_chirp_adapt) on every line length they are built for -- 256, 512, 1024, 2048, 4096 points for
    100, 200, 500, 1016, 2032 samples -- in both precisions: two rows, a fixed run of 12 steps and an adaptive run of 15 to 19, against the float64 restatement
    of the same call at the bound of the run's step count.  The plan of the line says which engine ran: a run that took another one fails here."""
    for k in ("SSFM_SMALL", "SSFM_CHIRP_SMALL", "SSFM_CHIRP_LOOP", "SSFM_FUSED_PATIENCE_TICKS", "SSFM_E", "SSFM_EF"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()                  # (a plan reads its knobs when it is made)
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 12, seed=5, power_w=8e-3)[:, :n]
    x = optical_signal(a)
    M = 1 << (2 * n - 2).bit_length()
    for kw, engine in ((dict(length=6.0, h=0.5, **workloads.SMF), "chirp_small"), (dict(length=3.0, phi_max=0.004, **workloads.SMF), "chirp_small_adaptive")):
        y = oa.FIBER(x, precision=precision, **kw).signal
        info = oa.devices.get_plan(M, 2, _lib.C64 if precision == "complex64" else _lib.C128, 0).last_run_info()
        assert info["engine"] == engine and not info["fell_back"], (info, kw)
        assert y.dtype == np.dtype(precision) and y.shape == a.shape
        ns = len(orc.fiber_c64(a, gv.dt, return_steps=True, **kw)[0]) - 1
        assert 10 <= ns <= 20, ns
        assert within(y, orc.fiber_c128(a, gv.dt, **kw), steps=ns, what=f"float64 restatement, line of {M} points ({engine})")


@pytest.mark.parametrize("n,npol", [(3000, 2), (8176, 2), (8176, 1), (15060, 2), (32752, 2), (40000, 1), (65533, 1)])
def test_any_length_medium_line_in_one_launch_against_oracle(n, npol, monkeypatch):
    """complex64 callers, fixed steps, 2048 < n <= 65536 (the reference's own generators: PRBS-9 / -11 words at 16 samples per bit are 8176 / 32752 samples):
    the whole run in one launch on one XCD on a complex64 line of M >= 2n - 1 points (k_medium_chirp behind ssfm_chirp_propagate_c64) -- against the oracle's complex64
    run and the float64 restatement after 26 steps (the last one short: the longest run below the window in which the line has no margin, round 6), the single
    full-length step of a fibre without nonlinearity, and the five-launch complex128 line of the same call (SSFM_MEDIUM=0).  The engine that ran is read back: a
    silent fall to the general path fails the test.  Then the window itself (opticomlib_amd.accuracy: 27 ... 1031 steps, derived from the line's measured error law
    8.5e-7 x steps^0.75 against half of the continuous bound tol(steps)): runs inside it take the complex128 line, a run beyond it (1100 steps) the one launch again."""
    for k in ("SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_ADAPT_FUSED", "SSFM_CHIRP_LOOP", "SSFM_FUSED_PATIENCE_TICKS", "SSFM_E", "SSFM_EF"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()                  # (a plan reads its knobs when it is made: none made under the knob suite's environment is reused here)
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 16, seed=n % 997, power_w=4e-3, n_pol=2)[:npol, :n]
    a = a[0] if npol == 1 else a
    x = optical_signal(a)
    M = 1 << (2 * n - 2).bit_length()
    for kw in (dict(length=12.7, h=0.5, **workloads.SMF), dict(length=40.0, alpha=0.2, beta_2=-21.7, beta_3=0.13, gamma=0.0),
               dict(length=4.0, phi_max=0.002, **workloads.SMF)):                   # (adaptive: 17 to 20 steps, k_medium_chirp_adapt)
        out = oa.FIBER(x, **kw)
        y = out.signal
        info = oa.devices.get_plan(M, npol, _lib.C64, 0).last_run_info()
        assert out.engine == "chirp_medium_c64", (out.engine, kw)
        assert info["engine"] == ("chirp_medium_adaptive" if "phi_max" in kw else "chirp_medium") and not info["fell_back"], info
        assert y.dtype == np.complex64 and y.shape == a.shape
        zo, Ao = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
        ns = len(zo) - 1
        assert within(y, Ao[-1], steps=ns, what="oracle")
        assert within(y, orc.fiber_c128(a, gv.dt, **kw), steps=ns, what="float64 restatement")
        monkeypatch.setenv("SSFM_MEDIUM", "0")
        y5 = oa.FIBER(x, **kw).signal
        monkeypatch.delenv("SSFM_MEDIUM")
        assert within(y, y5, steps=ns, what="the complex128 line of the same call")
    kw = dict(length=10.0, h=0.5, **workloads.SMF)
    y = oa.FIBER(x, **kw)
    back = oa.DBP(y, **kw)                                                                                # device-resident input of odd length
    assert within(back.signal, orc.dbp_c64(orc.fiber_c64(a, gv.dt, **kw), gv.dt, **kw), steps=2 * steps_of(kw), what="oracle FIBER + DBP")
    # Runs of 27 ... 1031 steps, where the complex64 line's own error law exceeds half of the stated tolerance (accuracy.c64_line_has_margin), take the
    # complex128 line -- fixed step by the count, adaptive by the estimate from the first step size: the float64 solution to the coefficients' rounding
    from opticomlib_amd import accuracy
    assert accuracy.c64_line_window() == (27, 1031) and oa.devices._C64_LINE_NO_MARGIN == (27, 1031)
    for kw in (dict(length=30.0, h=0.5, **workloads.SMF), dict(length=12.0, phi_max=0.002, **workloads.SMF),      # 60 steps; 50 to 60 steps
               dict(length=50.2, h=0.5, **workloads.SMF)):                                                          # 101 steps: round 5 ran these on the complex64 line
        out = oa.FIBER(x, **kw)
        assert out.engine == "chirp_line_c128", (out.engine, kw)
        zo, Ao = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
        assert within(out.signal, orc.fiber_c128(a, gv.dt, **kw), 5e-6, steps=len(zo) - 1, what="float64 restatement (complex128 line)")
        assert within(out.signal, Ao[-1], steps=len(zo) - 1, what="oracle (complex128 line)")
    if n == 3000:      # beyond the window: 1100 steps on the one-launch line again, inside tol(1100) = 3.3e-4 of the oracle and of the float64 solution
        kw = dict(length=137.5, h=0.125, **workloads.SMF)
        out = oa.FIBER(x, **kw)
        assert out.engine == "chirp_medium_c64" and steps_of(kw) == 1100, (out.engine, steps_of(kw))
        assert within(out.signal, orc.fiber_c64(a, gv.dt, **kw), kw=kw, what="oracle, 1100 steps on the complex64 line")
        # (the float64 solution of the reference's problem: float32 coefficients and schedule, float64 arithmetic -- fuzz_cases.truth_f64; the float64
        # restatement fiber_c128 rounds no coefficient and is another 1e-5 away after so many steps)
        hs, _ = oa.devices.step_schedule(kw["length"], kw["h"])
        truth = _fuzz_module().truth_f64(a, gv.dt, hs, kw)
        assert within(out.signal, truth, kw=kw, what="float64 solution, 1100 steps on the complex64 line")


def test_the_medium_chirp_line_hands_the_field_back_untouched_when_it_cannot_run(monkeypatch):
    """The one-XCD chirp-z engine from the plan level (ssfm_chirp_propagate_c64): without patience (SSFM_FUSED_PATIENCE_TICKS=-1) the launch's workgroups give up at their first meeting -- the
    call says so (False), the caller's field is bit for bit what it was, the plan counts a fallback and does not try again; a schedule of more than four
    step sizes is refused before anything is launched; and the same call with patience gives the oracle's result."""
    for k in ("SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_ADAPT_FUSED", "SSFM_E", "SSFM_EF"):
        monkeypatch.delenv(k, raising=False)
    gv(**workloads.BENCH_GV)
    n, M = 5001, 16384
    a = workloads.qpsk_field(1 << 13, seed=9, power_w=4e-3, n_pol=2)[:, :n].astype(np.complex64)
    chirp = _lib.chirp_device(n, False, 0).astype(np.complex64)
    Dt = _lib.DeviceArray.from_host(np.asarray(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, _lib.C64), dtype=np.complex64), np.complex64, 0)
    hs = np.array([0.5] * 20 + [0.25], dtype=np.float64)
    monkeypatch.setenv("SSFM_FUSED_PATIENCE_TICKS", "-1")
    p = _lib.Plan(M, 2, _lib.C64)
    try:
        A = _lib.DeviceArray.from_host(a, np.complex64, 0)
        assert p.chirp_propagate_c64(A, chirp, Dt, 1.3, hs) is False
        np.testing.assert_array_equal(A.to_host(), a)
        info = p.last_run_info()
        assert info["engine"] == "chirp_medium" and info["fell_back"] and info["fallbacks_total"] == 1
        assert p.chirp_propagate_c64(A, chirp, Dt, 1.3, hs) is False            # (the engine is off for this plan now)
        np.testing.assert_array_equal(A.to_host(), a)
    finally:
        p.close()
    p = _lib.Plan(M, 2, _lib.C64)
    try:
        A = _lib.DeviceArray.from_host(a, np.complex64, 0)
        assert p.chirp_propagate_c64(A, chirp, Dt, 1.3, None, length=5.0, phi_max=0.004, max_steps=1000) is None
        np.testing.assert_array_equal(A.to_host(), a)
        info = p.last_run_info()
        assert info["engine"] == "chirp_medium_adaptive" and info["fell_back"] and info["fallbacks_total"] == 1
    finally:
        p.close()
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS")
    q = _lib.Plan(M, 2, _lib.C64)
    try:
        A = _lib.DeviceArray.from_host(a, np.complex64, 0)
        assert q.chirp_propagate_c64(A, chirp, Dt, 1.3, np.array([0.5, 0.4, 0.3, 0.2, 0.1])) is False
        np.testing.assert_array_equal(A.to_host(), a)
        assert q.chirp_propagate_c64(A, chirp, Dt, 1.3, hs) is True
        ref = a
        for h in hs:
            ref = orc.fiber_c64(ref, gv.dt, length=float(h), h=float(h), alpha=0.2, beta_2=-21.7, beta_3=0.13, gamma=1.3)
        assert within(A.to_host(), ref, steps=len(hs), what="oracle, step by step")
        assert q.last_run_info()["engine"] == "chirp_medium"
        A = _lib.DeviceArray.from_host(a, np.complex64, 0)
        steps, z = q.chirp_propagate_c64(A, chirp, Dt, 1.3, None, length=5.0, phi_max=0.004, max_steps=1000)
        zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, length=5.0, phi_max=0.004, alpha=0.2, beta_2=-21.7, beta_3=0.13, gamma=1.3)
        assert abs(steps + 1 - len(zr)) <= 1 and len(z) == steps + 1 and abs(z[-1] - 5.0) < 1e-5
        m = min(len(z), len(zr)) - 1
        np.testing.assert_allclose(z[:m], zr[:m], rtol=2e-4)
        assert within(A.to_host(), Ar[-1], steps=steps, what=f"oracle adaptive ({steps} vs {len(zr) - 1} steps)")
        assert q.last_run_info()["engine"] == "chirp_medium_adaptive"
    finally:
        q.close()


def _fuzz_module():
    import sys
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag")
    if d not in sys.path:
        sys.path.insert(0, d)
    import fuzz_cases
    return fuzz_cases


@pytest.mark.parametrize("index", [39, 75, 81])
def test_the_three_fuzz_cases_round_4_left_beyond_the_tolerance(index, monkeypatch):
    """profiles/r04_final_fuzz.txt: 3 of 400 random propagations beyond the stated 2e-5 (13232 x 1, 35 steps, a gain fibre; 15060 x 2 adaptive, 81 steps;
    10426 x 1, 66 steps), all on the one-launch complex64 chirp-z line.  Measured in round 5 (profiles/r05_chirp_margin.txt): in all three the ORACLE
    itself sits 1.5 ... 2.6e-5 from the float64 solution (awkward lengths, strong nonlinearity), so no computation can be within 2e-5 of it; and the
    complex64 line had used up the margin that keeps it out of such trouble elsewhere.  Now: runs of 32 ... 100 steps take the complex128 line
    (devices._c64_line_has_margin), and the bound is stated against the float64 solution as well (fuzz_cases.judge): within half the tolerance of it or
    at most 1.5 x as far from it as the oracle; from the oracle within the tolerance or 2.5 x the oracle's own distance."""
    for k in ("SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_CHIRP_LOOP", "SSFM_CHIRP_SMALL", "SSFM_FUSED_PATIENCE_TICKS"):
        monkeypatch.delenv(k, raising=False)
    fc = _fuzz_module()
    gv(**workloads.BENCH_GV)
    case = [c for c in fc.cases(index + 1, 2026)][-1]
    i, n, npol, kw, a, pow2 = case
    assert (n, npol) == {39: (10426, 1), 75: (13232, 1), 81: (15060, 2)}[index]
    engine, steps, (ok, e_ho, e_ht, e_ot) = fc.run_case(oa, gv, optical_signal, kw, a)
    assert engine == "chirp_line_c128", (engine, steps)
    assert e_ht < 5e-6, (e_ht, e_ot)                              # the complex128 line: the float64 solution itself, to the rounding of the (adaptive: its own) schedule
    assert ok and e_ho <= 1.05 * e_ot, (e_ho, e_ht, e_ot)       # ... so what separates it from the oracle is the oracle's own distance


def test_fuzz_slice_against_the_oracle_and_the_float64_solution(monkeypatch):
    """The first 40 configurations of the stress run's stream (tests/diag/fuzz_many.py, seed 2026): every one within the stated bound of BOTH the oracle
    and the float64 solution (fuzz_cases.judge), whatever engine it takes."""
    for k in ("SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_CHIRP_LOOP", "SSFM_CHIRP_SMALL", "SSFM_FUSED_PATIENCE_TICKS"):
        monkeypatch.delenv(k, raising=False)
    fc = _fuzz_module()
    gv(**workloads.BENCH_GV)
    bad, engines = [], set()
    for i, n, npol, kw, a, pow2 in fc.cases(40, 2026):
        engine, steps, (ok, e_ho, e_ht, e_ot) = fc.run_case(oa, gv, optical_signal, kw, a)
        engines.add(engine)
        if not ok:
            bad.append((i, n, npol, steps, engine, e_ho, e_ht, e_ot))
    assert not bad, bad
    assert {"chirp_medium_c64", "chirp_line_c128"} <= engines, engines          # the slice covers both chirp-z lines


def test_any_length_with_nothing_to_propagate_is_the_identity():
    """length = 0 (the reference's loop does not run, devices.py:1172): the chirp-z path hands the input back -- fixed step (an empty schedule),
    the single full-length step of a dispersion-free fibre ([L] = [0]: round 3 returned SSFM_ERR_INVALID from the one-launch kernel) and adaptive."""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 10, seed=3, power_w=2e-3)[:, :777]
    x = optical_signal(a)
    for kw in (dict(length=0.0, h=0.5, **workloads.SMF), dict(length=0.0, gamma=1.3), dict(length=0.0, phi_max=0.01, **workloads.SMF)):
        y = oa.FIBER(x, **kw).signal
        np.testing.assert_array_equal(y, a.astype(np.complex64))


# The three chirp-z lines at their smallest lengths: (samples, precision, engine).  1000 samples: a line of 2048 points, the small complex64 line;
# 2049: a line of 8192, the first length of the medium line; complex128 callers: the complex128 line.  Dual polarisation, a fixed step that gives
# 5 steps and an adaptive bound that gives 16 or 17 / 14 steps (the tests assert 10 ... 40; the medium line runs below its window without margin, 27 steps).
_CHIRP_LINES = [(1000, "complex64", "chirp_small_c64"), (2049, "complex64", "chirp_medium_c64"), (1000, "complex128", "chirp_line_c128")]
_CHIRP_RUNS = {"fixed": dict(length=5, h=1.0, **workloads.SMF), "adaptive": dict(length=5, phi_max=0.004, **workloads.SMF)}


def _chirp_line_field(n):
    gv(**workloads.BENCH_GV)
    return workloads.qpsk_field(1 << 12, seed=21, power_w=5e-3)[:, :n]


@pytest.mark.parametrize("mode", ["fixed", "adaptive"])
@pytest.mark.parametrize("n,precision,engine", _CHIRP_LINES)
def test_any_length_return_steps_with_a_stride_and_with_positions(n, precision, engine, mode):
    """``return_steps`` on the chirp-z path (a step per call on the complex128 line), fixed and adaptive: ``every=3`` keeps rows 0, 3, ..., last of the plain
    ``return_steps`` call and ``z_list`` the first step that reaches each position -- below 0 (the input), between two steps, exactly on a step's z, beyond the
    length (the end field).  An adaptive run repeats bit for bit, so the bound is equality, ``z`` included."""
    x = optical_signal(_chirp_line_field(n))
    kw = dict(_CHIRP_RUNS[mode], precision=precision)
    z_all, A_all = oa.FIBER(x, return_steps=True, **kw)
    S = len(z_all) - 1
    assert (S == 5) if mode == "fixed" else (10 <= S <= 40), S
    assert A_all.shape == (S + 1, 2, n) and A_all.dtype == np.dtype(precision)
    keep = list(range(0, S, 3)) + [S]
    z3, A3 = oa.FIBER(x, return_steps=True, every=3, **kw)
    np.testing.assert_array_equal(z3, z_all[keep])
    np.testing.assert_array_equal(A3, A_all[keep])
    zl = [-1.0, 0.5 * (float(z_all[2]) + float(z_all[3])), float(z_all[4]), 7.0]
    idx = [next((k for k in range(S + 1) if z_all[k] >= v), S) for v in zl]
    assert idx == [0, 3, 4, S]
    zp, Ap = oa.FIBER(x, return_steps=True, z_list=zl, **kw)
    np.testing.assert_array_equal(zp, z_all[idx])
    np.testing.assert_array_equal(Ap, A_all[idx])


@pytest.mark.parametrize("mode", ["fixed", "adaptive"])
@pytest.mark.parametrize("n,precision,engine", _CHIRP_LINES)
def test_any_length_leaves_a_device_resident_input_as_it_was(n, precision, engine, mode):
    """The caller's array is never modified: a device-resident input reads back byte for byte the same after ``FIBER`` on each chirp-z line, given in the
    line's own type (the line works on a copy) and in the other one (on a cast)."""
    a = _chirp_line_field(n)
    for dtype in (np.complex64, np.complex128):
        x = _lib.DeviceArray.from_host(a.astype(dtype), dtype)
        before = x.to_host().tobytes()
        out = oa.FIBER(optical_signal.from_device(x), precision=precision, **_CHIRP_RUNS[mode])
        assert out.signal.shape == a.shape and np.isfinite(out.signal).all() and not np.array_equal(out.signal, a.astype(out.signal.dtype))
        assert x.to_host().tobytes() == before, (dtype, out.engine)


@pytest.mark.parametrize("mode", ["fixed", "adaptive"])
@pytest.mark.parametrize("n,precision,engine", _CHIRP_LINES)
def test_any_length_names_the_chirp_line_that_ran(n, precision, engine, mode):
    """``FIBER(...).engine`` on the three routes of the chirp-z path.  A one-launch route is skipped only where the environment sets a knob that governs
    it to the value that switches it off (the knob suite); every route it leaves on is still checked."""
    off = {"SSFM_CHIRP_LOOP": "python", "SSFM_FUSED_PATIENCE_TICKS": "-1"}
    if engine == "chirp_small_c64":
        off.update(SSFM_CHIRP_SMALL="0", SSFM_SMALL="0")
    elif engine == "chirp_medium_c64":
        off.update(SSFM_MEDIUM="0", **({"SSFM_MEDIUM_ADAPT": "0"} if mode == "adaptive" else {}))
    hit = {k: v for k, v in off.items() if os.environ.get(k) == v}
    if hit and engine != "chirp_line_c128":
        pytest.skip(f"the environment switches this one-launch engine off: {hit}")
    out = oa.FIBER(optical_signal(_chirp_line_field(n)), precision=precision, **_CHIRP_RUNS[mode])
    assert out.engine == engine, (out.engine, mode)


def test_lengths_beyond_the_range_are_rejected():
    gv(sps=16, R=10e9)
    with pytest.raises(ValueError, match="samples per polarisation"):
        oa.FIBER(optical_signal(np.ones((1 << 21) + 1, complex)), length=1, h=1.0)


# ----------------------------------------------------------------------- oracle, seeded inputs
@pytest.mark.parametrize("k,npol,steps", [(12, 1, 40), (15, 2, 25), (16, 2, 20), (17, 1, 12), (18, 2, 8), (19, 2, 5)])
def test_fixed_step_against_oracle(k, npol, steps):
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << k, seed=100 + k, n_pol=npol)
    a = a[0] if npol == 1 else a
    kw = dict(length=steps * 0.5, h=0.5, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    ref = orc.fiber_c64(a, gv.dt, **kw)
    assert y.shape == ref.shape
    assert within(y, ref, kw=kw, what="oracle")


def test_thousand_steps_against_oracle():
    """C2's step count (length=125, h=0.125 -> exactly 1000 float32 steps) at 2^13 x 2."""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 13, seed=2024)
    kw = dict(length=125, h=0.125, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    ref = orc.fiber_c64(a, gv.dt, **kw)
    assert within(y, ref, kw=kw, what="oracle, C2's schedule at 2^13 x 2")


@pytest.mark.parametrize("phi_max", [0.01, 0.05])
def test_adaptive_against_oracle(phi_max):
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 14, seed=7, power_w=10e-3)
    kw = dict(length=30, phi_max=phi_max, **workloads.SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    assert abs(len(z) - len(zr)) <= 1
    assert abs(z[-1] - 30.0) < 1e-4 and np.all(np.diff(z) > 0)
    # "the same bound after both reach z = L" -- the plain bound of the run's own step count, also on a +-1 mismatch
    # (rounds 1-5 allowed 5 x; the measured distance is 2e-6 ... 7e-6, profiles/r06_parity_margins.txt)
    assert within(A_z[-1], Ar[-1], steps=len(z) - 1, what=f"oracle adaptive, return_steps ({len(z) - 1} vs {len(zr) - 1} steps)")
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert within(y, Ar[-1], steps=len(zr) - 1, what="oracle adaptive")


def test_adaptive_gamma_zero_and_no_dispersion_single_step():
    gv(sps=16, R=10e9)
    a = workloads.qpsk_field(1 << 12, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for kw in (dict(length=10, alpha=0.2, beta_2=-20.0), dict(length=10, alpha=0.2, gamma=2.0)):
            z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
            zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
            np.testing.assert_array_equal(z, zr)
            assert len(z) == 2
            assert within(A_z[-1], Ar[-1], steps=1, what="oracle, single step")


def test_c128_against_oracle_dual_pol():
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 16, seed=11)
    kw = dict(length=10, h=1.0, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), precision="complex128", **kw).signal
    ref = orc.fiber_c128(a, gv.dt, **kw)
    assert within(y, ref, TOL_C128, kw=kw, what="float64 restatement")
    # and the complex64 path sits at the reference's float32 noise floor from it
    y32 = oa.FIBER(optical_signal(a), **kw).signal
    assert within(y32, ref, kw=kw, what="complex64 run against the float64 restatement")


@pytest.mark.parametrize("log2n, length", [(12, 20), (18, 3), (19, 2)])
def test_c128_adaptive_against_oracle(log2n, length):
    """(2^18 and 2^19: complex128 rows that form exp(D~ h) in the kernel run with 8 points per thread and their own copy of
    the operator, ssfm_host.hip `Ef_fly`; fixed steps with more step sizes than tables take the same rows)"""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << log2n, seed=12, power_w=10e-3)
    kw = dict(length=length, phi_max=0.05, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), precision="complex128", **kw).signal
    ref = orc.fiber_c128(a, gv.dt, **kw)
    assert within(y, ref, 1e-7)  # step sizes agree to rounding; splitting error tracks
    if log2n >= 18:
        hs = np.linspace(0.05, 0.35, 2 * length * 5 // 2)          # more distinct step sizes than operator tables
        hs = hs * (length / hs.sum())
        p = _lib.Plan(a.shape[-1], a.shape[0], _lib.C128)
        try:
            p.set_linear_operator(oa.devices.linear_operator(a.shape[-1], gv.dt, workloads.SMF["alpha"], workloads.SMF["beta_2"], workloads.SMF["beta_3"], _lib.C128))
            p.set_field(a)
            p.propagate_fixed(workloads.SMF["gamma"], hs)
            got = p.get_field()
        finally:
            p.close()
        D = orc.linear_operator_c128(a.shape[-1], gv.dt, workloads.SMF["alpha"], workloads.SMF["beta_2"], workloads.SMF["beta_3"])
        want = np.asarray(a, np.complex128)
        for h_ in hs:                                               # the loop of oracle/ssfm_numpy.fiber_c128 over a given schedule
            N_hat = 1j * workloads.SMF["gamma"] * np.abs(want) ** 2
            want = np.fft.ifft(np.fft.fft(want * np.exp(h_ / 2 * N_hat)) * np.exp(D * h_)) * np.exp(h_ / 2 * N_hat)
        assert within(got, want, TOL_C128)


# ----------------------------------------------------------------------- reference's own tests
def test_reference_test_FIBER_and_DBP():
    """tests/devices_test.py:257-277 of the reference, on the HIP path."""
    gv(sps=16, R=1e9)
    x = optical_signal(np.full(2048, np.sqrt(10e-3)))           # LASER(P0=10 dBm) CW
    y = oa.FIBER(x, length=10, alpha=0.2)
    assert isinstance(y, optical_signal)
    np.testing.assert_allclose(np.mean(np.abs(y.signal) ** 2), 10e-3 * np.exp(-0.2 / 4.343 * 10), rtol=1e-3)
    w = oa.DBP(oa.FIBER(x, 10), 10)
    np.testing.assert_allclose(w.signal, x.signal, atol=1e-5)
    d = oa.DM(x, 1000.0)
    assert isinstance(d, optical_signal) and d.size == x.size


# ----------------------------------------------------------------------- analytic properties
def test_pure_spm_closed_form():
    """beta = 0: one step of the whole length, A exp(-alpha L/2) exp(j gamma |A|^2 L) -- L, not L_eff
    (devices.py:1156,1177-1181)."""
    gv(sps=16, R=10e9)
    a = workloads.qpsk_field(1 << 12, seed=5, power_w=5e-3)
    L, al, g = 12.0, 0.2, 2.0
    y = oa.FIBER(optical_signal(a), length=L, alpha=al, gamma=g, precision="complex128").signal
    want = a * np.exp(-(al / 4.343) * L / 2) * np.exp(1j * g * np.abs(a) ** 2 * L)
    assert within(y, want, 1e-12)


def test_linear_fiber_equals_DM():
    """FIBER(gamma=0, alpha=0, beta_2) == DM(D = beta_2 L)."""
    gv(sps=16, R=10e9)
    a = workloads.qpsk_field(1 << 13, seed=6)
    y = oa.FIBER(optical_signal(a), length=40, beta_2=-20.0, precision="complex128").signal
    d = oa.DM(optical_signal(a), D=-20.0 * 40).signal
    assert within(y, d, 1e-11)


# ----------------------------------------------------------------------- full benchmark size
def _bench_field():
    gv(**workloads.BENCH_GV)
    return workloads.qpsk_field(1 << 20, seed=2024)


def test_full_size_against_oracle_few_steps():
    """2^20 x 2 complex64, C2's step size, 6 steps (the oracle needs ~1 s per step)."""
    a = _bench_field()
    kw = dict(length=6 * 0.125, h=0.125, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    ref = orc.fiber_c64(a, gv.dt, **kw)
    assert within(y, ref, kw=kw, what="oracle, 2^20 x 2")


def test_full_size_properties_1000_steps():
    """C2 in full (2^20 x 2, 1000 steps): energy follows exp(-alpha L) (the nonlinear and the
    dispersive operators are unitary), polarisations stay independent, and the result agrees
    with the complex128 run."""
    a = _bench_field()
    kw = dict(length=125, h=0.125, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    e_in = np.sum(np.abs(a) ** 2, axis=-1)
    e_out = np.sum(np.abs(y.astype(np.complex128)) ** 2, axis=-1)
    # per step the amplitude is multiplied by the float32 value of exp(-alpha/2 h) (devices.py:1179)
    att = np.exp(np.complex64(-np.float32(0.2 / 4.343) / 2) * np.float32(0.125)).real
    np.testing.assert_allclose(e_out / e_in, float(att) ** 2000, rtol=1e-4)
    y0 = oa.FIBER(optical_signal(a[0]), **kw).signal                     # one polarisation alone
    np.testing.assert_array_equal(y0, y[0])
    y128 = oa.FIBER(optical_signal(a), precision="complex128", **kw).signal
    assert within(y, y128, kw=kw, what="complex64 run against the complex128 run, C2")


def test_full_size_c2_against_the_strided_fixture(golden_dir):
    """Configuration C2 itself (2^20 x 2, complex64, 1000 steps) against the committed full-size fixture: every 257th
    sample, the per-polarisation power and the total energy of the oracle's run (tests/golden/make_c2_strided.py)."""
    g = np.load(os.path.join(golden_dir, "c2_full_strided.npz"))
    y = oa.FIBER(optical_signal(_bench_field()), length=125, h=0.125, **workloads.SMF).signal
    assert y.shape == (2, 1 << 20) and y.dtype == np.complex64
    assert within(y[:, ::257], g["samples"], steps=1000, what="C2 full size, the oracle's strided fixture")
    y2 = np.abs(y.astype(np.complex128)) ** 2
    np.testing.assert_allclose(np.mean(y2, axis=-1), g["power"], rtol=1e-4)
    np.testing.assert_allclose(np.sum(y2), float(g["energy"]), rtol=1e-4)


def test_full_size_c1_against_the_strided_fixture(golden_dir):
    """Configuration C1 (2^20 x 2, complex128, 100 x 1 km) against the float64 restatement's full-size run."""
    g = np.load(os.path.join(golden_dir, "c1_full_strided.npz"))
    y = oa.FIBER(optical_signal(_bench_field()), length=100, h=1.0, precision="complex128", **workloads.SMF).signal
    assert y.shape == (2, 1 << 20) and y.dtype == np.complex128
    assert within(y[:, ::257], g["samples"], TOL_C128, steps=100, what="C1 full size, the float64 restatement's strided fixture")
    np.testing.assert_allclose(np.mean(np.abs(y) ** 2, axis=-1), g["power"], rtol=1e-11)
    np.testing.assert_allclose(np.sum(np.abs(y) ** 2), float(g["energy"]), rtol=1e-11)


def test_full_size_c3_batch_and_c4_chain():
    """C3 at full size: 4 WDM channels of 2^20 x 2 batched in one plan are bit-identical to 4 separate FIBER calls.
    C4 at full size: FIBER then DBP of a PRBS realisation on the device against the oracle's chain (4 + 4 steps)."""
    from opticomlib_amd import dist as od
    gv(**workloads.BENCH_GV)
    n = 1 << 20
    fields = np.stack([workloads.qpsk_field(n, seed=3000 + c) for c in range(4)]).astype(np.complex64)
    kw = dict(length=5, h=0.125, **workloads.SMF)                       # 40 of C2's steps
    outs = od.propagate_channels(fields, gv.dt, **kw)
    for c in (0, 3):
        np.testing.assert_array_equal(outs[c], oa.FIBER(optical_signal(fields[c]), **kw).signal)
    a = workloads.prbs_field(n, seed=7, power_w=1e-3)
    kw4 = dict(length=4, h=1.0, **workloads.SMF)
    got = od.propagate_channels(np.stack([a, a]), gv.dt, dbp=True, **kw4)[1]
    ref = orc.dbp_c64(orc.fiber_c64(a, gv.dt, **kw4), gv.dt, **kw4)
    assert within(got, ref, steps=2 * steps_of(kw4), what="oracle FIBER + DBP, 2^20 x 2")


def test_full_size_c128_100_steps_roundtrip_structure():
    """C1 (2^20 x 2, complex128, 100 x 1 km): FIBER then DBP returns the input up to the known
    stale-N^ asymmetry, and linear-only propagation is exactly invertible."""
    a = _bench_field()
    lin = dict(length=100, h=1.0, alpha=0.2, beta_2=-21.7, beta_3=0.13)
    y = oa.FIBER(optical_signal(a), precision="complex128", **lin)
    back = oa.DBP(y, precision="complex128", **lin).signal
    assert within(back, a, 1e-10)
    kw = dict(length=100, h=1.0, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), precision="complex128", **kw)
    back = oa.DBP(y, precision="complex128", **kw).signal
    assert 1e-7 < relmax(back, a) < 5e-2


# ----------------------------------------------------------------------- LPF / BPF
TOL_FILT = 1e-11      # float64 recursion; chunked start states differ from the serial loop at the 1e-16 level


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["func"] in ("LPF", "BPF")])
def test_bessel_filters_golden(golden_dir, name):
    from opticomlib_amd.typing import electrical_signal
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gv(**case["gv"])
    sig, noi = case_input(case)
    kw = dict(case["kw"])
    if case["func"] == "LPF":
        x = electrical_signal(sig) if noi is None else electrical_signal(sig, noi)
        r = oa.LPF(x, **kw)
        if kw.get("retH"):
            y, H = r
            np.testing.assert_allclose(H, g["H"], rtol=1e-12, atol=1e-15)
        else:
            y = r
        assert isinstance(y, electrical_signal) and y.signal.dtype == np.float64
    else:
        x = optical_signal(sig) if noi is None else optical_signal(sig, noi)
        y = oa.BPF(x, **kw)
        assert isinstance(y, optical_signal) and y.n_pol == x.n_pol and y.signal.dtype == np.complex128
    assert y.signal.shape == g["out"].shape
    assert within(y.signal, g["out"], TOL_FILT)
    if "out_noise" in g:
        assert within(y.noise, g["out_noise"], TOL_FILT)
    else:
        assert y.noise is NULL


def test_bessel_filters_full_size_against_oracle_and_scipy():
    """2^20 x 2 complex BPF and 2^20 real LPF: the restated loop (oracle) on a 2^14 slice-sized case and
    SciPy's own sosfiltfilt (the reference's dependency) at full size."""
    from scipy import signal as sg
    from oracle import filters_numpy as fo
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 20, seed=77)
    y = oa.BPF(optical_signal(a), BW=60e9).signal
    sos, zi = fo.bessel_sos(4, 30e9, gv.fs)
    assert within(y, sg.sosfiltfilt(sos, a, axis=-1), TOL_FILT)
    p = np.abs(a[0]) ** 2
    z = oa.LPF(p, BW=20e9).signal
    sos, zi = fo.bessel_sos(4, 20e9, gv.fs)
    assert within(z, sg.sosfiltfilt(sos, p), TOL_FILT)
    b = workloads.qpsk_field(1 << 14, seed=78)
    out, _ = fo.bpf(b, 60e9, gv.fs)
    assert within(oa.BPF(optical_signal(b), BW=60e9).signal, out, TOL_FILT)


@pytest.mark.parametrize("order", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("n", [16, 31, 32, 33, 994, 995, 2047, 2048, 2049, 4066, 4067, 65599, (1 << 17) + 1])
def test_sosfiltfilt_lengths_and_orders_against_scipy(order, n):
    """Chunk (16), wavefront (64 chunks) and group (256 chunks) boundaries, odd lengths and every section count
    against SciPy's sosfiltfilt (the reference's dependency, devices.py:1365-1368)."""
    from scipy import signal as sg
    sos = sg.bessel(order, 0.07 if n > 4096 else 0.2, "low", norm="mag", output="sos")
    zi = sg.sosfilt_zi(sos)
    ntaps = 2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    if n <= 3 * ntaps:
        with pytest.raises(ValueError, match="greater than padlen"):          # SciPy raises ValueError for the same call
            _lib.sosfiltfilt(sos, zi, np.ones(n))
        return
    rng = np.random.default_rng(order * 1000 + n)
    x = rng.standard_normal(n).cumsum() * 0.05 + rng.standard_normal(n)
    assert within(_lib.sosfiltfilt(sos, zi, x), sg.sosfiltfilt(sos, x), TOL_FILT)
    xc = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n)))
    assert within(_lib.sosfiltfilt(sos, zi, xc), sg.sosfiltfilt(sos, xc, axis=-1), TOL_FILT)


@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
@pytest.mark.parametrize("log2n", [8, 9, 10, 11, 12, 13])
def test_single_launch_engine_against_the_two_kernel_engine(log2n, prec, monkeypatch):
    """Plans of up to 8192 samples run a fixed-step schedule in ONE launch (ssfm_kernels.hpp k_small: a workgroup keeps a row
    in registers); SSFM_SMALL=0 at plan creation selects the two-kernel engine for the same plan shape.  Same arithmetic per
    step, another FFT factorisation: agreement at rounding level, and both against the oracle."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(log2n)
    a = ((rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))) * 0.05).astype(np.complex64 if prec == _lib.C64 else np.complex128)
    hs = np.array([0.5] * 7 + [0.25, 0.5, 0.125, 0.5, 0.5, 0.03125], dtype=np.float32 if prec == _lib.C64 else np.float64)   # 4 distinct sizes
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec)
    got = {}
    monkeypatch.delenv("SSFM_FORCE_FLY", raising=False)               # (that diagnostic knob takes the tables, and with them this engine, away)
    monkeypatch.setenv("SSFM_MEDIUM", "0")                            # (8192 samples: k_small against the two-kernel engine, not the one-XCD engine)
    for small in ("1", "0"):
        monkeypatch.setenv("SSFM_SMALL", small)
        p = _lib.Plan(n, 3, prec)
        try:
            p.set_linear_operator(D)
            for rep in range(2):                                   # second run: cached tables, reused schedule buffer
                p.set_field(a)
                p.propagate_fixed(1.3, hs)
            got[small] = p.get_field()
            launches = p.last_propagate_ms()[1]
        finally:
            p.close()
        single = n <= (8192 if prec == _lib.C64 else 4096)
        assert launches == (1 if small == "1" and single else 1 + 2 * hs.size)
    tol = 2e-6 if prec == _lib.C64 else 1e-12
    assert within(got["1"], got["0"], tol, steps=hs.size, what="one-launch engine against the two-kernel engine")
    if prec == _lib.C128:
        Dn = orc.linear_operator_c128(n, gv.dt, 0.2, -21.7, 0.13)
        want = a.copy()
        for h_ in hs:
            N_hat = 1j * 1.3 * np.abs(want) ** 2
            want = np.fft.ifft(np.fft.fft(want * np.exp(h_ / 2 * N_hat), axis=-1) * np.exp(Dn * h_), axis=-1) * np.exp(h_ / 2 * N_hat)
        assert within(got["1"], want, TOL_C128, steps=hs.size, what="float64 restatement, step by step")
    else:
        Dc = orc.linear_operator_c64(n, gv.dt, 0.2, -21.7, 0.13)
        want = a.copy()
        for h_ in hs:
            want = orc.ssfm_step_c64(want, Dc, np.float32(1.3), np.float32(h_))
        assert within(got["1"], want, steps=hs.size, what="oracle, step by step")


@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
@pytest.mark.parametrize("log2n, rows", [(8, 1), (8, 2), (10, 2), (11, 2), (12, 1), (12, 2), (13, 1), (13, 2)])
def test_single_launch_adaptive_run_against_the_chunked_engine(log2n, rows, prec, monkeypatch):
    """Adaptive runs of small plans are ONE launch (k_small_adapt: all rows in one workgroup, step control between the
    inverse transform and the rotation); SSFM_SMALL=0 at plan creation gives the chunked three-kernel engine.  Same step
    rule: the z logs agree to rounding of |A|^2, the fields at rounding level, and a budgeted caller gets the chunked engine."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=40 + log2n, power_w=10e-3)[:rows]
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec)
    single = rows * n // (16 if (prec == _lib.C64 and n >= 4096) else 8) <= 512 and n <= 4096
    res = {}
    monkeypatch.setenv("SSFM_MEDIUM_ADAPT", "0")                      # (4096 x 2 and 8192: this test is about k_small_adapt and the chunked engine)
    for small in ("1", "0"):
        monkeypatch.setenv("SSFM_SMALL", small)
        p = _lib.Plan(n, rows, prec)
        try:
            p.set_linear_operator(D)
            for rep in range(2):
                p.set_field(a)
                steps, z, _ = p.propagate_adaptive(1.3, 6.0, 0.02, False)
            res[small] = (steps, z, p.get_field(), p.last_propagate_ms()[1])
            if small == "1":                                      # same plan, 5 steps per call: the chunked engine
                p.set_field(a)
                lib = _lib.load()
                st, dn = _lib._I64(0), _lib._I(0)
                _lib._check(lib.ssfm_adaptive_begin(p._h, 1.3, 6.0, 0.02, 0, 1 << 16, 0), "begin")
                while not dn.value:
                    _lib._check(lib.ssfm_adaptive_run(p._h, 5, None, _lib.C.byref(st), _lib.C.byref(dn)), "run")
                zb = np.zeros(st.value + 1)
                _lib._check(lib.ssfm_adaptive_finish(p._h, _lib.C.byref(st), zb.ctypes.data_as(_lib.C.POINTER(_lib._D))), "finish")
                res["budget"] = (st.value, zb, p.get_field())
        finally:
            p.close()
    s1, z1, f1, l1 = res["1"]
    s0, z0, f0, l0 = res["0"]
    assert l1 == (1 if single else l0) and l0 > 3
    assert s1 > 3 and abs(s1 - s0) <= 1 and abs(z1[-1] - 6.0) < 1e-5
    k = min(s1, s0, 12)
    np.testing.assert_allclose(z1[:k], z0[:k], rtol=2e-6 if prec == _lib.C64 else 1e-12)
    # two engines of this library on the same adaptive run (both within tol of the oracle: test_adaptive_*): the plain bound of the run's step count
    assert within(f1, f0, (tol_at(max(s1, s0)) if prec == _lib.C64 else 1e-9), steps=s1, what=f"one-launch adaptive engine against the chunked engine ({s1} vs {s0} steps)")
    sb, zb, fb = res["budget"]
    assert sb == s0 and np.array_equal(zb, z0) and np.array_equal(fb, f0)
    if prec == _lib.C128:
        ref = orc.fiber_c128(a if rows > 1 else a[0], gv.dt, 6.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.02)
        assert within(f1, ref, 1e-7, steps=s1, what="float64 restatement, adaptive")
    else:
        zo, Ao = orc.fiber_c64(a if rows > 1 else a[0], gv.dt, 6.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.02, return_steps=True)
        assert abs(len(zo) - 1 - s1) <= 1
        assert within(f1 if rows > 1 else f1[0], Ao[-1], steps=s1, what=f"oracle adaptive ({s1} vs {len(zo) - 1} steps)")


@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
@pytest.mark.parametrize("log2n, rows", [(9, 1), (9, 2), (10, 1), (11, 1)])
def test_single_launch_adaptive_run_at_the_other_sizes_against_oracle(log2n, rows, prec, monkeypatch):
    """k_small_adapt at the sizes and row counts the test above leaves out -- 512 samples with one row and with two, 1024 and 2048 with one: the whole run in
    one launch, named by the plan, against the float64 restatement of the run at the bound of its step count."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=40 + log2n, power_w=10e-3)[:rows]
    monkeypatch.setenv("SSFM_SMALL", "1")
    p = _lib.Plan(n, rows, prec)
    try:
        p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec))
        p.set_field(a)
        steps, z, _ = p.propagate_adaptive(1.3, 6.0, 0.008, False)
        f, info, launches = p.get_field(), p.last_run_info(), p.last_propagate_ms()[1]
    finally:
        p.close()
    assert info["engine"] == "small_adaptive" and not info["fell_back"] and launches == 1, (info, launches)
    assert 10 <= steps <= 20 and abs(z[-1] - 6.0) < 1e-5, steps
    ref = orc.fiber_c128(a if rows > 1 else a[0], gv.dt, 6.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.008)
    assert within(f if rows > 1 else f[0], ref, steps=steps, what=f"float64 restatement, adaptive ({steps} steps)")


@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
def test_single_launch_capture_against_the_two_kernel_engine(prec, monkeypatch):
    """return_steps on a small plan: the single launch writes the field after every step between its two half rotations
    (what k_time<END> hands to the capture of the two-kernel engine)."""
    n = 2048
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=5, power_w=5e-3)
    hs = np.array([0.5, 0.5, 0.25, 0.5, 0.125, 0.5, 0.5], dtype=np.float32 if prec == _lib.C64 else np.float64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec)
    got = {}
    monkeypatch.delenv("SSFM_FORCE_FLY", raising=False)
    for small in ("1", "0"):
        monkeypatch.setenv("SSFM_SMALL", small)
        p = _lib.Plan(n, 2, prec)
        try:
            p.set_linear_operator(D)
            p.set_field(a)
            snaps = p.propagate_fixed(1.3, hs, snapshots=True)
            got[small] = (np.array(snaps), p.get_field(), p.last_propagate_ms()[1])
        finally:
            p.close()
    s1, f1, l1 = got["1"]
    s0, f0, l0 = got["0"]
    assert l1 == 1 and l0 > hs.size and s1.shape == (hs.size + 1, 2, n) == s0.shape
    np.testing.assert_array_equal(s1[0], a.astype(s1.dtype))
    np.testing.assert_array_equal(s1[-1], f1)
    tol = 2e-6 if prec == _lib.C64 else 1e-12
    for k in range(1, hs.size + 1):
        assert within(s1[k], s0[k], tol, steps=k, what="one-launch capture against the two-kernel engine")
    assert within(f1, f0, tol, steps=hs.size, what="one-launch capture against the two-kernel engine, end field")


@pytest.mark.parametrize("log2n, rows", [(14, 1), (14, 2), (15, 1), (15, 2), (16, 1), (16, 2), (17, 1), (17, 2), (16, 4)])
def test_medium_single_launch_engine_against_the_two_kernel_engine(log2n, rows, monkeypatch):
    """complex64 plans of up to 2^17 samples in all (2^14 x 1..4, 2^15 x 1..4, 2^16 x 1..2, 2^17 x 1) run a fixed-step schedule in ONE launch
    (ssfm_kernels.hpp k_medium: the passes of the two-kernel engine separated by barriers, all workgroups on one XCD and meeting in its L2);
    SSFM_MEDIUM=0 at plan creation, or a larger plan, keeps the two-kernel engine.  The same passes on the same data: bit-identical
    fields, repeatedly (a stale read of another workgroup's data would show here); and against the oracle."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(100 + log2n)
    a = ((rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) * 0.05).astype(np.complex64)
    hs = np.array([0.5] * 30 + [0.25, 0.5, 0.125, 0.5, 0.5, 0.03125], dtype=np.float32)      # 4 distinct sizes
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS", raising=False)
    monkeypatch.delenv("SSFM_FORCE_FLY", raising=False)
    monkeypatch.delenv("SSFM_E", raising=False)
    monkeypatch.delenv("SSFM_MEDIUM_SPLIT", raising=False)
    got = {}
    for med in ("1", "0"):
        monkeypatch.setenv("SSFM_MEDIUM", med)
        p = _lib.Plan(n, rows, _lib.C64)
        try:
            p.set_linear_operator(D)
            outs = []
            for rep in range(3):
                p.set_field(a)
                p.propagate_fixed(1.3, hs if rep != 1 else hs[:7])
                outs.append((p.get_field(), p.last_propagate_ms()[1]))
                # which engine REALLY ran (a one-launch run that gave up would have been repeated on the two-kernel engine behind our back)
                one_launch = med == "1" and ((n if (rows == 2 and log2n >= 16) else n * rows) <= (1 << 17))
                info = p.last_run_info()
                assert info["engine"] == ("medium" if one_launch else "two_kernel") and not info["fell_back"] and info["fallbacks_total"] == 0, info
            got[med] = outs
        finally:
            p.close()
    for (f1, l1), (f0, l0) in zip(got["1"], got["0"]):
        split = rows == 2 and log2n >= 16                           # a dual-polarisation plan of long rows: one launch per row, on two XCDs
        assert l0 > 10 and (l1 == (2 if split else 1) if (n if split else n * rows) <= (1 << 17) else l1 == l0)
        np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(got["1"][0][0], got["1"][2][0])
    # every size against the oracle directly (a few seconds of CPU at 2^17 samples)
    A = a.copy()
    for h_ in hs:
        A = orc.ssfm_step_c64(A, orc.linear_operator_c64(n, gv.dt, 0.2, -21.7, 0.13), np.float32(1.3), h_)
    assert within(got["1"][0][0], A, steps=hs.size, what="oracle, step by step")


@pytest.mark.parametrize("log2n, rows, phase", [(12, 2, "1"), (12, 2, "0"), (13, 1, "0"), (14, 1, "0"), (15, 1, "0"), (16, 1, "0"), (17, 1, "0")])
def test_medium_single_launch_engine_on_its_smallest_shape_and_with_value_tables_against_oracle(log2n, rows, phase, monkeypatch):
    """k_medium where the tests above do not take it: the 64 x 64 shape (2^12 samples x 2 rows, which k_small takes unless SSFM_SMALL=0) with either kind
    of operator table, and the five larger shapes with tables of values (SSFM_PHASE_TABLE=0; a fibre's operator gets phase tables otherwise).  Fifteen
    steps of three sizes in one launch, named by the plan, against the float64 restatement step by step."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(100 + log2n)
    a = ((rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) * 0.05).astype(np.complex64)
    hs = np.array([0.5] * 12 + [0.25, 0.5, 0.125], dtype=np.float32)
    for k in ("SSFM_FUSED_PATIENCE_TICKS", "SSFM_FORCE_FLY", "SSFM_E", "SSFM_EF", "SSFM_MEDIUM_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SSFM_SMALL", "0")
    monkeypatch.setenv("SSFM_MEDIUM", "1")
    monkeypatch.setenv("SSFM_PHASE_TABLE", phase)
    p = _lib.Plan(n, rows, _lib.C64)
    try:
        p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13))
        p.set_field(a)
        p.propagate_fixed(1.3, hs)
        f, info, launches = p.get_field(), p.last_run_info(), p.last_propagate_ms()[1]
    finally:
        p.close()
    assert info["engine"] == "medium" and not info["fell_back"] and launches == 1, (info, launches)
    Dn = orc.linear_operator_c128(n, gv.dt, 0.2, -21.7, 0.13)
    want = a.astype(np.complex128)
    for h_ in hs.astype(np.float64):
        N_hat = 1j * 1.3 * np.abs(want) ** 2
        want = np.fft.ifft(np.fft.fft(want * np.exp(h_ / 2 * N_hat), axis=-1) * np.exp(Dn * h_), axis=-1) * np.exp(h_ / 2 * N_hat)
    assert within(f, want, steps=hs.size, what="float64 restatement, step by step")


def test_a_stream_ordered_consumer_never_sees_a_run_that_gave_up(tmp_path):
    """include/ssfm_amd.h "WHEN THE FIELD IS VALID": a caller that has asked for the plan's stream may order its own work behind
    ssfm_propagate_fixed without ssfm_synchronize.  The one-launch engine of medium plans only knows at its end whether its workgroups met;
    with no patience at all (SSFM_FUSED_PATIENCE_TICKS=-1) they give up, and the call itself must already have repeated the run on the
    two-kernel engine: a copy queued on the plan's stream right behind the call holds the right field, and the run info says what happened
    (examples/stream_ordered_consumer.cpp, built with hipcc: the consumer is a HIP program of its own)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "stream_ordered_consumer")
    libdir = os.path.join(root, "opticomlib_amd")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "stream_ordered_consumer.cpp"), "-o", exe,
                    "-L" + libdir, "-l:_ssfm_amd.so", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SSFM_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "engine 1 fell_back 1 fallbacks 1; stream-ordered copy equals the two-kernel result" in r.stdout


def test_strided_capture_golden_and_against_every_step(golden_dir):
    """``FIBER(return_steps=True, every=k)`` (ssfm_propagate_fixed_capture): the reference's return_steps golden vector sub-sampled, and -- bit for bit -- the
    rows of this library's own every-step capture; strides that divide the run, that do not, and one longer than the run."""
    g = np.load(os.path.join(golden_dir, "return_steps_1k.npz"))
    spec = CASES["return_steps_1k"]
    x = _signal(spec)
    kw = dict(spec["kw"])
    kw.pop("return_steps")
    z_all, A_all = oa.FIBER(x, return_steps=True, **kw)
    np.testing.assert_array_equal(z_all, g["z"])
    for every in (1, 2, 3, 5, 7):
        z, A_z = oa.FIBER(x, return_steps=True, every=every, **kw)
        keep = list(range(0, 5, every)) + [5]
        assert A_z.dtype == np.complex64 and A_z.shape == (len(keep),) + A_all.shape[1:]
        np.testing.assert_array_equal(z, g["z"][keep])
        assert within(A_z, g["A_z"][keep], steps=5, what=f"golden return_steps, every={every}")
        # the every-step capture of a plan this small is taken by the one-launch engine, the strided one by the two-kernel engine: the same arithmetic class
        assert within(A_z, A_all[keep], 2e-6, steps=5, what="strided capture against this library's every-step capture")


@pytest.mark.parametrize("prec,log2n,npol", [("c128", 16, 2), ("c128", 20, 2), ("c128", 12, 1), ("c64", 10, 1)])
def test_strided_capture_on_plans_whose_engine_works_in_place(prec, log2n, npol):
    """complex128 plans and the complex64 plans outside the unit layout transform the field buffer in place: their first launch overwrites the input, which
    the capture therefore copies ahead of the run (found by tests/diag/capture_stress.py: the input snapshot of such plans raced with the run).  Input,
    snapshots, end field and the scalar log, with and without the log, twice on the same plan."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    P, dt, rt, tol = (_lib.C128, np.complex128, np.float64, 1e-10) if prec == "c128" else (_lib.C64, np.complex64, np.float32, 5e-6)
    a = workloads.qpsk_field(n, seed=41, n_pol=2)[:npol].astype(dt)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(10, 0.05, dtype=rt)
    p = _lib.Plan(n, npol, P)
    try:
        p.set_linear_operator(D)
        for log in (False, True, False):
            p.set_field(a)
            cap = p.propagate_fixed_capture(1.3, hs, every=3, scalars=log)
            end = p.get_field()
            assert list(cap["steps"]) == [0, 3, 6, 9, 10]
            np.testing.assert_array_equal(cap["fields"][0], a)
            np.testing.assert_array_equal(cap["fields"][-1], end)
            for k, s_ in enumerate(cap["steps"][1:], start=1):
                p.set_field(a); p.propagate_fixed(1.3, hs[:s_]); p.synchronize()
                if p.last_run_info()["engine"] == "two_kernel" and not log:
                    np.testing.assert_array_equal(cap["fields"][k], p.get_field())
                else:
                    assert within(cap["fields"][k], p.get_field(), tol, steps=s_, what="snapshot against a plain run of that many steps")
            if log:
                power = np.mean(np.abs(cap["fields"].astype(np.complex128)) ** 2, axis=-1)
                np.testing.assert_allclose(cap["power"][cap["steps"]], power, rtol=1e-12 if prec == "c128" else 5e-6)
    finally:
        p.close()


@pytest.mark.parametrize("log2n,nsteps,every,check", [(14, 400, 1, (1, 33, 257, 399)), (20, 24, 2, (2, 12, 18, 22))])
def test_strided_capture_with_more_snapshots_than_device_blocks(log2n, nsteps, every, check):
    """The snapshots between the input and the end wait in a ring of at most eight device blocks (32 snapshots of a 2^14 x 2 field each, one of a 2^20 x 2
    field) that the helper thread empties while the run goes on: a run with more flushes than blocks writes blocks again -- every snapshot is still the
    plain run's of that many steps, bit for bit (spot-checked), and all of them follow the every-step capture of the three-launch form."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=37, n_pol=2).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(nsteps, 0.05, dtype=np.float32)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D)
        p.set_field(a)
        cap = p.propagate_fixed_capture(1.3, hs, every=every)
        end = p.get_field()
        assert len(cap["steps"]) == nsteps // every + 1 and len(cap["steps"]) - 2 > 8 * (32 if log2n == 14 else 1)
        np.testing.assert_array_equal(cap["fields"][0], a)
        np.testing.assert_array_equal(cap["fields"][-1], end)
        for s_ in check:
            p.set_field(a); p.propagate_fixed(1.3, hs[:s_]); p.synchronize()
            if p.last_run_info()["engine"] == "two_kernel":
                np.testing.assert_array_equal(cap["fields"][s_ // every], p.get_field())
            else:                                                    # (plans the one-launch engines take: another order of the same operations, up to 399 steps)
                assert within(cap["fields"][s_ // every], p.get_field(), 0.5 * tol_at(s_), steps=s_, what="snapshot (two-kernel engine) against a plain run (one-launch engine)")
        if log2n == 14:
            p.set_field(a)
            every_step = p.propagate_fixed(1.3, hs, snapshots=True)
            assert within(cap["fields"], every_step[cap["steps"]], 0.5 * tol_at(nsteps), steps=nsteps, what="strided capture against the every-step capture, all snapshots")
        # a second capture run on the same plan right behind the first (the helper of the first is joined by the next call on the plan)
        p.set_field(a)
        again = p.propagate_fixed_capture(1.3, hs, every=every)
        np.testing.assert_array_equal(again["fields"], cap["fields"])
    finally:
        p.close()


def _capture_against_plain_runs(p, a, hs, cap, check):
    """Snapshot s_ of an every-step strided capture against a plain run of s_ steps: bit for bit where that run is the two-kernel engine's."""
    for s_ in check:
        p.set_field(a); p.propagate_fixed(1.3, hs[:s_]); p.synchronize()
        if p.last_run_info()["engine"] == "two_kernel":
            np.testing.assert_array_equal(cap["fields"][s_], p.get_field())
        else:
            assert within(cap["fields"][s_], p.get_field(), 0.5 * tol_at(s_), steps=s_, what="snapshot (two-kernel engine) against a plain run (one-launch engine)")


@pytest.mark.parametrize("nsteps", [33, 34, 257, 258])
def test_strided_capture_at_the_seams_of_the_ring(nsteps):
    """The ring of a 2^14 x 2 complex64 capture (256 KiB per field) is eight blocks of 32 snapshots (ssfm_capture.hpp CapRing).  With a snapshot at every step,
    33 / 34 / 257 / 258 steps leave 32 / 33 / 256 / 257 snapshots between the input and the end field: one block exactly, one snapshot into a second block,
    the ring exactly full, and the first block written again behind its wait.  Input and end field bit for bit, all snapshots against the plan's own
    every-step capture, and the snapshots on either side of each seam against plain runs of that many steps."""
    n = 1 << 14
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=37, n_pol=2).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(nsteps, 0.05, dtype=np.float32)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D)
        p.set_field(a)
        cap = p.propagate_fixed_capture(1.3, hs, every=1)
        end = p.get_field()
        assert list(cap["steps"]) == list(range(nsteps + 1))
        np.testing.assert_array_equal(cap["fields"][0], a)
        np.testing.assert_array_equal(cap["fields"][-1], end)
        p.set_field(a)
        every_step = p.propagate_fixed(1.3, hs, snapshots=True)
        assert within(cap["fields"], every_step, 0.5 * tol_at(nsteps), steps=nsteps, what="strided capture against the every-step capture, all snapshots")
        _capture_against_plain_runs(p, a, hs, cap, [s_ for s_ in (32, 33, 256, 257) if s_ <= nsteps])
    finally:
        p.close()


@pytest.mark.parametrize("nsteps", [9, 10])
def test_strided_capture_of_two_lanes_at_the_seams_of_the_ring(nsteps, monkeypatch):
    """Two lanes fill the ring: a 2^19 x 2 complex64 field is 8 MiB, one snapshot per block, eight blocks.  With a snapshot at every step, 9 steps fill the
    ring exactly and 10 write its first block again -- both lanes' threads wait for the same transfer.  Every snapshot against a plain run."""
    n = 1 << 19
    gv(**workloads.BENCH_GV)
    monkeypatch.setenv("SSFM_LANES", "2")
    a = workloads.qpsk_field(n, seed=31, n_pol=2).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(nsteps, 0.05, dtype=np.float32)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        assert p.lanes == 2
        p.set_linear_operator(D)
        p.set_field(a)
        cap = p.propagate_fixed_capture(1.3, hs, every=1)
        end = p.get_field()
        assert list(cap["steps"]) == list(range(nsteps + 1))
        np.testing.assert_array_equal(cap["fields"][0], a)
        np.testing.assert_array_equal(cap["fields"][-1], end)
        _capture_against_plain_runs(p, a, hs, cap, range(1, nsteps + 1))
    finally:
        p.close()


@pytest.mark.parametrize("log2n,npol,lanes", [(14, 2, 1), (16, 1, 1), (19, 2, 2), (20, 2, 2)])
def test_strided_capture_and_scalar_log_against_the_plain_run(log2n, npol, lanes, monkeypatch):
    """ssfm_propagate_fixed_capture at the plan level, one lane and two: every snapshot is bit for bit the field a plain run of that many steps leaves (the same
    kernels in the same order: a capture step only splits the column launch), the run's end is the plain run's end, and the scalar log -- power and peak of
    every row after every step, accumulated inside the column kernels -- agrees with the snapshots' own."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    monkeypatch.setenv("SSFM_LANES", str(lanes))
    a = workloads.qpsk_field(n, seed=31, n_pol=2)[:npol].astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.array([0.25] * 22 + [0.125], dtype=np.float32)
    p = _lib.Plan(n, npol, _lib.C64)
    try:
        assert p.lanes == lanes
        p.set_linear_operator(D)
        p.set_field(a)
        cap = p.propagate_fixed_capture(1.3, hs, every=5)
        end = p.get_field()
        assert list(cap["steps"]) == [0, 5, 10, 15, 20, 23] and p.last_run_info()["engine"] == "two_kernel"
        np.testing.assert_array_equal(cap["fields"][0], a)
        np.testing.assert_array_equal(cap["fields"][-1], end)
        for k, s_ in enumerate(cap["steps"][1:], start=1):
            p.set_field(a); p.propagate_fixed(1.3, hs[:s_]); p.synchronize()
            want = p.get_field()
            if p.last_run_info()["engine"] == "two_kernel":
                np.testing.assert_array_equal(cap["fields"][k], want)
            else:                                                    # (plans the one-launch engines take: another order of the same operations)
                assert within(cap["fields"][k], want, 5e-6, steps=s_, what="snapshot against a plain run (one-launch engine)")
        # with the scalar log the column kernels are another instantiation (the log is a template parameter, so that every other run keeps its kernels to the
        # last instruction): the same operations, fields equal to the last bits of a fused product
        p.set_field(a)
        log = p.propagate_fixed_capture(1.3, hs, every=5, scalars=True)
        assert within(log["fields"], cap["fields"], 0.5 * TOL_100, steps=23, what="capture with the scalar log against the capture without")  # (two roundings of the same 23 steps: the distance two engines of this library keep)
        cap = log
        power = np.mean(np.abs(cap["fields"].astype(np.complex128)) ** 2, axis=-1)
        peak = np.max(np.abs(cap["fields"].astype(np.complex128)) ** 2, axis=-1)
        assert cap["power"].shape == (24, npol) and cap["peak"].shape == (24, npol)
        np.testing.assert_allclose(cap["power"][cap["steps"]], power, rtol=5e-6)         # (the log sums |A|^2 in float32, as the kernels hold it)
        np.testing.assert_allclose(cap["peak"][cap["steps"]], peak, rtol=2e-6)
        assert np.all(np.diff(cap["power"], axis=0) < 0)              # 0.2 dB/km: the power falls at every step
        # scalars alone: no field leaves the device, the run is the plain run
        p.set_field(a)
        only = p.propagate_fixed_capture(1.3, hs, scalars=True)
        assert "fields" not in only
        np.testing.assert_array_equal(only["power"], cap["power"])                        # (the log is reduced in a fixed order: reproducible bit for bit)
        np.testing.assert_array_equal(only["peak"], cap["peak"])
        np.testing.assert_array_equal(p.get_field(), log["fields"][-1])
    finally:
        p.close()


@pytest.mark.parametrize("half_phase,steps,bound", [(0.1, 20, TOL_100), (0.4, 10, 5e-5)])
def test_the_16_bit_stale_power_holds_its_stated_phase_bound(half_phase, steps, bound, monkeypatch):
    """The large complex64 plans carry the stale |A|^2 across the launch boundary as 16-bit fixed point relative to each thread's own maximum
    (ssfm_kernels.hpp p16_layout): the ABSOLUTE error of the nonlinear phase is at most 2^-17 of the thread's largest half-step phase.  The goldens and the
    benchmark configurations turn <= 0.05 rad per half step; this test goes where the bound starts to show: a peak of 0.1 rad per half step over 20 steps
    stays inside the suite's tolerance, 0.4 rad over 10 steps inside 5e-5 (the estimate 2^-17 / sqrt(3) x phase x sqrt(half steps) gives 8e-6; a step
    that turns 0.8 rad carries a splitting error of percents anyway -- and the reference does not bound a user-given h)."""
    for k in ("SSFM_E", "SSFM_EF", "SSFM_LANES"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()
    gv(**workloads.BENCH_GV)
    n = 1 << 18
    a = workloads.qpsk_field(n, seed=77, n_pol=1, power_w=1.0)[0]
    gamma, h = 1.3, 0.5
    peak = float(np.max(np.abs(a) ** 2))
    a = a * np.sqrt(half_phase / (0.5 * h * gamma * peak))          # the input's peak turns `half_phase` rad in half a step
    kw = dict(length=h * steps, h=h, alpha=0.2, beta_2=-21.7, beta_3=0.13, gamma=gamma)
    out = oa.FIBER(optical_signal(a), **kw)
    assert out.engine == "two_kernel"
    assert within(out.signal, orc.fiber_c64(a, gv.dt, **kw), bound, kw=kw, what=f"oracle, {half_phase} rad per half step")


def test_the_lanes_of_a_plan_get_hardware_queues_of_their_own(monkeypatch):
    """The runtime maps the streams of a priority class onto four hardware queues; with 3 (mod 4) other streams of the class alive the second
    lane of a new plan used to land on the queue of the first (profiles/r04_order_dependence.txt): lanes one after the other; and lanes on queues of
    their own can still be in each other's way (3-6 x slower).  Round 5: plan creation rates every lane with the plan's OWN kernels (launch period with
    the other lane running / alone), and every long two-lane run is looked at afterwards -- a slow one has its lanes rated again and repaired before the
    next run (``lanes_remade``, ssfm_host.hip lane_health).  So at the test level NO plan is ever made a second time: with 0 ... 5 other plans alive a
    two-lane run takes the same time, whatever the library had to do to get there."""
    import time
    gv(**workloads.BENCH_GV)
    n = 1 << 19
    monkeypatch.setenv("SSFM_LANES", "2")
    monkeypatch.setenv("SSFM_LANE_POOL_OFF", "1")                 # (every plan of this test makes and rates FRESH streams; the pool of rated pairs has a test of its own below)
    a = workloads.qpsk_field(n, seed=4).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(300, 0.125, np.float32)
    others, times, infos = [], [], []

    def make_and_time():
        p = _lib.Plan(n, 2, _lib.C64)
        try:
            assert p.lanes == 2
            p.set_linear_operator(D); p.set_field(a)
            p.propagate_fixed(1.3, hs); p.synchronize()            # (a slow first run is repaired here: ssfm_synchronize looks at the run)
            best = None
            for rep in range(3):              # (the best of three: a box that is still waking up is slow once)
                t0 = time.perf_counter()
                p.propagate_fixed(1.3, hs); p.synchronize()
                dt_run = time.perf_counter() - t0
                best = dt_run if best is None else min(best, dt_run)
            return best, p.last_run_info()
        finally:
            p.close()

    try:
        for k in range(6):
            t, info = make_and_time()
            assert not info["lanes_share_queue"] and info["lanes"] == 2 and not info["lanes_dropped"], (k, info)
            assert 0 < info["lane_score"] <= 1.6 and info["lane_last_us"] <= 1.8 * info["lane_pair_us"], (k, info)
            times.append(t); infos.append(info)
            q = _lib.Plan(1 << 14, 1, _lib.C64)                       # one more USED high-priority stream stays alive
            q.set_linear_operator(oa.devices.linear_operator(1 << 14, gv.dt, 0.2, -21.7, 0.13))
            q.set_field(workloads.qpsk_field(1 << 14, seed=k, n_pol=1)); q.propagate_fixed(1.3, hs[:3]); q.synchronize()
            others.append(q)
    finally:
        for q in others:
            q.close()
    assert max(times) < 1.35 * min(times), (times, infos)


def test_a_plan_whose_lane_goes_bad_heals_itself_and_a_hopeless_one_drops_to_one_lane(monkeypatch):
    """The run-time half of the lane health check, driven through its test hook: ``SSFM_LANE_FAULT=1`` makes the plan believe a much better launch period
    than it can reach, so that the next long run looks slow -- the lanes are rated again on scratch fields (they are fine: nothing is replaced, the run's
    period becomes the new normal, the caller's field is untouched); ``SSFM_LANE_FAULT=2`` makes every rating come out bad: two repairs in a row fail and
    the plan drops to one lane, whose results are bit-identical (the lanes are independent rows)."""
    gv(**workloads.BENCH_GV)
    n = 1 << 19
    monkeypatch.setenv("SSFM_LANES", "2")
    a = workloads.qpsk_field(n, seed=5).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(80, 0.125, np.float32)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D); p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        want = p.get_field().copy()
        base = p.last_run_info()
        assert base["lanes"] == 2 and base["lanes_remade"] == 0
        p.lane_fault(1)
        p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        info = p.last_run_info()
        assert info["lanes"] == 2 and not info["lanes_dropped"], info
        assert info["lane_heals"] == base["lane_heals"] + 1, (base, info)           # the lanes were looked at ...
        assert np.array_equal(p.get_field(), want)                                   # ... on scratch fields: the result is the run's
        p.lane_fault(2)
        for _ in range(3):
            p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        info = p.last_run_info()
        assert info["lanes_dropped"] and info["lanes"] == 1, info
        p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        assert np.array_equal(p.get_field(), want)
        assert p.last_run_info()["engine"] == "two_kernel"
    finally:
        p.close()


def test_a_plan_that_dropped_to_one_lane_tries_its_second_lane_again(monkeypatch):
    """The way back (ssfm_lanes.hpp cooldown_due): a plan that dropped to one lane rates its lanes once more at its 32nd look -- one look per propagate_fixed
    and synchronize call, two per last_run_info() (it synchronises first), so in the seventh run of this loop.  With the fault hook cleared the rating is the plan's own: lanes it finds good
    (``lane_score`` <= 1.6) come back, lanes it finds in the way (a contended GPU) stay dropped; either way the heal happens once and every run's field is
    bit-identical to the two-lane result."""
    gv(**workloads.BENCH_GV)
    n = 1 << 19
    monkeypatch.setenv("SSFM_LANES", "2")
    a = workloads.qpsk_field(n, seed=5).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(80, 0.125, np.float32)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D); p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        want = p.get_field().copy()
        assert p.last_run_info()["lanes"] == 2
        p.lane_fault(2)
        for _ in range(3):
            p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
        dropped = p.last_run_info()
        assert dropped["lanes_dropped"] and dropped["lanes"] == 1, dropped
        p.lane_fault(0)
        infos = []
        for _ in range(32):
            p.set_field(a); p.propagate_fixed(1.3, hs); p.synchronize()
            infos.append(p.last_run_info())
            assert np.array_equal(p.get_field(), want), infos[-1]
        heals = [i["lane_heals"] - dropped["lane_heals"] for i in infos]
        assert heals[0] == 0 and heals[-1] == 1 and sorted(heals) == heals, heals            # the cooldown's heal happened, and happened once
        first = infos[heals.index(1)]
        print(f"cooldown heal after {heals.index(1) + 1} runs: lane_score {first['lane_score']:.3f}, lanes {first['lanes']}, lanes_dropped {first['lanes_dropped']}")
        if first["lane_score"] <= 1.6:
            assert first["lanes"] == 2 and not first["lanes_dropped"], first                   # the plan's own rating found the lanes good: they are back
        else:
            assert first["lanes"] == 1 and first["lanes_dropped"], first                       # (a contended machine is not a failure of the rule)
    finally:
        p.close()


@pytest.mark.parametrize("rows", [1, 2, 4])
def test_plans_of_8192_samples_take_the_one_xcd_engine(rows, monkeypatch):
    """At 8192 samples the one-XCD engine (k_medium, 64 x 128 shape) is faster than the one-workgroup-per-row kernel of the small plans
    (5.4 against 6.4 us per step) and is the default: one launch, bit-identical to the two-kernel engine (SSFM_SMALL=0 SSFM_MEDIUM=0),
    within the oracle's tolerance, and close to the small-plan kernel's result (SSFM_MEDIUM=0)."""
    n = 8192
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(813 + rows)
    a = ((rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) * 0.05).astype(np.complex64)
    hs = np.array([0.5] * 20 + [0.25, 0.5, 0.125], dtype=np.float32)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    for k in ("SSFM_FUSED_PATIENCE_TICKS", "SSFM_FORCE_FLY", "SSFM_E"):
        monkeypatch.delenv(k, raising=False)
    got = {}
    for name, env in (("default", {"SSFM_MEDIUM": "1", "SSFM_SMALL": "1"}), ("small", {"SSFM_MEDIUM": "0", "SSFM_SMALL": "1"}),
                      ("two-kernel", {"SSFM_MEDIUM": "0", "SSFM_SMALL": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p = _lib.Plan(n, rows, _lib.C64)
        try:
            p.set_linear_operator(D)
            p.set_field(a)
            p.propagate_fixed(1.3, hs)
            got[name] = (p.get_field(), p.last_propagate_ms()[1])
        finally:
            p.close()
    assert got["default"][1] == 1 and got["small"][1] == 1 and got["two-kernel"][1] > 10
    np.testing.assert_array_equal(got["default"][0], got["two-kernel"][0])
    assert within(got["default"][0], got["small"][0], steps=hs.size, what="one-XCD engine against the one-workgroup engine")
    if rows <= 2:
        A = a.copy()
        for h_ in hs:
            A = orc.ssfm_step_c64(A, orc.linear_operator_c64(n, gv.dt, 0.2, -21.7, 0.13), np.float32(1.3), h_)
        assert within(got["default"][0], A, steps=hs.size, what="oracle, step by step")


def test_medium_single_launch_engine_on_several_plans_at_once(monkeypatch):
    """Plans take turns on the XCDs, so that single-launch runs of different plans -- here four host threads, each with its own plan,
    twenty runs each, all in flight together -- do not wait for each other's workgroups; every result equals the two-kernel engine's."""
    import threading
    n = 1 << 14
    gv(**workloads.BENCH_GV)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(40, 0.25, np.float32)
    fields = [workloads.qpsk_field(n, seed=40 + k, power_w=5e-3).astype(np.complex64) for k in range(4)]
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS", raising=False)
    monkeypatch.delenv("SSFM_FORCE_FLY", raising=False)
    monkeypatch.delenv("SSFM_E", raising=False)
    monkeypatch.setenv("SSFM_MEDIUM", "0")
    want = []
    for a in fields:
        q = _lib.Plan(n, 2, _lib.C64)
        try:
            q.set_linear_operator(D); q.set_field(a); q.propagate_fixed(1.3, hs)
            want.append(q.get_field())
        finally:
            q.close()
    monkeypatch.setenv("SSFM_MEDIUM", "1")
    plans = [_lib.Plan(n, 2, _lib.C64) for _ in fields]
    errors = []
    def work(k):
        try:
            plans[k].set_linear_operator(D)
            for rep in range(20):
                plans[k].set_field(fields[k]); plans[k].propagate_fixed(1.3, hs)
                got = plans[k].get_field()
                if not np.array_equal(got, want[k]):
                    errors.append((k, rep, "mismatch"))
            if os.environ.get("SSFM_MEDIUM_EXPECT", "1") == "1" and plans[k].last_propagate_ms()[1] != 1:
                errors.append((k, "launches", plans[k].last_propagate_ms()[1]))
        except Exception as e:                                            # noqa: BLE001
            errors.append((k, repr(e)))
    try:
        ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in ts: t.start()
        for t in ts: t.join()
    finally:
        for p in plans: p.close()
    assert not errors, errors


def test_medium_single_launch_engine_without_patience_falls_back(monkeypatch):
    """A workgroup of k_medium never waits longer than its patience at a barrier; with none at all some give up: the plan restores the
    input, repeats the run on the two-kernel engine -- bit for bit its result -- and keeps to it."""
    n = 1 << 15
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=3, power_w=5e-3).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(25, 0.2, np.float32)
    monkeypatch.setenv("SSFM_MEDIUM", "0")
    q = _lib.Plan(n, 2, _lib.C64)
    try:
        q.set_linear_operator(D); q.set_field(a); q.propagate_fixed(1.3, hs)
        f0 = q.get_field()
    finally:
        q.close()
    monkeypatch.setenv("SSFM_MEDIUM", "1")
    monkeypatch.setenv("SSFM_FUSED_PATIENCE_TICKS", "-1")
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D)
        for rep in range(3):
            p.set_field(a); p.propagate_fixed(1.3, hs)
            np.testing.assert_array_equal(p.get_field(), f0)
    finally:
        p.close()


@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
@pytest.mark.parametrize("log2n, rows", [(14, 1), (14, 2), (15, 2), (16, 2), (17, 1)])
def test_fused_adaptive_column_kernel_against_the_three_launch_engine(log2n, rows, prec, monkeypatch):
    """Plans of 2^14 ... 2^18 samples finish a step and begin the next in ONE launch of the column kernel (TM_MID_A: the
    workgroups wait inside the kernel for the global max |A|^2); SSFM_ADAPT_FUSED=0 at plan creation keeps END and BEGIN apart.
    Same step rule on the same maxima: identical z logs; the fields differ by the rounding of one merged rotation per step."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=60 + log2n, power_w=10e-3)[:rows]
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec)
    res = {}
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS", raising=False)     # (the knob suite runs everything without patience too)
    for fused in ("1", "0"):
        monkeypatch.setenv("SSFM_ADAPT_FUSED", fused)
        p = _lib.Plan(n, rows, prec)
        try:
            p.set_linear_operator(D)
            for rep in range(2):
                p.set_field(a)
                steps, z, _ = p.propagate_adaptive(1.3, 4.0, 0.002, False)
            res[fused] = (steps, z, p.get_field(), p.last_propagate_ms()[1])
        finally:
            p.close()
    s1, z1, f1, l1 = res["1"]
    s0, z0, f0, l0 = res["0"]
    assert s1 > 10 and abs(z1[-1] - 4.0) < 1e-5
    assert l1 < l0 and l1 <= 2 * s1 + 40 and l0 >= 3 * s0           # two launches per step instead of three
    assert abs(s1 - s0) <= 1
    k = min(s1, s0, 12)
    np.testing.assert_allclose(z1[:k], z0[:k], rtol=2e-6 if prec == _lib.C64 else 1e-12)
    assert within(f1, f0, (tol_at(max(s1, s0)) if prec == _lib.C64 else 1e-9), steps=s1, what=f"fused adaptive kernel against three launches per step ({s1} vs {s0} steps)")
    if True:                       # every size against the oracle directly: the plain bound of the run's own step count ("the same bound after both reach z = L")
        if prec == _lib.C128:
            ref = orc.fiber_c128(a if rows > 1 else a[0], gv.dt, 4.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.002)
            assert within(f1, ref, 1e-7, steps=s1, what="float64 restatement, adaptive")
        else:
            zo, Ao = orc.fiber_c64(a if rows > 1 else a[0], gv.dt, 4.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.002, return_steps=True)
            assert abs(len(zo) - 1 - s1) <= 1
            assert within(f1 if rows > 1 else f1[0], Ao[-1], steps=s1, what=f"oracle adaptive ({s1} vs {len(zo) - 1} steps)")


@pytest.mark.parametrize("log2n, rows", [(12, 2), (13, 1), (13, 2), (14, 1), (14, 2), (14, 4), (15, 2), (16, 1), (16, 2), (17, 1)])
def test_medium_adaptive_run_in_one_launch(log2n, rows, monkeypatch):
    """complex64 plans of up to 2^17 samples in all take a whole ADAPTIVE run in one launch on one XCD (k_medium_adapt: k_medium's
    passes, the step size found on the way; every workgroup keeps the step control state itself).  SSFM_MEDIUM_ADAPT=0 keeps two
    launches per step.  Same step rule on the same maxima: the same number of steps, z logs equal, fields equal to rounding; twice in
    a row (the flag words are epochs: a stale one would show); against the oracle at the small sizes."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    rng = np.random.default_rng(300 + log2n + rows)
    a = (workloads.qpsk_field(n, seed=80 + log2n, power_w=10e-3)[:1] * np.ones((rows, 1))).astype(np.complex64)
    a = (a * (1 + 0.1 * rng.standard_normal((rows, 1)))).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS", raising=False)
    monkeypatch.setenv("SSFM_ADAPT_FUSED", "1")
    monkeypatch.setenv("SSFM_MEDIUM", "1")
    monkeypatch.setenv("SSFM_SMALL", "0" if log2n == 12 else "1")          # (4096 x 2: the reference run is the launch-per-pass engine, not k_small_adapt)
    res = {}
    for one in ("1", "0"):
        monkeypatch.setenv("SSFM_MEDIUM_ADAPT", one)
        p = _lib.Plan(n, rows, _lib.C64)
        try:
            p.set_linear_operator(D)
            outs = []
            for rep in range(2):
                p.set_field(a)
                steps, z, _ = p.propagate_adaptive(1.3, 5.0, 0.003, False)
                outs.append((steps, z, p.get_field(), p.last_propagate_ms()[1]))
                info = p.last_run_info()
                assert (info["engine"] == "medium_adaptive") == (one == "1") and not info["fell_back"], info
            res[one] = outs
        finally:
            p.close()
    (s1, z1, f1, l1), (s1b, z1b, f1b, _) = res["1"]
    s0, z0, f0, l0 = res["0"][0]
    assert s1 > 10 and abs(z1[-1] - 5.0) < 1e-5
    assert l1 <= 3 and l0 >= 2 * s0                                   # |A|^2 maximum, first step size, the run itself
    assert s1 == s1b and np.array_equal(z1, z1b) and np.array_equal(f1, f1b)
    assert abs(s1 - s0) <= 1
    k = min(s1, s0, 12)
    np.testing.assert_allclose(z1[:k], z0[:k], rtol=2e-6)
    assert within(f1, f0, steps=max(s1, s0), what=f"one-launch adaptive engine against two launches per step ({s1} vs {s0} steps)")
    if rows <= 2:                  # (the reference takes one or two polarisations) every size against the oracle directly, at the plain bound of the step count
        zo, Ao = orc.fiber_c64(a if rows > 1 else a[0], gv.dt, 5.0, 0.2, -21.7, 0.13, 1.3, phi_max=0.003, return_steps=True)
        assert abs(len(zo) - 1 - s1) <= 1
        assert within(f1 if rows > 1 else f1[0], Ao[-1], steps=s1, what=f"oracle adaptive ({s1} vs {len(zo) - 1} steps)")


@pytest.mark.parametrize("log2n, rows", [(18, 2), (19, 1), (19, 2), (20, 2)])
def test_fused_adaptive_column_kernel_on_large_grids(log2n, rows, monkeypatch, golden_dir):
    """complex64 plans whose column kernel has up to 512 workgroups (2^20 x 2: two per CU, all resident) run the same fused kernel:
    every workgroup publishes (step, max |A|^2) as one 8-byte word and reads everybody's (AdaptState::wgmax) -- two launches per step
    instead of three (SSFM_ADAPT_FUSED=0).  Each engine against the ORACLE's run of the same field at full size (z log, every 257th sample,
    power: tests/golden/make_adaptive_strided.py), and against each other; the run info says which engine really ran."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=70 + log2n, power_w=10e-3)[:rows]
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    monkeypatch.delenv("SSFM_FUSED_PATIENCE_TICKS", raising=False)
    g = np.load(os.path.join(golden_dir, "adaptive_full_strided.npz"))
    key = f"{log2n}x{rows}"
    zo, so, po = g[f"z_{key}"], g[f"samples_{key}"], g[f"power_{key}"]
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("SSFM_ADAPT_FUSED", fused)
        p = _lib.Plan(n, rows, _lib.C64)
        try:
            p.set_linear_operator(D)
            for rep in range(2):
                p.set_field(a)
                steps, z, _ = p.propagate_adaptive(1.3, 6.0, 0.004, False)
            info = p.last_run_info()
            assert info["engine"] == ("adaptive_fused" if fused == "1" else "adaptive_3_launches") and not info["fell_back"], info
            res[fused] = (steps, z, p.get_field(), p.last_propagate_ms()[1])
        finally:
            p.close()
        # against the oracle (the reference's arithmetic): same number of steps within one, the z log while both are in step, the field
        f = res[fused][2].reshape(rows, n)
        assert abs(steps - (len(zo) - 1)) <= 1, (steps, len(zo) - 1)
        k = min(steps, len(zo) - 1, 12)
        np.testing.assert_allclose(np.asarray(z)[:k + 1], zo[:k + 1], rtol=5e-6, atol=1e-7)
        assert within(f[:, ::257], so, steps=steps, what=f"the oracle's full-size adaptive fixture ({steps} vs {len(zo) - 1} steps)")
        np.testing.assert_allclose(np.mean(np.abs(f.astype(np.complex128)) ** 2, axis=-1), po, rtol=1e-4)
    s1, z1, f1, l1 = res["1"]
    s0, z0, f0, l0 = res["0"]
    assert s1 > 10 and abs(z1[-1] - 6.0) < 1e-5
    assert l1 < l0 and l1 <= 2 * s1 + 40 and l0 >= 3 * s0
    assert abs(s1 - s0) <= 1
    k = min(s1, s0, 12)
    np.testing.assert_allclose(z1[:k], z0[:k], rtol=2e-6)
    assert within(f1, f0, steps=max(s1, s0), what=f"fused adaptive kernel against three launches per step ({s1} vs {s0} steps)")


def test_fused_adaptive_kernel_gives_up_and_the_run_falls_back(monkeypatch):
    """A workgroup of the fused kernel never waits longer than its patience for the others (a GPU shared with another job
    may not run the whole grid at once).  With no patience at all some workgroups give up: the plan restores the input, runs
    the three-launch engine instead -- bit for bit its result -- and keeps to it."""
    n = 1 << 15
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=3, power_w=10e-3)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    monkeypatch.setenv("SSFM_ADAPT_FUSED", "0")
    q = _lib.Plan(n, 2, _lib.C64)
    try:
        q.set_linear_operator(D); q.set_field(a)
        s0, z0, _ = q.propagate_adaptive(1.3, 4.0, 0.002, False)
        f0 = q.get_field()
    finally:
        q.close()
    monkeypatch.setenv("SSFM_ADAPT_FUSED", "1")
    monkeypatch.setenv("SSFM_FUSED_PATIENCE_TICKS", "-1")
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D)
        for rep in range(2):                       # the second run starts on the three-launch engine
            p.set_field(a)
            s1, z1, _ = p.propagate_adaptive(1.3, 4.0, 0.002, False)
            assert s1 == s0 and np.array_equal(z1, z0) and np.array_equal(p.get_field(), f0)
    finally:
        p.close()


def test_operator_tables_of_one_schedule_do_not_evict_each_other():
    """The table cache holds four step sizes per plan.  Schedules {a, b}, {c, d}, {a, e} in this order used to hand the third
    run e's table for a's steps (round-robin victim = a's slot).  Both engines; against a fresh plan, bit for bit."""
    gv(**workloads.BENCH_GV)
    for n in (4096, 1 << 15):
        rng = np.random.default_rng(n)
        a = ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.05).astype(np.complex64)
        D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
        scheds = [np.array(v, np.float32) for v in ([0.5, 0.25, 0.5], [0.125, 0.0625, 0.125], [0.5, 1.0, 0.5, 1.0])]
        p = _lib.Plan(n, 2, _lib.C64)
        try:
            p.set_linear_operator(D)
            for hs in scheds:
                p.set_field(a)
                p.propagate_fixed(1.3, hs)
            got = p.get_field()
        finally:
            p.close()
        q = _lib.Plan(n, 2, _lib.C64)
        try:
            q.set_linear_operator(D)
            q.set_field(a)
            q.propagate_fixed(1.3, scheds[-1])
            want = q.get_field()
        finally:
            q.close()
        assert np.array_equal(got, want)


@pytest.mark.parametrize("waves", ["1", "4"])
def test_sosfiltfilt_both_workgroup_shapes(waves, monkeypatch):
    """The filter kernels exist with 1 (round 6; 2 before) and with 4 wavefronts per workgroup and pick by the size of the call
    (sos_filter.hip `run_filter`); here both shapes run every size, across their group boundaries (64 W chunks of 12)."""
    from scipy import signal as sg
    monkeypatch.setenv("SOS_WAVES_FORCE", waves)
    # (... and of 18: with four wavefronts a call that fits the one-launch form takes the long chunk; 18 * 64 = 1152 per wavefront, 4608 per group)
    for order, n in ((4, 768 - 30), (4, 768 - 29), (4, 3 * 768 - 30 + 1), (4, 1530), (4, 1537), (4, 3060), (4, 3073), (3, 12 * 128 * 7 + 5), (8, 12 * 256 * 3 - 31), (4, (1 << 18) + 3),
                     (4, 4608 - 30), (4, 4608 - 29), (4, 2 * 4608 - 30 - 18), (2, 1152 * 3 - 18), (5, 18 * 256 * 5 + 1), (4, 18 * 64 * 9 - 30 + 17)):
        sos = sg.bessel(order, 0.07 if n > 4096 else 0.2, "low", norm="mag", output="sos")
        zi = sg.sosfilt_zi(sos)
        rng = np.random.default_rng(n)
        x = rng.standard_normal(n).cumsum() * 0.05 + rng.standard_normal(n)
        assert within(_lib.sosfiltfilt(sos, zi, x), sg.sosfiltfilt(sos, x), TOL_FILT)
        xc = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))
        assert within(_lib.sosfiltfilt(sos, zi, xc), sg.sosfiltfilt(sos, xc, axis=-1), TOL_FILT)
        # the other shape right after: the tables of the group level are rebuilt for it
        monkeypatch.setenv("SOS_WAVES_FORCE", "4" if waves == "1" else "1")
        assert within(_lib.sosfiltfilt(sos, zi, x), sg.sosfiltfilt(sos, x), TOL_FILT)
        monkeypatch.setenv("SOS_WAVES_FORCE", waves)


def test_sosfiltfilt_on_device_buffers():
    """ssfm_sosfiltfilt(on_device = 1) on the field buffers of complex128 plans: same result as the host entry
    point, out of place and in place (a propagated field is filtered where it lies)."""
    from scipy import signal as sg
    sos = sg.bessel(4, 0.1, "low", norm="mag", output="sos")
    zi = sg.sosfilt_zi(sos)
    rng = np.random.default_rng(5)
    n = 1 << 16
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    want = _lib.sosfiltfilt(sos, zi, x)
    p, q = _lib.Plan(n, 2, _lib.C128), _lib.Plan(n, 2, _lib.C128)
    try:
        p.set_field(x)
        p.synchronize()
        _lib.sosfiltfilt_device(sos, zi, p.field_device_ptr, q.field_device_ptr, n, 2, True)
        assert np.array_equal(q.get_field(), want)
        assert np.array_equal(p.get_field(), x)                        # input untouched
        _lib.sosfiltfilt_device(sos, zi, p.field_device_ptr, p.field_device_ptr, n, 2, True)
        assert np.array_equal(p.get_field(), want)
        assert _lib.sosfiltfilt_last_ms() > 0
        # the same bytes read as 4 real rows of 2n samples would be a different filter problem; as 2 x 2n
        # REAL rows with interleaved re/im it is not valid either -- real mode is checked on its own data
        p.set_field(x)
        p.synchronize()
        _lib.sosfiltfilt_device(sos, zi, p.field_device_ptr, p.field_device_ptr, 2 * n, 2, False)
        got = p.get_field().view(np.float64)
        assert np.array_equal(got, _lib.sosfiltfilt(sos, zi, x.view(np.float64)))
    finally:
        p.close()
        q.close()


@pytest.mark.parametrize("order,n,rows,cplx", [(4, 1 << 16, 2, True), (2, 5000, 1, False), (8, 70001, 2, True), (5, 300000, 1, False),
                                               (4, 1 << 20, 2, True), (3, 777, 3, True)])
def test_sosfiltfilt_in_one_launch_and_in_three(order, n, rows, cplx, monkeypatch):
    """Both forms of the filter against SciPy and against each other: the one-launch kernel (every workgroup of the call
    resident, group totals handed over through flags in HBM) and the three-launch form that longer calls, or a call that
    could not get its whole grid running, use."""
    from scipy import signal as sg
    sos = sg.bessel(order, 0.06, "low", norm="mag", output="sos")
    zi = sg.sosfilt_zi(sos)
    rng = np.random.default_rng(n + order)
    x = rng.standard_normal((rows, n)).cumsum(axis=-1) * 0.02 + rng.standard_normal((rows, n))
    if cplx:
        x = x + 1j * rng.standard_normal((rows, n))
    want = sg.sosfiltfilt(sos, x, axis=-1)
    monkeypatch.delenv("SSFM_SOS_ONE_LAUNCH", raising=False)
    one = _lib.sosfiltfilt(sos, zi, x)
    launches_default = _lib.sosfiltfilt_last_launches()
    monkeypatch.setenv("SSFM_SOS_ONE_LAUNCH", "0")
    three = _lib.sosfiltfilt(sos, zi, x)
    assert _lib.sosfiltfilt_last_launches() == 3
    assert within(one, want, TOL_FILT) and within(three, want, TOL_FILT)
    assert within(one, three, 1e-13)
    if order <= 4:
        assert launches_default == 1                                   # (orders 5 to 8 fit one workgroup per CU: the longest calls fall back)


@pytest.mark.parametrize("wn", [0.3, 0.06, 0.004, 0.0012, 0.0003])
@pytest.mark.parametrize("n,rows,cplx", [(1 << 18, 2, True), (60000, 1, False), (1 << 20, 1, False)])
def test_sosfiltfilt_start_states_from_the_totals_that_matter(wn, n, rows, cplx, monkeypatch):
    """Round 6: a workgroup of the one-launch form builds its start state from the nearest totals only, as many as the powers of the group map stay
    above 1e-40 (one at these cut-offs down to fs / 500, two or three below, ALL of them -- the round-5 path -- for the narrowest here).  Same result as
    with every total (SSFM_SOS_NEAR=0), and SciPy's within the filter's conditioning."""
    from scipy import signal as sg
    sos = sg.bessel(4, wn, "low", norm="mag", output="sos")
    zi = sg.sosfilt_zi(sos)
    rng = np.random.default_rng(int(n + 1e5 * wn))
    x = rng.standard_normal((rows, n)).cumsum(axis=-1) * 0.02 + rng.standard_normal((rows, n))
    if cplx:
        x = x + 1j * rng.standard_normal((rows, n))
    want = sg.sosfiltfilt(sos, x, axis=-1)
    bound = max(TOL_FILT, 5 * 5e-20 * (2.0 / wn) ** 3)                  # (conditioning of the chunked recurrence)
    monkeypatch.delenv("SSFM_SOS_ONE_LAUNCH", raising=False)              # (the look-back is the one-launch form's: the knobs this test depends on are pinned)
    monkeypatch.delenv("SSFM_SOS_MEET", raising=False)
    monkeypatch.delenv("SSFM_SOS_NEAR", raising=False)
    near = _lib.sosfiltfilt(sos, zi, x)
    assert _lib.sosfiltfilt_last_launches() == 1
    r_near = _lib.sosfiltfilt_last_route()
    assert r_near["tagged"] and not r_near["meet"]
    if wn >= 0.06:
        assert r_near["look"] == 1, r_near                              # (the near look-back really ran: the comparison below is of two paths)
    monkeypatch.setenv("SSFM_SOS_NEAR", "0")
    every = _lib.sosfiltfilt(sos, zi, x)
    assert _lib.sosfiltfilt_last_launches() == 1
    assert _lib.sosfiltfilt_last_route()["look"] == 0                   # ... and every total went into this one
    assert within(near, want, bound) and within(every, want, bound)
    assert within(near, every, max(1e-13, bound / 10))
    # ... and the ONE-meeting kernels (opt-in: they are not faster; taken when the look-back is at most two groups, else the default runs)
    monkeypatch.delenv("SSFM_SOS_NEAR", raising=False)
    monkeypatch.setenv("SSFM_SOS_MEET", "1")
    met = _lib.sosfiltfilt(sos, zi, x)
    assert _lib.sosfiltfilt_last_launches() == 1
    r_met = _lib.sosfiltfilt_last_route()
    assert not r_met["meet"] or 1 <= r_met["look"] <= 2, r_met
    if wn >= 0.06 and n <= 1 << 18:
        assert r_met["meet"], r_met                                     # (one group back: the single-meeting kernel is what ran)
    assert within(met, want, bound) and within(met, near, max(1e-13, bound / 10))


def test_sosfiltfilt_one_launch_gives_up_cleanly(monkeypatch):
    """A grid that cannot make progress as a whole (here: forced, a wait of 0.01 us) hands the call to the three-launch
    form: same result, input untouched."""
    from scipy import signal as sg
    sos = sg.bessel(4, 0.1, "low", norm="mag", output="sos")
    zi = sg.sosfilt_zi(sos)
    rng = np.random.default_rng(11)
    n = 1 << 17
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    want = sg.sosfiltfilt(sos, x, axis=-1)
    p, q = _lib.Plan(n, 2, _lib.C128), _lib.Plan(n, 2, _lib.C128)
    try:
        p.set_field(x)
        p.synchronize()
        monkeypatch.setenv("SSFM_SOS_PATIENCE_US", "1")
        _lib.sosfiltfilt_device(sos, zi, p.field_device_ptr, q.field_device_ptr, n, 2, True)
        # (a 1 us wait may or may not be enough on an idle GPU: either form is acceptable, the result is not)
        assert _lib.sosfiltfilt_last_launches() in (1, 3)
        assert within(q.get_field(), want, TOL_FILT)
        assert np.array_equal(p.get_field(), x)
        _lib.sosfiltfilt_device(sos, zi, p.field_device_ptr, p.field_device_ptr, n, 2, True)      # in place
        assert within(p.get_field(), want, TOL_FILT)
    finally:
        p.close()
        q.close()


def test_narrow_filters_warn_and_stay_within_the_documented_bound():
    from scipy import signal as sg
    gv(sps=16, R=10e9)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(60000).cumsum() * 0.01 + rng.standard_normal(60000)
    with pytest.warns(RuntimeWarning, match="below fs/500"):
        y = oa.LPF(x, BW=gv.fs / 2000).signal
    sos = sg.bessel(4, gv.fs / 2000, "low", fs=gv.fs, norm="mag", output="sos")
    assert within(y, sg.sosfiltfilt(sos, x), 5 * 5e-20 * 2000 ** 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        oa.LPF(x, BW=gv.fs / 300)                                      # no warning in the usual range


def test_bessel_filter_errors():
    gv(sps=16, R=10e9)
    with pytest.raises(TypeError, match=r"`input` must be of type \(optical_signal\)."):
        oa.BPF(np.ones(64), 1e9)
    with pytest.raises(ValueError, match="1D"):            # raised by the electrical_signal constructor, as in the reference
        oa.LPF(np.ones((2, 64)), 1e9)
    with pytest.raises(ValueError, match="greater than padlen"):          # SciPy raises ValueError for the same call
        oa.LPF(np.ones(10), 1e9)


# ----------------------------------------------------------------------- PD / EDFA
TOL_FRONT = 1e-11     # square law to 1 ulp (the reference's complex multiply fuses one product), then the filter


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["func"] in ("PD", "EDFA")])
def test_receiver_front_end_golden(golden_dir, name):
    """Same np.random seed as the capture (tests/golden/make_golden.py): the realisation is the reference's."""
    from opticomlib_amd.typing import electrical_signal
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x = _signal(case)
    if "np_seed" in case:
        np.random.seed(case["np_seed"])
    y = getattr(oa, case["func"])(x, **case["kw"])
    if case["func"] == "PD":
        assert isinstance(y, electrical_signal) and y.signal.dtype == np.float64
    else:
        assert isinstance(y, optical_signal) and y.n_pol == 2 and y.signal.dtype == np.complex128
    assert y.execution_time > 0
    assert y.signal.shape == g["out"].shape
    assert within(y.signal, g["out"], TOL_FRONT)
    if "out_noise" in g:
        assert within(y.noise, g["out_noise"], TOL_FRONT)
    else:
        assert y.noise is NULL


def test_square_law_against_oracle_full_size():
    """2^20 x 2 with noise: the device square law against the restated reference algebra."""
    from oracle import frontend_numpy as fe
    rng = np.random.default_rng(9)
    n = 1 << 20
    s = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.03
    nz = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.003
    for sig, noi in ((s, nz), (s[0], nz[0]), (s, None)):
        got_s, got_n = _lib.square_law(sig, noi, 0.7)
        want_s, want_n = fe.square_law(sig, noi, 0.7)
        np.testing.assert_allclose(got_s, want_s, rtol=1e-15, atol=0)
        if noi is None:
            assert got_n is None
        else:
            np.testing.assert_allclose(got_n, want_n, rtol=0, atol=1e-15 * np.max(np.abs(want_n)))


def test_pd_statistics_and_modes():
    """Noise terms: variances of the thermal / shot currents as specified (devices.py:1521-1527), every mode
    accepted in any letter case, the reference's errors."""
    from scipy.constants import e, k as kB
    gv(sps=16, R=10e9)
    n = 1 << 16
    x = optical_signal(np.full(n, np.sqrt(1e-3), complex))             # 1 mW CW
    from scipy import signal as sg
    BW = 0.3 * gv.fs
    sos = sg.bessel(4, BW, "low", fs=gv.fs, norm="mag", output="sos")
    _, H = sg.sosfreqz(sos, worN=4096, fs=gv.fs, whole=True)
    keep = np.mean(np.abs(H) ** 4)                                      # zero-phase filter: |H|^2 in amplitude
    np.random.seed(1)
    y = oa.PD(x, BW=BW, include_noise="Thermal-Only", i_dark=0.0)
    S_T = 4 * kB * 300.0 * gv.fs / 2 / 50.0
    assert abs(np.var(y.noise) / (S_T * 50.0 ** 2 * keep) - 1) < 0.05
    np.testing.assert_allclose(y.signal[100:-100], 1e-3 * 50.0, rtol=1e-9)
    y = oa.PD(x, BW=BW, include_noise="shot-only", i_dark=0.0)
    S_N = 2 * e * 1e-3 * gv.fs / 2
    assert abs(np.var(y.noise) / (S_N * 50.0 ** 2 * keep) - 1) < 0.05
    for mode in ("ase-only", "ase-thermal", "ase-shot", "thermal-shot", "ALL", "none"):
        y = oa.PD(x, BW=10e9, include_noise=mode)
        assert (y.noise is NULL) == (mode == "none")
    with pytest.raises(ValueError, match="must be one of the following"):
        oa.PD(x, BW=10e9, include_noise="everything")


def test_adaptive_large_grid_against_oracle():
    """Adaptive step control with a grid of hundreds of workgroups (two-level slot reduction): 2^18 x 2 and
    2^19 x 1, step positions and field against the oracle."""
    gv(**workloads.BENCH_GV)
    for k, npol in ((18, 2), (19, 1)):
        a = workloads.qpsk_field(1 << k, seed=40 + k, n_pol=npol, power_w=8e-3)
        a = a[0] if npol == 1 else a
        kw = dict(length=6, phi_max=0.005, **workloads.SMF)
        z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
        zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
        assert len(z) == len(zr) and len(z) > 10
        np.testing.assert_allclose(z, zr, rtol=2e-5)
        assert within(A_z[-1], Ar[-1], steps=len(z) - 1, what="oracle adaptive, return_steps")
        assert within(oa.FIBER(optical_signal(a), **kw).signal, Ar[-1], steps=len(z) - 1, what="oracle adaptive")


def test_arbitrary_step_schedule_through_the_abi():
    """ssfm_propagate_fixed takes ANY float32 schedule: few distinct sizes use one operator table each, many distinct
    sizes evaluate exp(D~ h) in the kernel -- both against the oracle's single steps."""
    gv(**workloads.BENCH_GV)
    n = 1 << 13
    a = workloads.qpsk_field(n, seed=77, power_w=3e-3)
    D = orc.linear_operator_c64(n, gv.dt, 0.2, -21.7, 0.13)
    rng = np.random.default_rng(5)
    for hs in (np.array([0.5, 0.25, 0.5, 0.25, 1.0, 0.5], np.float32), rng.uniform(0.05, 0.6, 14).astype(np.float32)):
        p = _lib.Plan(n, 2, _lib.C64)
        try:
            p.set_linear_operator(D)
            p.set_field(a)
            p.propagate_fixed(1.3, hs)
            got = p.get_field()
        finally:
            p.close()
        A = a.astype(np.complex64)
        for h_ in hs:
            A = orc.ssfm_step_c64(A, D, np.float32(1.3), h_)
        assert within(got, A, steps=hs.size, what="oracle, step by step")


# ----------------------------------------------------------------------- randomised parameters
def _fuzz_cases(count=24):
    rng = np.random.default_rng(2025)
    cases = []
    for i in range(count):
        k = int(rng.integers(8, 14))
        npol = int(rng.integers(1, 3))
        adaptive = bool(rng.integers(0, 2))
        sign = -1.0 if rng.integers(0, 4) == 0 else 1.0                 # a quarter are back-propagations
        fib = dict(alpha=sign * float(rng.uniform(0, 0.4)), beta_2=sign * float(rng.uniform(-25, 25)),
                   beta_3=sign * float(rng.choice([0.0, rng.uniform(-0.3, 0.3)])), gamma=sign * float(rng.choice([0.0, rng.uniform(0.5, 3)])))
        length = float(rng.uniform(1, 30))
        kw = dict(length=length, **fib)
        if adaptive:
            kw["phi_max"] = float(rng.choice([0.01, 0.03, 0.05]))
        else:
            kw["h"] = float(rng.choice([length / 7.3, 0.5, 1.0, length * 2]))          # incl. short last step and h > length
        cases.append((i, k, npol, float(rng.choice([1e-3, 5e-3, 2e-2])), kw))
    return cases


@pytest.mark.parametrize("i,k,npol,power,kw", _fuzz_cases(), ids=lambda v: str(v) if isinstance(v, int) else None)
def test_random_parameters_against_oracle(i, k, npol, power, kw):
    """Random sizes, polarisation counts, fibres (incl. negated = DBP, gamma = 0, beta_3 = 0), fixed steps
    (incl. a short last step and h > length) and adaptive steps against the oracle."""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << k, seed=500 + i, n_pol=npol, power_w=power)
    a = a[0] if npol == 1 else a
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # gamma = 0 in adaptive mode divides by zero, as in the reference
        zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
        z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
        y = oa.FIBER(optical_signal(a), **kw).signal
    steps = len(zr) - 1
    tol = tol_at(steps)
    if "h" in kw:
        np.testing.assert_array_equal(z, zr)
    else:
        assert abs(len(z) - len(zr)) <= 1
    assert within(A_z[-1], Ar[-1], tol, steps=len(z) - 1, what=f"oracle, return_steps ({len(z) - 1} vs {steps} steps)") and within(y, Ar[-1], tol, steps=steps, what="oracle")
    assert y.shape == a.shape and y.dtype == np.complex64


# ----------------------------------------------------------------------- device random numbers (rng="device")
def _philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) in plain Python integers."""
    c = list(ctr)
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def test_device_generator_known_answers_and_statistics():
    # Random123's published known-answer vectors for philox4x32_10
    assert _philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    seed, stream = 0x0123456789ABCDEF, 7
    x = _lib.randn_device((1001,), 2.0, seed, stream).to_host()
    for p in (0, 1, 250, 500):                                   # pair p -> elements 2p, 2p+1 (the last pair is cut)
        c = _philox4x32_10((p, 0, stream, 0), (seed & 0xFFFFFFFF, seed >> 32))
        u1 = (((c[0] >> 5) << 26 | (c[1] >> 6)) + 0.5) * 2.0 ** -53
        u2 = (((c[2] >> 5) << 26 | (c[3] >> 6)) + 0.5) * 2.0 ** -53
        r = np.sqrt(-2 * np.log(u1))
        assert abs(x[2 * p] - 2.0 * r * np.cos(2 * np.pi * u2)) < 1e-12
        if 2 * p + 1 < x.size:
            assert abs(x[2 * p + 1] - 2.0 * r * np.sin(2 * np.pi * u2)) < 1e-12
    n = 1 << 20
    a = _lib.randn_device((n,), 1.0, 42, 1).to_host()
    b = _lib.randn_device((n,), 1.0, 42, 2).to_host()
    np.testing.assert_array_equal(a, _lib.randn_device((n,), 1.0, 42, 1).to_host())       # reproducible
    assert abs(a.mean()) < 4e-3 and abs(a.var() - 1) < 6e-3 and abs(np.mean(a ** 4) - 3) < 0.05
    assert abs(np.mean(a * b)) < 4e-3 and abs(np.mean(a[:-1] * a[1:])) < 4e-3             # streams / neighbours uncorrelated
    assert abs(np.mean(np.abs(a) > 3) - 0.0027) < 4e-4
    z = _lib.randn_device((2, 1 << 16), 0.5, 1, 1, np.complex128).to_host()
    assert z.dtype == np.complex128 and abs(z.real.var() - 0.25) < 0.01 and abs(z.imag.var() - 0.25) < 0.01
    assert abs(np.mean(z.real * z.imag)) < 0.005


def test_pd_and_edfa_with_the_device_generator():
    """rng="device": the reference's statistics (not its draws), everything stays on the GPU."""
    from scipy import signal as sg
    from scipy.constants import e, h, k as kB
    gv(sps=16, R=10e9)
    n = 1 << 17
    x = optical_signal(np.full(n, np.sqrt(1e-3), complex))
    BW = 0.3 * gv.fs
    sos = sg.bessel(4, BW, "low", fs=gv.fs, norm="mag", output="sos")
    _, H = sg.sosfreqz(sos, worN=4096, fs=gv.fs, whole=True)
    keep = np.mean(np.abs(H) ** 4)
    oa.device_rng_seed(2024)
    y = oa.PD(x, BW=BW, include_noise="thermal-only", i_dark=0.0, rng="device")
    assert isinstance(y._raw("signal"), _lib.DeviceArray) and isinstance(y._raw("noise"), _lib.DeviceArray)
    S_T = 4 * kB * 300.0 * gv.fs / 2 / 50.0
    assert abs(np.var(y.noise) / (S_T * 50.0 ** 2 * keep) - 1) < 0.05
    np.testing.assert_allclose(y.signal[100:-100], 1e-3 * 50.0, rtol=1e-9)
    y2 = oa.PD(x, BW=BW, include_noise="shot-only", i_dark=0.0, rng="device")
    assert abs(np.var(y2.noise) / (2 * e * 1e-3 * gv.fs / 2 * 50.0 ** 2 * keep) - 1) < 0.05
    oa.device_rng_seed(2024)
    np.testing.assert_array_equal(oa.PD(x, BW=BW, include_noise="thermal-only", i_dark=0.0, rng="device").noise, y.noise)
    # all terms, noisy dual-pol input: signal part identical to the host-generator path, noise mean = beat + dark terms
    a = workloads.qpsk_field(1 << 14, seed=3)
    xin = optical_signal(a, 0.05 * a[::-1].copy())
    yd = oa.PD(xin, BW=20e9, rng="device")
    np.random.seed(0)
    yh = oa.PD(xin, BW=20e9)
    assert within(yd.signal, yh.signal, 1e-12)
    assert abs(np.mean(yd.noise) - np.mean(yh.noise)) < 0.05 * np.std(yh.noise) and abs(np.std(yd.noise) / np.std(yh.noise) - 1) < 0.05
    for mode in ("ase-only", "ase-thermal", "ase-shot", "thermal-shot", "ALL"):
        assert oa.PD(xin, BW=20e9, include_noise=mode, rng="device").noise.shape == (1 << 14,)
    assert oa.PD(optical_signal(a), BW=20e9, include_noise="ase-only", rng="device").noise.shape == (1 << 14,)
    with pytest.raises(ValueError, match="`rng` must be"):
        oa.PD(xin, BW=20e9, rng="cuda")
    # EDFA: gain, ASE power h f0 NF (G - 1) fs over two polarisations, y polarisation of a 1-pol input empty
    G, NF = 20.0, 5.0
    x1 = optical_signal(np.full(n, np.sqrt(1e-4), complex))
    ed = oa.EDFA(x1, G=G, NF=NF, rng="device")
    assert ed.on_device and ed.n_pol == 2 and ed.shape == (2, n)
    np.testing.assert_allclose(ed.signal[0], np.sqrt(1e-4) * 10.0, rtol=1e-14)
    assert not ed.signal[1].any()
    P_ase = 10 ** (NF / 10) * h * gv.f0 * (10 ** (G / 10) - 1) * gv.fs
    assert abs(np.mean(np.abs(ed.noise) ** 2, axis=-1).sum() / P_ase - 1) < 0.02
    np.random.seed(1)
    eh = oa.EDFA(xin, G=G, NF=NF, BW=60e9)
    edv = oa.EDFA(xin, G=G, NF=NF, BW=60e9, rng="device")
    assert within(edv.signal, eh.signal, 1e-12)
    assert abs(np.mean(np.abs(edv.noise) ** 2) / np.mean(np.abs(eh.noise) ** 2) - 1) < 0.05


# ----------------------------------------------------------------------- DAC
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["func"] == "DAC"])
def test_dac_golden(golden_dir, name):
    from opticomlib_amd.typing import electrical_signal
    case = CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gv(**case["gv"])
    seq = oa.PRBS(order=case["bits"][0], len=case["bits"][1])
    np.testing.assert_array_equal(seq.data, g["bits"])
    kw = dict(case["kw"])
    if "h" in kw:
        kw["h"] = np.asarray(kw["h"], dtype=float)
    y = oa.DAC(seq, **kw)
    assert isinstance(y, electrical_signal) and y.noise is NULL and y.execution_time > 0
    assert y.signal.shape == g["out"].shape and y.signal.dtype == g["out"].dtype
    assert within(y.signal, g["out"], 1e-12)


def test_laser_and_mzm_against_golden(golden_dir):
    """LASER and MZM are HIP kernels in the reference's order of operations: against the reference's own vectors they
    differ by the last bits of cos / sin / sqrt (device math library against NumPy's)."""
    from cases import case_drive
    from opticomlib_amd.typing import electrical_signal
    for name, case in CASES.items():
        if case["func"] not in ("LASER", "MZM") or case["kw"].get("BW"):
            continue
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        gv(**case["gv"])
        if case["func"] == "LASER":
            if "np_seed" in case:
                np.random.seed(case["np_seed"])
            y = oa.LASER(**case["kw"])
            assert y.on_device and y.n_pol == 1 and y.noise is NULL and y.signal.dtype == g["out"].dtype
            assert within(y.signal, g["out"], 1e-14)
            continue
        sig, noi = case_input(case)
        v, vn = case_drive(case)
        x = optical_signal(sig) if noi is None else optical_signal(sig, noi)
        y = oa.MZM(x, v if vn is None else electrical_signal(v, vn), **case["kw"])
        assert y.signal.shape == g["out"].shape and within(y.signal, g["out"], 1e-14)
        if "out_noise" in g:
            assert within(y.noise, g["out_noise"], 1e-14)
        else:
            assert y.noise is NULL
        np.testing.assert_array_equal(x.signal, sig)                  # the input is not modified
    # CW laser: exact (one sqrt on the host, a fill on the device); scalar and integer drives are spread / cast
    gv(sps=16, R=10e9, N=64)
    cw = oa.LASER(P0=10)
    np.testing.assert_array_equal(cw.signal, np.full(1024, np.sqrt(10 ** (10 / 10 - 3))))
    k, loss = np.pi / 2 / 5.0, 10 ** (-0.3)
    for drive in (1.25, np.arange(1024) % 3, np.linspace(0, 5, 1024) + 0.1j):
        got = oa.MZM(cw, drive, bias=0.5, loss_dB=3).signal
        gt = k * (np.asarray(drive) + 0.5)
        want = cw.signal * (loss ** 0.5 * (np.cos(gt) + 1j * (2 * (10 ** -2.6) ** 0.5) / 2 * np.sin(gt)))
        assert within(got, want, 1e-14)
    with pytest.raises(ValueError):
        oa.MZM(cw, np.ones(100))                                      # lengths that do not broadcast
    # all options of the laser at 2^20 samples, seeded: same draws as the oracle
    from oracle import transmitter_numpy as tx
    gv(sps=16, R=10e9, N=1 << 16)
    np.random.seed(5); got = oa.LASER(P0=3, lw=1e5, rin=-150, df=2e9).signal
    np.random.seed(5); want = tx.laser(gv.t, gv.dt, gv.fs, 3, lw=1e5, rin=-150, df=2e9)
    assert got.dtype == want.dtype == np.complex128 and within(got, want, 1e-13)


def test_device_cumsum_min_and_laser_with_the_device_generator():
    """ssfm_device_cumsum against numpy.cumsum (tile edges, one tile, many tiles), ssfm_device_reduce(SSFM_REDUCE_MIN), and the laser's
    phase / intensity noise from the device generator: the statistics of the reference's model."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 255, 4096, 4097, 3 * 4096 - 1, 300_000, (1 << 20) + 7, 1 << 21):
        x = rng.standard_normal(n)
        d = _lib.DeviceArray.from_host(x, np.float64, 0)
        exact = np.cumsum(x.astype(np.longdouble))                   # 64-bit mantissa: the yardstick for both
        got = _lib.cumsum_device(d).to_host()
        scale = max(1.0, float(np.max(np.abs(exact))))
        # the tiled scan groups the additions as a tree (error ~ log n), NumPy's loop adds left to right (~ sqrt n .. n)
        assert np.max(np.abs(got - exact)) <= 4e-16 * scale * np.log2(n + 2)
        assert np.max(np.abs(got - np.cumsum(x))) <= 4e-16 * scale * (np.log2(n + 2) + np.sqrt(n))
        assert _lib.min_device(d) == x.min()
    ones = _lib.cumsum_device(_lib.DeviceArray.from_host(np.ones(1 << 20), np.float64, 0)).to_host()
    np.testing.assert_array_equal(ones, np.arange(1, (1 << 20) + 1, dtype=float))      # exact where the sums are exact
    gv(sps=16, R=10e9, N=1 << 16)
    n = gv.t.size
    oa.device_rng_seed(7)
    a = oa.LASER(P0=3, lw=1e6, rng="device")
    b = oa.LASER(P0=3, lw=1e6, rng="device")
    oa.device_rng_seed(7)
    a2 = oa.LASER(P0=3, lw=1e6, rng="device")
    assert a.on_device and a.signal.dtype == np.complex128
    np.testing.assert_array_equal(a.signal, a2.signal)             # same seed, same realisation
    assert np.max(np.abs(a.signal - b.signal)) > 1e-3               # the next draw is another one
    amp = np.sqrt(10 ** (3 / 10 - 3))
    assert np.max(np.abs(np.abs(a.signal) - amp)) < 1e-15           # pure phase noise
    steps = np.diff(np.unwrap(np.angle(a.signal)))
    var = 2 * np.pi * 1e6 * gv.dt                                    # Wiener increments of variance 2 pi lw dt
    assert abs(steps.var() / var - 1) < 0.01 and abs(steps.mean()) < 4 * np.sqrt(var / n)
    assert abs(np.corrcoef(steps[:-1], steps[1:])[0, 1]) < 0.01     # independent increments
    r = oa.LASER(P0=3, rin=-150, rng="device").signal
    assert r.dtype == np.float64
    x = (r / amp) ** 2 - 1                                          # the intensity noise itself
    assert abs(x.var() / (10 ** -15 * gv.fs) - 1) < 0.01 and abs(x.mean()) < 4 * np.sqrt(10 ** -15 * gv.fs / n)
    with pytest.raises(ValueError, match="RIN"):
        oa.LASER(P0=3, rin=-90, rng="device")
    with pytest.raises(ValueError, match="rng"):
        oa.LASER(P0=3, rng="cuda")
    all3 = oa.LASER(P0=0, lw=1e5, rin=-150, df=1e9, rng="device").signal
    assert all3.dtype == np.complex128 and abs(np.mean(np.abs(all3) ** 2) / 1e-3 - 1) < 1e-3


def test_device_pulses_match_the_reference_expressions():
    """ssfm_load_pulse: the DAC's built-in pulses generated in GPU memory.  The time grid is NumPy's linspace bit for
    bit (the rectangular pulse is therefore exact); the others differ by the last bits of exp / sin / cos."""
    from oracle import transmitter_numpy as tx
    from opticomlib_amd import devices as od
    plan = od.get_plan(1 << 16, 1, _lib.C128, 0)

    def device_pulse(spec):
        npts = spec[0][1]
        plan.load_pulse(*spec[0])
        out = _lib.DeviceArray((1 << 16,), np.complex128, 0)
        plan.copy_from_field(0, out.ptr, (1 << 16) * 16)
        h = out.to_host()
        assert not h[npts:].any()                                  # zero-padded
        return (h if spec[1] else h.real)[:npts], h[:npts].imag

    for span, sps in ((4, 16), (7, 9), (1020, 32), (4092, 16), (60, 1000)):
        for T in (1, 2):
            got, im = device_pulse(od._nrz_spec(span, sps, T))
            np.testing.assert_array_equal(got, tx.nrz_pulse(span, sps, T)); assert not im.any()
        for T, m, c in ((1, 1, 0.0), (2, 1, 0.5), (1, 2, 0.0), (1, 3, 0.0), (2, 1, -0.8)):
            got, _ = device_pulse(od._gauss_spec(span, sps, T=T, m=m, c=c))
            want = tx.gauss_pulse(span, sps, T=T, m=m, c=c)
            assert got.dtype == want.dtype == np.complex128
            # exp amplifies the last bit of its argument by |argument| (NumPy's own complex square is SIMD-dependent
            # in that bit): a relative bound that grows with -ln|pulse|, i.e. 1e-15 at the peak, 3e-13 at 1e-300
            mag = np.abs(want)
            assert np.all(np.abs(got - want) <= 4e-16 * (2 + np.abs(np.log(mag + 1e-320))) * mag + 1e-300)
        for beta in (0.0, 0.05, 0.25, 0.5, 1.0, 1 / 3):
            for shape in ("normal", "sqrt"):
                got, im = device_pulse(od._rcos_spec(beta, span, sps, shape))
                want = tx.rcos_pulse(beta, span, sps, shape)
                # unit-peak pulses compared on their own scale: next to the removable singularities (1 - (2 beta t)^2 -> 0,
                # cos -> 0) the quotient amplifies the last bit of NumPy's SIMD cos / sin by 1/den (seen: 2e-14)
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13); assert not im.any()
    with pytest.raises(_lib.SsfmError):
        plan.load_pulse(7, 10, 0.0, 1.0, 9.0, 0, [])
    with pytest.raises(_lib.SsfmError):
        plan.load_pulse(1, 10, 0.0, 1.0, 9.0, 3, [1.0, 0.0])
    with pytest.raises(_lib.SsfmError):
        plan.load_pulse(0, (1 << 16) + 1, 0.0, 1.0, 9.0, 0, [-0.5, 0.5])


def test_transmitter_stays_on_the_device():
    """LASER and DAC leave their results in GPU memory, MZM multiplies them there, FIBER takes the product from there:
    nothing is downloaded before somebody reads a result, and the numbers are the oracle's (to the last bits of cos / sin)."""
    from oracle import transmitter_numpy as tx
    gv(sps=16, R=10e9, N=256)
    bits = oa.PRBS(9, len=256)
    rng = np.random.default_rng(2)
    amp = np.sqrt(10 ** (3 / 10 - 3))
    c2_sig, c2_noi = np.stack([np.full(4096, amp), np.full(4096, 0.5 * amp)]).astype(complex), 1e-3 * (rng.standard_normal((2, 4096)) + 0j)
    carrier2 = optical_signal(c2_sig, c2_noi)
    before = dict(_lib.TRANSFERS)
    drive = oa.DAC(bits, Vpp=5.0, offset=-2.5, pulse_shape="gaussian")
    drive_r = oa.DAC(bits, Vpp=2.0, pulse_shape="nrz", coupling="AC")
    assert isinstance(drive._raw("signal"), _lib.DeviceArray) and drive._raw("signal").dtype == np.complex128
    assert isinstance(drive_r._raw("signal"), _lib.DeviceArray) and drive_r._raw("signal").dtype == np.float64
    cw = oa.LASER(P0=3)
    assert cw.on_device and cw._raw("signal").dtype == np.float64
    m1 = oa.MZM(cw, drive, bias=-2.5, Vpi=5.0, loss_dB=3)
    m2 = oa.MZM(carrier2, drive_r, bias=0.3, Vpi=4.0, ER_dB=30, pol="y")
    y = oa.FIBER(m1, length=10, h=1.0, **workloads.SMF)
    f = oa.BPF(cw, 20e9)
    assert m1.on_device and m2.on_device and y.on_device and f.on_device
    assert _lib.TRANSFERS["d2h"] == before["d2h"]
    w1, _ = tx.mzm(np.full(4096, amp), None, tx.dac(bits.data, 16, gv.fs, pulse_shape="gaussian", Vpp=5.0, offset=-2.5), None, gv.fs, bias=-2.5, Vpi=5.0, loss_dB=3)
    w2, w2n = tx.mzm(c2_sig, c2_noi, tx.dac(bits.data, 16, gv.fs, pulse_shape="nrz", Vpp=2.0, coupling="AC"), None, gv.fs, bias=0.3, Vpi=4.0, ER_dB=30, pol="y")
    assert within(m1.signal, w1, 1e-14)
    assert within(m2.signal, w2, 1e-14) and within(m2.noise, w2n, 1e-14) and not m2.signal[0].any()
    assert f.signal.dtype == np.float64 and within(f.signal, np.full(4096, amp), 1e-12)  # a real envelope stays real through the filter
    assert within(y.signal, orc.fiber_c64(w1, gv.dt, length=10, h=1.0, **workloads.SMF), steps=10, what="oracle, device-resident chain")


def test_dac_inputs_errors_and_long_sequence():
    from oracle import transmitter_numpy as tx
    gv(sps=16, R=10e9)
    want = oa.DAC([0, 1, 0, 1, 1], Vpp=2.0).signal
    for form in ("01011", "0 1 0 1 1", (0, 1, 0, 1, 1), np.array([0, 1, 0, 1, 1], bool), oa.binary_sequence([0, 1, 0, 1, 1])):
        np.testing.assert_array_equal(oa.DAC(form, Vpp=2.0).signal, want)
    with pytest.raises(ValueError, match="pulse_shape"):
        oa.DAC("010", pulse_shape="triangle")
    with pytest.raises(ValueError, match="Vpp"):
        oa.DAC("010", Vpp=50)
    with pytest.raises(ValueError, match="offset"):
        oa.DAC("010", offset=50)
    with pytest.raises(ValueError, match="greater than 0"):
        oa.DAC("010", pulse_shape="gaussian", T=0)
    with pytest.raises(ValueError, match="less than 2\\*sps"):
        oa.DAC("010", pulse_shape="gaussian", T=3 * 16)
    with pytest.raises(ValueError, match="`m` must be greater than 0"):
        oa.DAC("010", pulse_shape="gaussian", T=8, m=0)
    with pytest.raises(ValueError, match="coupling"):
        oa.DAC("010", coupling="XX")
    bits = oa.PRBS(15, len=1 << 15).data                          # 2^19 samples: a convolution of 2^20 points
    y = oa.DAC(bits, pulse_shape="gaussian", Vpp=5.0, offset=-2.5).signal
    assert within(y, tx.dac(bits, 16, gv.fs, pulse_shape="gaussian", Vpp=5.0, offset=-2.5), 1e-12)


def test_mzm_with_filter_and_the_transmitter_chain(golden_dir):
    """MZM(BW=...) against the reference vector, then PRBS -> DAC -> MZM(LASER) -> FIBER -> PD as the reference's
    example script chains them (examples/ook_transmission_fiber_simulation.py), checked against the oracles."""
    from cases import case_drive
    from oracle import transmitter_numpy as tx, frontend_numpy as fe
    case = CASES["mzm_2pol_y_bw"]
    g = np.load(os.path.join(golden_dir, "mzm_2pol_y_bw.npz"))
    gv(**case["gv"])
    sig, _ = case_input(case)
    v, _ = case_drive(case)
    y = oa.MZM(optical_signal(sig), v, **case["kw"])
    assert within(y.signal, g["out"], TOL_FILT) and not y.signal[0].any()
    gv(sps=64, R=10e9, N=1 << 10)
    seq = oa.PRBS(order=9, len=gv.N)
    drive = oa.DAC(seq, Vpp=5.0, offset=-2.5, pulse_shape="gaussian")
    mod = oa.MZM(oa.LASER(P0=5), drive, bias=-2.5, Vpi=5.0, loss_dB=3, ER_dB=26)
    bits = seq.data
    want_v = tx.dac(bits, 64, gv.fs, pulse_shape="gaussian", Vpp=5.0, offset=-2.5)
    want_m, _ = tx.mzm(tx.laser(gv.t, gv.dt, gv.fs, 5), None, want_v, None, gv.fs, bias=-2.5, Vpi=5.0, loss_dB=3, ER_dB=26)
    assert mod.signal.shape == (1 << 16,) and within(mod.signal, want_m, 1e-12)
    kw = dict(length=50, alpha=0.2, beta_2=-20, gamma=2)
    out = oa.FIBER(mod, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        zo, Ao = orc.fiber_c64(want_m, gv.dt, return_steps=True, **kw)
        ref = Ao[-1]
    assert within(out.signal, ref, steps=len(zo) - 1, what="oracle, the reference's example link (adaptive)")
    rx = oa.PD(out, BW=gv.R * 0.75, include_noise="none")
    want_rx, _ = fe.pd(ref, None, gv.fs, gv.R * 0.75, include_noise="none")
    assert within(rx.signal, want_rx, 1e-4)  # |E|^2 of fields that agree to 2e-5


def test_the_example_link_at_a_whole_prbs_word():
    """The same chain on a WHOLE PRBS word, as the reference's scripts use it (PRBS(order) has 2^order - 1 bits): order 11 at 64 samples per bit = 131 008 samples, not a
    power of two -- the transmitter on the device, the fibre adaptive (h=None) on the chirp-z line that holds complex64 values between float64 passes (round 6), the detector's
    filter at that length."""
    from oracle import transmitter_numpy as tx, frontend_numpy as fe
    gv(sps=64, R=10e9, N=(1 << 11) - 1)
    seq = oa.PRBS(order=11)
    assert seq.data.size == (1 << 11) - 1
    drive = oa.DAC(seq, Vpp=5.0, offset=-2.5, pulse_shape="gaussian")
    mod = oa.MZM(oa.LASER(P0=8), drive, bias=-2.5, Vpi=5.0, loss_dB=3, ER_dB=26)
    n = ((1 << 11) - 1) * 64
    want_v = tx.dac(seq.data, 64, gv.fs, pulse_shape="gaussian", Vpp=5.0, offset=-2.5)
    want_m, _ = tx.mzm(tx.laser(gv.t, gv.dt, gv.fs, 8), None, want_v, None, gv.fs, bias=-2.5, Vpi=5.0, loss_dB=3, ER_dB=26)
    assert mod.signal.shape == (n,) and within(mod.signal, want_m, 1e-12)
    kw = dict(length=80, alpha=0.2, beta_2=-20, gamma=2)
    out = oa.FIBER(mod, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        zo, Ao = orc.fiber_c64(want_m, gv.dt, return_steps=True, **kw)
    steps = len(zo) - 1
    assert steps >= 10 and within(out.signal, Ao[-1], steps=steps, what=f"oracle, the example link at a whole PRBS-11 word (adaptive, {steps} steps)")
    rx = oa.PD(out, BW=gv.R * 0.75, include_noise="none")
    want_rx, _ = fe.pd(Ao[-1], None, gv.fs, gv.R * 0.75, include_noise="none")
    assert within(rx.signal, want_rx, 1e-4)  # |E|^2 of fields that agree to 2e-5


# ----------------------------------------------------------------------- device-resident signals
def _chain(x, keep):
    """FIBER -> EDFA-like noise loading -> FIBER -> DBP -> DM -> BPF -> PD, as a link script would write it."""
    from opticomlib_amd import devices as od
    old = od.KEEP_ON_DEVICE
    od.KEEP_ON_DEVICE = keep
    try:
        kw = dict(length=4, h=0.5, **workloads.SMF)
        y = oa.FIBER(x, **kw)
        rng = np.random.default_rng(1)
        ase = (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)) * 1e-4
        y2 = optical_signal.from_device(y._raw("signal"), ase) if y.on_device else optical_signal(y.signal, ase)
        z = oa.FIBER(y2, **kw)                               # complex64 signal + complex128 noise, summed then cast
        b = oa.DBP(z, **kw)
        d = oa.DM(b, D=-30.0)
        f = oa.BPF(d, BW=80e9)
        p = oa.PD(f, BW=20e9, include_noise="none")
        return y, z, b, d, f, p
    finally:
        od.KEEP_ON_DEVICE = old


def test_device_resident_chain_is_bit_identical_and_lazy():
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 14, seed=31)
    host = _chain(optical_signal(a), keep=False)
    assert not any(getattr(o, "on_device", False) for o in host[:5])
    before = dict(_lib.TRANSFERS)
    devc = _chain(optical_signal(a), keep=True)
    after = dict(_lib.TRANSFERS)
    y, z, b, d, f, p = devc
    assert all(o.on_device for o in (y, z, b, d, f)) and _lib._lib is not None and isinstance(p._raw("signal"), _lib.DeviceArray)
    assert z.shape == (2, 1 << 14) and z.size == 1 << 14 and z.n_pol == 2 and "device" in repr(z)
    # nothing crossed PCIe except the input field and the host-made noise (2 uploads), nothing came back yet
    assert after["h2d"] - before["h2d"] == 2 and after["d2h"] - before["d2h"] == 0
    for got, want in zip(devc, host):
        np.testing.assert_array_equal(got.signal, want.signal)
    assert not z.on_device                                   # reading .signal made it a host signal
    assert z.signal.dtype == np.complex64 and d.signal.dtype == np.complex128 and p.signal.dtype == np.float64
    assert y.noise is NULL and p.noise is NULL


def test_device_resident_signal_semantics():
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 12, seed=32)
    y = oa.FIBER(optical_signal(a[0]), length=2, h=1.0, **workloads.SMF)
    assert y.on_device and y.n_pol == 1 and y.shape == (1 << 12,) and len(y) == 1 << 12
    w = optical_signal(y)                                    # re-wrapping keeps the data where it is
    assert w.on_device
    ref = y.signal.copy()
    assert not y.on_device and isinstance(y.signal, np.ndarray)
    y.signal[0] = 0                                          # a host signal now: in-place edits are the user's
    np.testing.assert_array_equal(w.signal, ref)             # ... and do not leak into other wrappers' downloads
    # noise on the device, DM keeps signal and noise apart
    s = oa.FIBER(optical_signal(a), length=1, h=1.0, **workloads.SMF)
    nz = oa.FIBER(optical_signal(0.1 * a[::-1]), length=1, h=1.0, **workloads.SMF)
    both = optical_signal.from_device(s._raw("signal"), nz._raw("signal"))
    out = oa.DM(both, D=50.0)
    want = oa.DM(optical_signal(s.signal, nz.signal), D=50.0)
    np.testing.assert_array_equal(out.signal, want.signal)
    np.testing.assert_array_equal(out.noise, want.noise)
    fresh = oa.FIBER(optical_signal(a), length=1, h=1.0, **workloads.SMF)
    direct = optical_signal(fresh._raw("signal"))            # the constructor takes device arrays as they are
    assert direct.on_device and direct.n_pol == 2
    mixed = optical_signal(fresh._raw("signal"), 0.1 * a)    # device signal + host noise: an ordinary host signal
    assert not mixed.on_device and mixed.noise.shape == (2, 1 << 12)
    e = oa.EDFA(s, G=10, NF=5)                               # host-side device (np.random): materialises its input
    assert e.n_pol == 2 and e.signal.shape == (2, 1 << 12)


def test_read_back_arrays_are_ordinary_numpy_arrays():
    """Results are read back into pooled page-locked buffers wrapped as NumPy arrays: they must behave like any other
    array (writable, survive the device object and the plan, usable after the buffer of another result was recycled)."""
    import gc
    from opticomlib_amd import devices as od
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 4096)) + 1j * rng.standard_normal((2, 4096))
    d = _lib.DeviceArray.from_host(x, np.complex128, 0)
    a = d.to_host()
    assert type(a) is np.ndarray and a.flags.writeable and a.flags.c_contiguous and a.dtype == np.complex128
    np.testing.assert_array_equal(a, x)
    del d
    gc.collect()
    a *= 2                                                          # the array owns its memory through its base
    np.testing.assert_array_equal(a, 2 * x)
    b = a[1, 10:20].copy()
    view = a[0]
    del a
    gc.collect()
    other = _lib.DeviceArray.from_host(np.zeros((2, 4096), complex), np.complex128, 0).to_host()    # same size: must not reuse the live block
    np.testing.assert_array_equal(view, 2 * x[0])
    np.testing.assert_array_equal(b, 2 * x[1, 10:20])
    assert not other.any()
    del view, other
    gc.collect()
    y = oa.FIBER(optical_signal(x * 0.01), length=5, h=1.0, **workloads.SMF)
    s1 = y.signal
    od.release_plans()
    assert within(s1, orc.fiber_c64((x * 0.01), gv.dt, length=5, h=1.0, **workloads.SMF), steps=5, what="oracle")
    assert _lib.host_empty((0,), np.float64).size == 0
    import pickle
    np.testing.assert_array_equal(pickle.loads(pickle.dumps(s1)), s1)


def test_real_valued_device_signal_feeds_every_device():
    """A CW laser is a float64 array in GPU memory (as it is a float64 NumPy array in the reference): every device
    must take it from there and agree with the same call on the host array."""
    from opticomlib_amd import devices as od
    gv(sps=16, R=10e9, N=256)
    cw = oa.LASER(P0=3)
    assert cw.on_device and cw._raw("signal").dtype == np.float64
    host = optical_signal(np.full(gv.t.size, np.sqrt(10 ** (3 / 10 - 3))))
    before = _lib.TRANSFERS["d2h"]
    outs = {
        "FIBER": lambda x: oa.FIBER(x, length=3, h=1.0, **workloads.SMF),
        "FIBER128": lambda x: oa.FIBER(x, length=3, h=1.0, precision="complex128", **workloads.SMF),
        "DM": lambda x: oa.DM(x, D=-300),
        "BPF": lambda x: oa.BPF(x, 40e9),
        "PD": lambda x: oa.PD(x, BW=8e9, include_noise="none"),
        "MZM": lambda x: oa.MZM(x, 1.5, bias=0.5),
    }
    dev = {k: f(cw) for k, f in outs.items()}
    np.random.seed(3); dev["EDFA"] = oa.EDFA(cw, G=10, NF=5)
    assert _lib.TRANSFERS["d2h"] == before and cw.on_device            # nothing was downloaded on the way
    ref = {k: f(host) for k, f in outs.items()}
    np.random.seed(3); ref["EDFA"] = oa.EDFA(host, G=10, NF=5)
    for k in ref:
        assert dev[k].signal.dtype == ref[k].signal.dtype and dev[k].signal.shape == ref[k].signal.shape, k
        np.testing.assert_array_equal(dev[k].signal, ref[k].signal, err_msg=k)
        if ref[k].noise is not NULL:
            np.testing.assert_array_equal(dev[k].noise, ref[k].noise, err_msg=k)
    assert dev["BPF"].signal.dtype == np.float64 and dev["DM"].signal.dtype == np.complex128


def test_signal_call_is_the_fourier_transform_on_the_device():
    """``x('w')`` / ``x('t')`` of both signal classes (reference typing.py:1421-1462 and its tests
    tests/typing_test.py:1140-1209): fft / ifft of signal and noise, with and without the shifts, any length."""
    from opticomlib_amd.typing import electrical_signal
    rng = np.random.default_rng(12)
    for n in (2, 7, 8, 100, 3000, 4096, 65537, 1 << 17):
        for shape in ((n,), (2, n)):
            sig = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
            noi = 0.1 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
            x = optical_signal(sig, noi)
            for shift in (False, True):
                W = x("w", shift=shift)
                assert isinstance(W, optical_signal) and W.on_device and W.n_pol == x.n_pol
                ws, wn = np.fft.fft(sig, axis=-1), np.fft.fft(noi, axis=-1)
                if shift:
                    ws, wn = np.fft.fftshift(ws, axes=-1), np.fft.fftshift(wn, axes=-1)
                assert W.signal.dtype == np.complex128 and W.signal.shape == shape
                assert within(W.signal, ws, 1e-13) and within(W.noise, wn, 1e-13)
                T = x("t", shift=shift)
                ts = np.fft.ifft(sig, axis=-1)
                assert within(T.signal, np.fft.ifftshift(ts, axes=-1) if shift else ts, 1e-13)
            back = x("f")("t")                                         # device-resident all the way
            assert within(back.signal, sig, 1e-13) and within(back.noise, noi, 1e-13)
    v = rng.standard_normal(1000)
    E = electrical_signal(v)("w")
    assert isinstance(E, electrical_signal) and E.noise is NULL and within(E.signal, np.fft.fft(v), 1e-13)
    c64 = optical_signal((rng.standard_normal(512) + 1j * rng.standard_normal(512)).astype(np.complex64))
    assert c64("w").signal.dtype == np.fft.fft(c64.signal).dtype == np.complex64
    assert within(c64("w").signal, np.fft.fft(c64.signal.astype(complex)), 1e-6)
    with pytest.raises(ValueError, match="domain"):
        c64("x")
    with pytest.raises(ValueError, match="no CPU fallback"):
        optical_signal(np.ones(1, complex))("w")


def test_sum_and_real_gain_of_device_resident_signals_stay_on_the_device():
    """Combining two modulated carriers (``a + b``) and a real gain / loss factor (``0.5 * a``) are the two operators a
    link script applies between devices: on device-resident signals they run on the GPU, bit-identical to NumPy."""
    gv(sps=16, R=10e9, N=256)
    rng = np.random.default_rng(8)
    bits1, bits2 = oa.PRBS(9, len=256, seed=3), oa.PRBS(9, len=256, seed=77)
    ch = []
    for bits, df in ((bits1, -2e10), (bits2, 2e10)):
        drive = oa.DAC(bits, Vpp=5.0, offset=-2.5, pulse_shape="gaussian")
        ch.append(oa.MZM(oa.LASER(P0=3, df=df), drive, bias=-2.5, Vpi=5.0))
    noisy = optical_signal.from_device(ch[1]._raw("signal"), _lib.DeviceArray.from_host(1e-3 * (rng.standard_normal(4096) + 0j), np.complex128, 0))
    before = _lib.TRANSFERS["d2h"]
    both = ch[0] + ch[1]
    with_noise = ch[0] + noisy
    half = 0.5 * both
    atten = with_noise * 10 ** (-0.3)
    out = oa.FIBER(half, length=5, h=1.0, **workloads.SMF)
    assert all(x.on_device for x in (both, with_noise, half, atten, out)) and _lib.TRANSFERS["d2h"] == before
    a, b = ch[0].signal, ch[1].signal
    np.testing.assert_array_equal(both.signal, a + b)
    assert both.noise is NULL
    np.testing.assert_array_equal(with_noise.signal, a + b)
    np.testing.assert_array_equal(with_noise.noise, noisy.noise)
    np.testing.assert_array_equal(half.signal, 0.5 * (a + b))
    np.testing.assert_array_equal(atten.signal, (a + b) * 10 ** (-0.3))
    np.testing.assert_array_equal(atten.noise, noisy.noise * 10 ** (-0.3))
    assert within(out.signal, orc.fiber_c64(0.5 * (a + b), gv.dt, length=5, h=1.0, **workloads.SMF), steps=5, what="oracle")
    # everything else keeps the host path: other types, shapes, complex factors
    np.testing.assert_array_equal((both * (1 + 1j)).signal, (a + b) * (1 + 1j))
    np.testing.assert_array_equal((both + 1.0).signal, (a + b) + 1.0)


def test_device_array_basics():
    x = (np.arange(24).reshape(2, 12) * (1 + 0.5j)).astype(np.complex64)
    d = _lib.DeviceArray.from_host(x)
    assert d.shape == (2, 12) and d.dtype == np.complex64 and d.size == 24 and d.ndim == 2
    np.testing.assert_array_equal(d.to_host(), x)
    d128 = d.astype(np.complex128)
    np.testing.assert_array_equal(d128.to_host(), x.astype(np.complex128))
    np.testing.assert_array_equal(d128.astype(np.complex64).to_host(), x)
    np.testing.assert_array_equal((d + d).to_host(), x + x)
    ptr = d.ptr
    d.free()
    assert d.ptr == 0
    e = _lib.DeviceArray((2, 12), np.complex64)              # same size: comes back from the pool
    assert e.ptr == ptr
    with pytest.raises(TypeError):
        _lib.DeviceArray((4,), np.float32)


def test_devices_accept_the_reference_librarys_own_objects():
    """A script written against opticomlib swaps single devices: objects with the reference's layout go in,
    objects of the caller's class come out, and the sampling grid is the caller's gv (not ours)."""
    import foreign_types as ft
    ft.gv.set(**workloads.BENCH_GV)
    gv(sps=4, R=1e9)                                            # our own gv deliberately different
    a = workloads.qpsk_field(1 << 12, seed=33)
    kw = dict(length=3, h=1.0, **workloads.SMF)
    y = oa.FIBER(ft.optical_signal(a), **kw)
    assert type(y) is ft.optical_signal and isinstance(y.signal, np.ndarray) and y.noise is ft.NULL and y.execution_time > 0
    b = oa.BPF(oa.DBP(y, **kw), BW=100e9)
    v = oa.PD(b, BW=20e9, include_noise="none")
    assert type(b) is ft.optical_signal and type(v) is ft.electrical_signal
    d, H = oa.DM(ft.optical_signal(a[0]), D=10.0, retH=True)
    assert type(d) is ft.optical_signal and H.shape == (1 << 12,)
    gv(**workloads.BENCH_GV)                                    # the native path on the same grid gives the same numbers
    yn = oa.FIBER(optical_signal(a), **kw)
    np.testing.assert_array_equal(y.signal, yn.signal)
    vn = oa.PD(oa.BPF(oa.DBP(yn, **kw), BW=100e9), BW=20e9, include_noise="none")
    np.testing.assert_array_equal(v.signal, vn.signal)
    with pytest.raises(TypeError, match="`input` must be of type 'optical_signal'."):
        oa.FIBER(ft.electrical_signal(np.ones(256)), length=1)


def test_repeated_calls_do_not_leak_device_memory():
    """200 link chains of changing sizes: device buffers go back to the pool, plans are reused; free HBM does not
    drift by more than the pool's cap."""
    import gc
    gv(**workloads.BENCH_GV)
    kw = dict(length=2, h=1.0, **workloads.SMF)

    def chain(k, odd):
        n = (1 << k) - (17 if odd else 0)
        a = workloads.qpsk_field(1 << k, seed=k)[:, :n]
        y = oa.DBP(oa.FIBER(optical_signal(a), **kw), **kw)
        return oa.PD(oa.BPF(y, BW=100e9), BW=20e9, include_noise="none").signal

    for k in (10, 12, 13):
        chain(k, False), chain(k, True)                          # warm-up: plans and tables exist
    gc.collect()
    free0, total, pooled0 = _lib.device_mem_info()
    for i in range(200):
        chain((10, 12, 13)[i % 3], i % 2 == 1)
    gc.collect()
    free1, _, pooled1 = _lib.device_mem_info()
    assert total > 100 * 2 ** 30
    assert pooled1 <= 2 * 2 ** 30
    assert free0 - free1 < 256 * 2 ** 20, (free0, free1, pooled0, pooled1)


def test_plan_cycles_leak_nothing_and_change_nothing(monkeypatch):
    """Plans made, run and destroyed over and over: every resource a plan makes on first use -- the schedule on the device, operator tables, the one-launch
    engines' barrier words and pinned error words, the backup of the field, the z log, the capture's ring, input copy, scalar log, stream, events and
    helper thread, the scratch field, the transfer slots, the chirp line's tables and workspaces -- is made and given back in every cycle.  After three
    warm-up cycles, twenty more: free device memory does not drift, and every run's output, engine, fall-back flag and launch count are the first
    cycle's, bit for bit and count for count.

    The bound on the drift is the allocator's granularity and nothing else: the runtime hands device memory out in 2 MiB pieces.  Measured before the
    plan's members owned their buffers: a drift of 0 bytes over the twenty cycles; the bound is 2 MiB = 2097152 bytes above that."""
    import gc
    for k in ("SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_MEDIUM_SPLIT", "SSFM_ADAPT_FUSED", "SSFM_SMALL", "SSFM_CHIRP_SMALL", "SSFM_CHIRP_LOOP", "SSFM_FUSED_PATIENCE_TICKS",
              "SSFM_E", "SSFM_EF", "SSFM_EF_FLY", "SSFM_LANES", "SSFM_FORCE_FLY", "SSFM_PHASE_TABLE"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()
    gv(**workloads.BENCH_GV)
    parent_drift, granularity = 0, 2 << 20
    field = workloads.qpsk_field(1 << 14, seed=5, power_w=4e-3, n_pol=2).astype(np.complex64)
    sched = np.array([0.5] * 7 + [0.25], dtype=np.float32)
    ops = {n: np.asarray(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, _lib.C64), dtype=np.complex64) for n in (1 << 10, 1 << 12, 1 << 13, 1 << 14)}
    H = np.exp(-np.square(np.fft.fftfreq(1 << 12) * 8.0)).astype(np.complex64)              # an LPF-like transfer function
    chirps = {n: (_lib.chirp_device(n, False, 0).astype(np.complex64),
                  _lib.DeviceArray.from_host(np.asarray(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, _lib.C64), dtype=np.complex64), np.complex64, 0))
              for n in (1001, 5001)}
    hs64 = np.array([0.5] * 7 + [0.25], dtype=np.float64)
    op128 = np.asarray(oa.devices.linear_operator(1 << 14, gv.dt, 0.2, -21.7, 0.13, _lib.C128), dtype=np.complex128)

    def on_plan(n, batch, body, prec=_lib.C64):
        p = _lib.Plan(n, batch, prec)
        try:
            out = body(p)
            info = p.last_run_info()
            return [np.array(o, copy=True) for o in out], (info["engine"], info["fell_back"], p.last_propagate_ms()[1])
        finally:
            p.close()

    def fixed(n, batch):
        def body(p):
            p.set_linear_operator(ops[n]); p.set_field(field[:batch, :n]); p.propagate_fixed(1.3, sched)
            return [p.get_field()]
        return on_plan(n, batch, body)

    def fixed_capture(p):          # (a complex128 plan transforms its field in place: the capture keeps a copy of the input as well)
        p.set_linear_operator(op128); p.set_field(field)
        c = p.propagate_fixed_capture(1.3, hs64, every=2, scalars=True)
        return [c["steps"], c["fields"], c["power"], c["peak"], p.get_field()]

    def adaptive(p):
        p.set_linear_operator(ops[1 << 14]); p.set_field(field)
        steps, z, _ = p.propagate_adaptive(1.3, 4.0, 0.004, False)
        return [np.int64(steps), z, p.get_field()]

    def adaptive_capture(p):
        p.set_linear_operator(ops[1 << 14]); p.set_field(field)
        steps, z, taken, fields = p.propagate_adaptive_capture(1.3, 4.0, 0.004, every=2, capacity=64)
        return [np.int64(steps), z, taken, fields, p.get_field()]

    def transfers(p):
        p.set_field(field[:, : 1 << 12])
        Hd = p.apply_dispersion(gv.dt, 3.4e-23, want_H=True)          # DM: the scratch field
        a = p.get_field()
        p.apply_transfer(H)
        b = p.get_field()
        p.transfer_table(H, 0); p.transfer_table(np.conj(H), 1)        # the resident slots
        p.apply_table(0); p.apply_table(1)
        return [Hd, a, b, p.get_field()]

    def chirp(n):
        def body(p):
            A = _lib.DeviceArray.from_host(field[:, :n], np.complex64, 0)
            assert p.chirp_propagate_c64(A, chirps[n][0], chirps[n][1], 1.3, hs64) is True
            p.synchronize()                                     # (the small line's fixed-step run is asynchronous, A is not the plan's field)
            return [A.to_host()]
        return body

    def cycle():
        got = [fixed(1 << 10, 1), fixed(1 << 13, 2), on_plan(1 << 14, 2, fixed_capture, _lib.C128), on_plan(1 << 14, 2, adaptive), on_plan(1 << 14, 2, adaptive_capture),
               on_plan(1 << 12, 2, transfers), on_plan(1 << 11, 2, chirp(1001)), on_plan(1 << 14, 2, chirp(5001))]
        oa.devices.release_plans()
        return got

    first = cycle()
    print("engines of a cycle:", [info for _, info in first])
    assert [info[0] for _, info in first[:2]] == ["small", "medium"], first[0][1:]             # the engines the sizes were chosen for
    assert [info[0] for _, info in first[6:]] == ["chirp_small", "chirp_medium"]
    assert not any(info[1] for _, info in first)

    def same_as_first(got, i):
        for k, ((outs, info), (outs0, info0)) in enumerate(zip(got, first)):
            assert info == info0, (i, k, info, info0)
            assert len(outs) == len(outs0)
            for a, b in zip(outs, outs0):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (i, k, info)

    for i in range(2):
        same_as_first(cycle(), i + 1)
    gc.collect()
    free0, _, pooled0 = _lib.device_mem_info()
    for i in range(20):
        same_as_first(cycle(), i + 3)
    gc.collect()
    free1, _, pooled1 = _lib.device_mem_info()
    print(f"free device memory after the warm-up {free0}, after twenty cycles {free1}: drift {free0 - free1} bytes (pooled {pooled0} -> {pooled1})")
    assert abs(free0 - free1) <= parent_drift + granularity, (free0, free1, pooled0, pooled1)


def test_c_abi_from_plain_c(tmp_path):
    """examples/c_abi_demo.c: the shared library used from C with nothing but include/ssfm_amd.h."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_demo")
    libdir = os.path.join(root, "opticomlib_amd")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_abi_demo.c"), "-o", exe,
                    "-L" + libdir, "-l:_ssfm_amd.so", "-lm", "-Wl,-rpath," + libdir], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SSFM_")}          # (the knob suite's settings are not the demo's business)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ABI version 3" in r.stdout and "back-propagated" in r.stdout
    assert "last run: engine 4, fell back 0" in r.stdout or "last run: engine 5, fell back 0" in r.stdout        # (budgeted adaptive calls: a launch-per-pass engine)
    assert "operator label after set: 0x5eed, after a new operator: 0" in r.stdout          # the plan cleared the label itself
    assert "adaptive:" in r.stdout and "z_end = 20.000000 km" in r.stdout
    assert "PRBS-7: 10000001000001100001" in r.stdout                                         # reference tests/devices_test.py:52-71


# ----------------------------------------------------------------------- API behaviour on the device
def test_call_order_and_argument_errors():
    p = _lib.Plan(4096, 2, _lib.C64)
    try:
        with pytest.raises(oa.SsfmError, match="ssfm_set_linear_operator first"):
            p.propagate_fixed(1.3, np.ones(3, np.float32))
        p.set_linear_operator(np.zeros(4096, np.complex64))
        with pytest.raises(oa.SsfmError, match="must be finite and > 0"):
            p.propagate_fixed(1.3, np.array([1.0, 0.0], np.float32))
        with pytest.raises(ValueError):
            p.set_linear_operator(np.zeros(100, np.complex64))
    finally:
        p.close()
    with pytest.raises(oa.SsfmError, match="power of two"):
        _lib.Plan(3000, 2, _lib.C64)
    with pytest.raises(oa.SsfmError, match="not available"):
        _lib.Plan(4096, 2, _lib.C64, device=99)
    # every `int device` entry point: a device that is not there is SSFM_ERR_NO_DEVICE, checked before anything is touched
    lib = _lib.load()
    buf = _lib.DeviceArray((1 << 16,), np.complex128)
    p = buf.ptr
    sos, zi = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]), np.zeros((1, 2))
    tg, yset = np.zeros(64), np.zeros(4)
    host = np.zeros(1 << 14)
    ptr = _lib._ptr
    i64, i32, u32, dbl = C.byref(C.c_int64()), C.byref(C.c_int()), C.byref(C.c_uint32()), C.byref(C.c_double())
    fl, sz, vp = C.byref(C.c_float()), C.byref(C.c_size_t()), C.byref(C.c_void_p())
    info = (C.c_int64 * 3)()
    calls = {
        "ssfm_plan_create": lambda: lib.ssfm_plan_create(vp, 99, 4096, 2, _lib.C64),
        "ssfm_sosfiltfilt": lambda: lib.ssfm_sosfiltfilt(99, ptr(sos), ptr(zi), 1, p, p, 1024, 1, 0, 1),
        "ssfm_sosfiltfilt_last": lambda: lib.ssfm_sosfiltfilt_last(99, fl, i32),
        "ssfm_sosfiltfilt_last_route": lambda: lib.ssfm_sosfiltfilt_last_route(99, (C.c_int * 8)()),
        "ssfm_square_law": lambda: lib.ssfm_square_law(99, p, None, 1, 1024, 1.0, 1.0, p, None, 1),
        "ssfm_square_law (host)": lambda: lib.ssfm_square_law(99, ptr(host), None, 1, 1024, 1.0, 1.0, ptr(host), None, 0),
        "ssfm_device_alloc": lambda: lib.ssfm_device_alloc(99, 1024, vp),
        "ssfm_device_free": lambda: lib.ssfm_device_free(99, p, 1024),
        "ssfm_device_copy": lambda: lib.ssfm_device_copy(99, p, p, 1024, _lib.COPY_D2D),
        "ssfm_device_convert": lambda: lib.ssfm_device_convert(99, p, _lib.C128, p, _lib.C64, 1024),
        "ssfm_device_add": lambda: lib.ssfm_device_add(99, p, p, p, _lib.C128, 1024),
        "ssfm_device_randn": lambda: lib.ssfm_device_randn(99, p, 1024, 1, 0, 0.0, 1.0),
        "ssfm_device_sum3": lambda: lib.ssfm_device_sum3(99, p, p, None, None, 0.0, 1.0, 1024),
        "ssfm_device_scale_add": lambda: lib.ssfm_device_scale_add(99, p, p, 1.0, None, 1024),
        "ssfm_device_cumsum": lambda: lib.ssfm_device_cumsum(99, p, p, 1024),
        "ssfm_mzm": lambda: lib.ssfm_mzm(99, p, None, p, None, 1, 1024, p, None, 0, 1.0, 0.0, 1.0, 0.0, 0),
        "ssfm_laser": lambda: lib.ssfm_laser(99, p, 1024, 1.0, None, None, 0, 0.0, 1.0, 1.0),
        "ssfm_device_axpb": lambda: lib.ssfm_device_axpb(99, p, p, 1.0, 0.0, 1024, 0),
        "ssfm_device_shift": lambda: lib.ssfm_device_shift(99, p, p, 1024, 0, 1.0, 0.0),
        "ssfm_device_reduce": lambda: lib.ssfm_device_reduce(99, _lib.REDUCE_MEAN, p, None, 1, 1024, 0, dbl),
        "ssfm_prbs": lambda: lib.ssfm_prbs(99, p, 1024, 7, 1, u32),
        "ssfm_device_mem_info": lambda: lib.ssfm_device_mem_info(99, sz, sz, sz),
        "ssfm_device_chirp": lambda: lib.ssfm_device_chirp(99, p, 1024, 0),
        "ssfm_device_sort_f64": lambda: lib.ssfm_device_sort_f64(99, p, 1024),
        "ssfm_eye_prepare": lambda: lib.ssfm_eye_prepare(99, p, None, 0, 1024, 0, p),
        "ssfm_eye_resample_stage": lambda: lib.ssfm_eye_resample_stage(99, 0, p, 1024, p, 1024),
        "ssfm_eye_estimate": lambda: lib.ssfm_eye_estimate(99, p, 1024, ptr(tg), 32, ptr(yset), yset.size, ptr(host), 64, i64),
        "ssfm_eye_levels": lambda: lib.ssfm_eye_levels(99, p, 1024, 32, 0, 16, 0.5, 500, ptr(host), 64),
        "ssfm_device_sample": lambda: lib.ssfm_device_sample(99, p, None, 0, 2, 256, 0.5, None, p),
        "ssfm_device_count_diff": lambda: lib.ssfm_device_count_diff(99, p, p, 1024, i64),
        "ssfm_ppm_encode": lambda: lib.ssfm_ppm_encode(99, p, 256, 4, p),
        "ssfm_ppm_decode": lambda: lib.ssfm_ppm_decode(99, p, 1024, 4, None, 0, i64),
        "ssfm_ppm_decide": lambda: lib.ssfm_ppm_decide(99, p, None, 0, 0, 1, 256, 4, 1, 0.5, p, None, p),
        "ssfm_ppm_faulty": lambda: lib.ssfm_ppm_faulty(99, p, 256, p, p, i64),
        "ssfm_ppm_resolve": lambda: lib.ssfm_ppm_resolve(99, p, None, 0, 0, 1, 256, 4, 0.5, p, None, None, 0, 1, 0, p, None),
        "ssfm_fbg_solve": lambda: lib.ssfm_fbg_solve(99, 1024, ptr(host), ptr(host), ptr(host), 0.0, 0, 1e-6, 1e-9, None, None, p, info),
        "ssfm_fbg_delay": lambda: lib.ssfm_fbg_delay(99, p, p + (1 << 16), 1024, 1e-12, 0.0, 0),
        "ssfm_pm": lambda: lib.ssfm_pm(99, p, None, p, None, 1, 1024, p, None, 0, 1.0),
        "ssfm_shortest_int": lambda: lib.ssfm_shortest_int(99, p, 1024, 50.0, ptr(host)),
        "ssfm_adc_quantize": lambda: lib.ssfm_adc_quantize(99, p, 1024, -1.0, 1.0, 16, 0, p),
        "ssfm_welch": lambda: lib.ssfm_welch(99, p, _lib.C128, 1, 1024, 1024, 256, 1.0, 0, p),
        "ssfm_welch_frames": lambda: lib.ssfm_welch_frames(99, p, _lib.C128, 1, 1024, 1024, 256, 0, 7, 8, p),
        "ssfm_welch_accumulate": lambda: lib.ssfm_welch_accumulate(99, p, 256, 1, 7, 0, 7, p),
        "ssfm_welch_finish": lambda: lib.ssfm_welch_finish(99, p, 1, 256, 1.0, 0, p),
    }
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssfm_amd.h")).read()
    names = set(re.findall(r"SSFM_API int (ssfm_\w+)\((?:ssfm_plan\*\* out, )?int device", hdr))
    assert names == {k.split()[0] for k in calls}
    for name, call in calls.items():
        assert call() == 4, (name, lib.ssfm_last_error())


def test_many_rows_equal_separate_runs():
    """Rows never interact in fixed-step mode: 3 fields (6 rows, two lanes of 3) propagated in one plan
    are bit-identical to 3 separate dual-pol calls; the plan/operator cache survives parameter changes."""
    gv(**workloads.BENCH_GV)
    n = 1 << 14
    fields = [workloads.prbs_field(n, seed=s) for s in (1, 2, 3)]
    kw = dict(length=6, h=0.5, **workloads.SMF)
    sep = [oa.FIBER(optical_signal(f), **kw).signal for f in fields]
    other = oa.FIBER(optical_signal(fields[0]), length=3, h=0.5, alpha=0.1, beta_2=-5.0, gamma=2.0).signal
    again = oa.FIBER(optical_signal(fields[0]), **kw).signal
    np.testing.assert_array_equal(again, sep[0])
    assert relmax(other, sep[0]) > 1e-3
    hs, _ = oa.devices.step_schedule(6, 0.5)
    p = _lib.Plan(n, 6, _lib.C64)
    try:
        p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13))
        p.set_field(np.concatenate(fields).astype(np.complex64))
        p.propagate_fixed(1.3, hs)
        out = p.get_field().reshape(3, 2, n)
    finally:
        p.close()
    for k in range(3):
        np.testing.assert_array_equal(out[k], sep[k])


def test_fiber_then_dbp_prbs_realisations_against_oracle():
    """Configuration C4 in miniature: FIBER(100 x 1 km) then DBP on LFSR-PRBS realisations; parity is
    against the reference-semantics DBP output (the stale-N^ round trip is not the identity)."""
    gv(**workloads.BENCH_GV)
    kw = dict(length=20, h=1.0, **workloads.SMF)
    for seed in (1, 2):
        a = workloads.prbs_field(1 << 14, seed=seed, power_w=4e-3)
        y = oa.FIBER(optical_signal(a), **kw)
        x_hat = oa.DBP(y, **kw).signal
        ref = orc.dbp_c64(orc.fiber_c64(a, gv.dt, **kw), gv.dt, **kw)
        assert within(x_hat, ref, steps=2 * steps_of(kw), what="oracle FIBER + DBP, PRBS realisation")
        assert relmax(x_hat, a.astype(np.complex64)) > 10 * relmax(x_hat, ref)


def test_progress_bar_path_agrees():
    """show_progress splits the run into chunks at sync points; at a chunk seam the two nonlinear half
    rotations are applied separately instead of merged, so agreement is to rounding, not bitwise."""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 13, seed=9)
    kw = dict(length=30, h=0.3, **workloads.SMF)
    y0 = oa.FIBER(optical_signal(a), **kw).signal
    y1 = oa.FIBER(optical_signal(a), show_progress=True, **kw).signal
    assert within(y1, y0, 1e-5, kw=kw, what="progress-bar run against the plain run")


def test_progress_bar_on_every_engine(capsys):
    """show_progress with fixed and adaptive steps, power-of-two and other lengths: same results as without."""
    gv(**workloads.BENCH_GV)
    for n in (1 << 12, 3000):
        a = workloads.qpsk_field(1 << 12, seed=8, power_w=5e-3)[:, :n]
        for kw in (dict(length=5, h=0.5, **workloads.SMF), dict(length=5, phi_max=0.02, **workloads.SMF)):
            y0 = oa.FIBER(optical_signal(a), **kw).signal
            y1 = oa.FIBER(optical_signal(a), show_progress=True, **kw).signal
            assert within(y1, y0, 1e-5)
            z, A_z = oa.FIBER(optical_signal(a), show_progress=True, return_steps=True, **kw)
            assert within(A_z[-1], y0, 1e-5) and len(z) == A_z.shape[0]


def test_zero_and_negative_length_return_the_cast_input():
    """reference: the loop `while z < length` never runs (devices.py:1172) and the input comes back as complex64."""
    gv(sps=16, R=10e9)
    a = workloads.qpsk_field(1 << 10, seed=4)
    for L in (0.0, -5.0):
        y = oa.FIBER(optical_signal(a), length=L, h=1.0, alpha=0.2, beta_2=-20, gamma=2).signal
        np.testing.assert_array_equal(y, a.astype(np.complex64))
        z, A_z = oa.FIBER(optical_signal(a), length=L, h=1.0, gamma=2, return_steps=True)
        assert z.tolist() == [0.0] and A_z.shape == (1, 2, 1 << 10)


def test_propagate_channels_batches_fields_in_one_plan():
    """dist.propagate_channels (single process): fixed-step fields go through one plan and equal
    separate FIBER calls bit for bit; adaptive fields run one by one."""
    from opticomlib_amd import dist as od
    gv(**workloads.BENCH_GV)
    n = 1 << 13
    fields = np.stack([workloads.qpsk_field(n, seed=3000 + c) for c in range(3)])
    kw = dict(length=8, h=0.5, **workloads.SMF)
    outs = od.propagate_channels(fields, gv.dt, **kw)
    assert len(outs) == 3
    for c in range(3):
        np.testing.assert_array_equal(outs[c], oa.FIBER(optical_signal(fields[c]), **kw).signal)
    kwa = dict(length=8, **workloads.SMF)
    outs = od.propagate_channels(fields, gv.dt, **kwa)
    for c in range(3):
        np.testing.assert_array_equal(outs[c], oa.FIBER(optical_signal(fields[c]), **kwa).signal)


def test_propagate_channels_fiber_then_dbp_on_device():
    """C4's chain with dbp=True: forward and back-propagation of all realisations in one plan, the field
    never leaving the GPU in between -- bit-identical to DBP(FIBER(x)) through the host API, and within
    tolerance of the oracle's DBP(FIBER(x))."""
    from opticomlib_amd import dist as od
    gv(**workloads.BENCH_GV)
    n = 1 << 13
    fields = np.stack([workloads.prbs_field(n, seed=s, power_w=4e-3) for s in (1, 2, 3)])
    kw = dict(length=10, h=0.5, **workloads.SMF)
    outs = od.propagate_channels(fields, gv.dt, dbp=True, **kw)
    for c in range(3):
        via_host = oa.DBP(oa.FIBER(optical_signal(fields[c]), **kw), **kw).signal
        np.testing.assert_array_equal(outs[c], via_host)
    ref = orc.dbp_c64(orc.fiber_c64(fields[0], gv.dt, **kw), gv.dt, **kw)
    assert within(outs[0], ref, steps=2 * steps_of(kw), what="oracle FIBER + DBP")
    one = od.propagate_channels(fields[:1], gv.dt, dbp=True, **kw)             # single unit: host-API branch
    np.testing.assert_array_equal(one[0], outs[0])
    odd = fields[:2, :, :3000]                                                 # not a power of two: one by one, chirp-z
    got = od.propagate_channels(odd, gv.dt, **kw)
    assert within(got[1], orc.fiber_c64(odd[1], gv.dt, **kw), kw=kw, what="oracle, 3000 samples")


# ----------------------------------------------------------------------- symmetries of the propagator
@pytest.mark.parametrize("prec,tol", [("complex64", 2e-5), ("complex128", 1e-11)])
def test_symmetries_shift_and_global_phase(prec, tol):
    """The scalar NLSE with periodic boundaries commutes with circular time shifts and with a global phase
    (also numerically: every operator of the scheme does).  Size-independent properties, run at 2^18 x 2."""
    gv(**workloads.BENCH_GV)
    n = 1 << 18
    a = workloads.qpsk_field(n, seed=21)
    kw = dict(length=20, h=0.5, precision=prec, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    ys = oa.FIBER(optical_signal(np.roll(a, 12345, axis=-1)), **kw).signal
    assert within(ys, np.roll(y, 12345, axis=-1), tol, steps=40, what="shift symmetry")
    ph = np.exp(0.7j)
    yp = oa.FIBER(optical_signal(a * ph), **kw).signal
    assert within(yp, y * ph, tol, steps=40, what="global phase symmetry")


def test_gaussian_broadening_and_soliton_closed_forms():
    """Analytic solutions of the equation the fibre solves (not taken from the reference): a Gaussian pulse in a linear
    dispersive fibre, A(z,t) = T0/sqrt(q) exp(-t^2 / 2q), q = T0^2 - j beta_2 z; the fundamental soliton
    sqrt(P0) sech(t/T0) with gamma P0 T0^2 = |beta_2|, which only acquires the phase gamma P0 z / 2 -- reproduced with
    the second-order accuracy of the symmetric split step; and energy conservation without attenuation."""
    N, dt = 1 << 14, 0.5e-12
    gv(sps=16, R=1 / (16 * dt))
    assert gv.dt == pytest.approx(dt, rel=1e-12)
    t = (np.arange(N) - N // 2) * gv.dt * 1e12                     # ps
    T0, b2, g = 10.0, -21.7, 1.3
    q = T0 ** 2 - 1j * b2 * 20.0
    pulse = np.exp(-t ** 2 / (2 * T0 ** 2)).astype(complex)
    want = T0 / np.sqrt(q) * np.exp(-t ** 2 / (2 * q))
    for prec, tol in (("complex128", 1e-12), ("complex64", 5e-6)):
        got = oa.FIBER(optical_signal(pulse), length=20.0, h=1.0, beta_2=b2, precision=prec).signal
        assert np.max(np.abs(got - want)) < tol
        got = oa.FIBER(optical_signal(pulse), length=20.0, beta_2=b2, precision=prec).signal      # adaptive: one step
        assert np.max(np.abs(got - want)) < tol
    assert np.max(np.abs(oa.DM(optical_signal(pulse), D=b2 * 20.0).signal - want)) < 1e-12
    P0 = abs(b2) / (g * T0 ** 2)
    sol = (np.sqrt(P0) / np.cosh(t / T0)).astype(complex)
    want = sol * np.exp(1j * g * P0 * 10.0 / 2)
    err = {}
    for h in (0.1, 0.05):
        got = oa.FIBER(optical_signal(sol), length=10.0, h=h, beta_2=b2, gamma=g, precision="complex128").signal
        err[h] = np.max(np.abs(got - want)) / np.sqrt(P0)
        assert abs(np.sum(np.abs(got) ** 2) / np.sum(np.abs(sol) ** 2) - 1) < 1e-12
    assert err[0.1] < 2e-4 and 3.5 < err[0.1] / err[0.05] < 4.5    # second order in the step size
    got = oa.FIBER(optical_signal(sol), length=10.0, h=0.05, beta_2=b2, gamma=g).signal
    assert np.max(np.abs(got - want)) / np.sqrt(P0) < 2e-4 and abs(np.sum(np.abs(got) ** 2) / np.sum(np.abs(sol) ** 2) - 1) < 1e-4
    back = oa.DBP(oa.FIBER(optical_signal(sol), length=10.0, h=0.05, beta_2=b2, gamma=g, precision="complex128"),
                  length=10.0, h=0.05, beta_2=b2, gamma=g, precision="complex128").signal
    assert np.max(np.abs(back - sol)) / np.sqrt(P0) < 1e-4          # back-propagation undoes the fibre (to the splitting error)


def test_linearity_without_kerr_effect():
    """gamma = 0: the fibre is linear -- FIBER(a x1 + b x2) = a FIBER(x1) + b FIBER(x2)."""
    gv(**workloads.BENCH_GV)
    n = 1 << 16
    x1 = workloads.qpsk_field(n, seed=31)
    x2 = workloads.qpsk_field(n, seed=32)
    kw = dict(length=50, h=2.0, alpha=0.2, beta_2=-21.7, beta_3=0.13, precision="complex128")
    f = lambda x: oa.FIBER(optical_signal(x), **kw).signal
    lhs = f(0.3 * x1 + (0.2 - 0.9j) * x2)
    rhs = 0.3 * f(x1) + (0.2 - 0.9j) * f(x2)
    assert within(lhs, rhs, 1e-12)


def test_two_to_the_22_against_oracle():
    """Largest supported size (N1 = 512 column tiles, 8192-point rows): 2^22 x 1, three steps."""
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(1 << 22, seed=5, n_pol=1)[0]
    kw = dict(length=3 * 0.25, h=0.25, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    ref = orc.fiber_c64(a, gv.dt, **kw)
    assert within(y, ref, kw=kw, what="oracle, 2^22 x 1")
    y21 = oa.FIBER(optical_signal(a[: 1 << 21]), **kw).signal
    assert within(y21, orc.fiber_c64(a[: 1 << 21], gv.dt, **kw), kw=kw, what="oracle, 2^21 x 1")


# ----------------------------------------------------------------------- PRBS on the device
def test_prbs_bit_exact_against_golden_and_oracle(golden_dir):
    """The HIP generator (ssfm_prbs) against vectors captured from the reference, the reference's own literal test
    vectors (tests/devices_test.py:52-71) and the serial oracle on random orders / seeds / lengths, incl. the final
    register state (return_seed) and every chunk boundary of the kernel (256 bits per thread)."""
    from oracle import prbs_numpy as po
    from test_oracle_golden import REF_PRBS_20
    for name, case in CASES.items():
        if case["func"] != "PRBS":
            continue
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        seq, last = oa.PRBS(return_seed=True, **case["kw"])
        assert isinstance(seq, oa.binary_sequence) and seq.type is oa.binary_sequence
        assert isinstance(seq._raw(), _lib.DeviceArray) and len(seq) == g["out"].size          # still on the device, size known
        assert seq.data.dtype == np.uint8
        np.testing.assert_array_equal(seq.data, g["out"])
        assert last == int(g["seed_out"])
    for order, want in REF_PRBS_20.items():
        assert oa.PRBS(order=order, len=20).data.tolist() == want
    rng = np.random.default_rng(7)
    for order in po.TAPS:
        for _ in range(12):
            n, seed = int(rng.integers(1, 4000)), int(rng.integers(1, 1 << 40))
            if seed % (1 << order) == 0:
                continue
            a, la = oa.PRBS(order, n, seed, return_seed=True)
            b, lb = po.prbs(order, n, seed)
            np.testing.assert_array_equal(a.data, b)
            assert la == lb
    for n in (1, 255, 256, 257, 511, 512, 65536, 65537, (1 << 18) + 3):
        a, la = oa.PRBS(23, n, seed=0x2f3a1, return_seed=True)
        b, lb = po.prbs(23, n, 0x2f3a1)
        np.testing.assert_array_equal(a.data, b)
        assert la == lb
    # continuing from the returned state reproduces the uninterrupted sequence
    a, st = oa.PRBS(15, 1000, seed=99, return_seed=True)
    b = oa.PRBS(15, 500, seed=st)
    np.testing.assert_array_equal(np.concatenate([a.data, b.data]), oa.PRBS(15, 1500, seed=99).data)
    assert np.all(oa.PRBS(7, len=2 * 127) == oa.PRBS(7, len=127).data.tolist() * 2)
    with pytest.warns(UserWarning, match="changed to 1"):
        assert oa.PRBS(7, len=10, seed=0).data.tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0]          # devices_test.py:57
    assert oa.PRBS(7).size == 127
    with pytest.raises(oa.SsfmError, match="not a state"):
        _lib.prbs_device(7, 10, 0)


def test_prbs_feeds_the_dac_without_leaving_the_gpu():
    """PRBS -> DAC: the bits go from the generator's kernel into the pulse shaper's input in GPU memory -- no
    upload, no download -- and the drive signal equals the one shaped from the same bits given as a host array."""
    gv(sps=16, R=10e9, N=512)
    before = dict(_lib.TRANSFERS)
    bits = oa.PRBS(15, len=512, seed=77)
    v = oa.DAC(bits, Vpp=2.0, pulse_shape="rcos", beta=0.3)
    assert _lib.TRANSFERS == before and isinstance(v._raw("signal"), _lib.DeviceArray)
    v_host = oa.DAC(bits.data.copy(), Vpp=2.0, pulse_shape="rcos", beta=0.3)
    np.testing.assert_array_equal(v.signal, v_host.signal)


def test_c4_realisation_generated_on_the_device():
    """workloads.prbs_field_device (LFSR bits, symbols, Gaussian shaping, power normalisation: all HIP) against the
    host construction from the oracle's LFSR: equal to the rounding of the two FFTs, exact power, nothing uploaded
    per realisation once the shaping filter is resident."""
    from oracle import prbs_numpy as po
    n, sps = 1 << 14, 16
    for seed in (1, 5, 1 << 15):                                  # (2^15 is 0 modulo 2^order: becomes 1)
        bits, _ = po.prbs(15, 4 * (n // sps), seed)
        b = bits.reshape(2, n // sps, 2).astype(np.int64)
        sym = ((2 * b[..., 0] - 1) + 1j * (2 * b[..., 1] - 1)) / np.sqrt(2)
        want = workloads._shape_pulses(sym, n, sps, 1e-3)
        before = _lib.TRANSFERS["h2d"]
        got = workloads.prbs_field_device(n, seed=seed)
        if seed != 1:
            assert _lib.TRANSFERS["h2d"] == before               # (the first call uploads the shaping filter once)
        assert got.shape == (2, n) and got.dtype == np.complex64
        g = got.to_host()
        assert within(g, want, 3e-7)
        np.testing.assert_allclose(np.mean(np.abs(g.astype(np.complex128)) ** 2, axis=-1), 1e-3, rtol=1e-6)
    np.testing.assert_array_equal(workloads.prbs_field(n, seed=5).astype(np.complex64).shape, (2, n))


def test_full_size_c4_against_the_strided_fixture(golden_dir):
    """Configuration C4 at its stated size: a realisation generated on the device from the LFSR seed, FIBER(100 x 1 km)
    then DBP(100 x 1 km) without leaving the GPU, against the committed fixture of the oracle's chain
    (tests/golden/make_c4_strided.py): every 257th sample, power and energy after FIBER and after DBP."""
    from opticomlib_amd import dist as od
    g = np.load(os.path.join(golden_dir, "c4_full_strided.npz"))
    gv(**workloads.BENCH_GV)
    n = 1 << 20
    a = workloads.prbs_field_device(n, seed=int(g["seed"]))
    assert within(a.to_host()[:, ::257], g["input_samples"], 3e-7)
    kw = dict(length=100, h=1.0, **workloads.SMF)
    y = oa.FIBER(optical_signal.from_device(a), **kw)
    x = oa.DBP(y, **kw)
    for got, key, ns in ((y.signal, "fiber", 100), (x.signal, "dbp", 200)):
        # the FIBER leg at tol(100) = 2e-5, FIBER + DBP at tol(200) = 4.5e-5 (rounds 4-5 held both to 6e-5)
        assert within(got[:, ::257], g[key + "_samples"], steps=ns, what=f"C4 full size, the oracle's strided fixture, {key} leg")
        p2 = np.abs(got.astype(np.complex128)) ** 2
        np.testing.assert_allclose(np.mean(p2, axis=-1), g[key + "_power"], rtol=1e-4)
        np.testing.assert_allclose(np.sum(p2), float(g[key + "_energy"]), rtol=1e-4)
    # the sharded entry point on device-resident units gives the same bits (one unit, one rank)
    stacked = _lib.DeviceArray((1, 2, n), np.complex64)
    _lib._check(_lib.load().ssfm_device_copy(0, _lib._VP(stacked.ptr), _lib._VP(a.ptr), a.nbytes, 2), "ssfm_device_copy")
    out = od.propagate_channels(stacked, gv.dt, dbp=True, **kw)
    np.testing.assert_array_equal(out[0], x.signal)


# ----------------------------------------------------------------------- what a plan holds is the plan's knowledge
def test_sweeping_a_parameter_through_minus_one_and_minus_two_restages_the_operator():
    """hash(-1.0) == hash(-2.0): with hash-derived plan labels the second call of such a sweep silently reused the first
    call's operator.  Every call of the sweep must match the oracle for ITS parameters, also through DBP's
    negated ones."""
    gv(sps=8, R=16e9, N=64)
    n = 4096
    rng = np.random.default_rng(11)
    a = ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.03).astype(np.complex64)
    x = optical_signal(a)
    for fn, orc_sign in ((oa.FIBER, 1.0), (oa.DBP, -1.0)):
        for name in ("beta_2", "beta_3", "alpha"):
            for val in (-1.0, -2.0, 1.0, 2.0):
                kw = dict(length=3, h=1.0, alpha=0.2, beta_2=-20.0, beta_3=0.1, gamma=1.5)
                kw[name] = val
                okw = {k: (orc_sign * v if k in ("alpha", "beta_2", "beta_3", "gamma") else v) for k, v in kw.items()}
                want = orc.fiber_c64(a, gv.dt, **okw)
                assert within(fn(x, **kw).signal, want, kw=kw, what=f"oracle, {fn.__name__} {name}={val}"), (fn.__name__, name, val)


def test_interleaved_users_of_one_plan_never_see_a_stale_table():
    """FIBER (complex128), DM, DAC, a chirp-z FIBER and x('w') all end up on complex128 plans of the same length and
    batch and reuse its operator staging and table slots.  Which operator / table is staged is tracked by the C plan
    (ssfm_plan_set_tag / _get_tag): interleaving the users in every order must give each its oracle result."""
    from oracle import transmitter_numpy as tx
    gv(sps=8, R=16e9, N=64)
    n = 4096
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.03
    kw = dict(length=4, h=1.0, alpha=0.2, beta_2=-21.7, beta_3=0.1, gamma=1.5)
    want_f = orc.fiber_c128(a, gv.dt, **kw)
    want_dm = orc.dm_c128(a, gv.dt, -300.0)[0]
    bits = (rng.integers(0, 2, 256)).astype(np.uint8)                    # 256 x 8 = 2048 samples -> DAC plan of 4096 points
    want_dac = tx.dac(bits, 8, gv.fs, pulse_shape="gaussian", Vpp=1.5)
    odd = a[:2001]                                                       # chirp-z on a 4096-point plan
    want_odd = orc.fiber_c64(odd, gv.dt, **kw)
    want_w = np.fft.fft(odd)

    def fiber():
        assert within(oa.FIBER(optical_signal(a), precision="complex128", **kw).signal, want_f, TOL_C128)

    def dm():
        assert within(oa.DM(optical_signal(a), D=-300.0).signal, want_dm, 1e-12)

    def dac():
        assert within(oa.DAC(bits, Vpp=1.5, pulse_shape="gaussian").signal, want_dac, 1e-12)

    def odd_fiber():
        assert within(oa.FIBER(optical_signal(odd), **kw).signal, want_odd, TOL_100)

    def spectrum():
        assert within(optical_signal(odd)("w").signal, want_w, 1e-12)

    users = [fiber, dm, dac, odd_fiber, spectrum]
    import itertools
    for order in list(itertools.permutations(range(5)))[::7]:            # 18 of the 120 orders, every user in every position
        for k in order:
            users[k]()
    for u in users:                                                      # and repeated calls hit the cached state
        u(); u()
    # the tags themselves: a label survives until the buffer is reused
    p = _lib.Plan(n, 1, _lib.C128)
    try:
        assert p.tag(0) == 0 and p.tag(1) == 0
        p.set_linear_operator(np.zeros(n, complex)); p.set_tag(0, 17)
        assert p.tag(0) == 17
        p.transfer_table(np.ones(n, complex), 0); p.set_tag(1, 5)
        assert p.tag(0) == 0 and p.tag(1) == 5                           # the upload went through the operator's staging buffer
        p.set_field(a); p.table_from_field(0)
        assert p.tag(1) == 0
        p.set_linear_operator(np.zeros(n, complex)); p.set_tag(0, 9)
        p.apply_dispersion(gv.dt, 1e-24, want_H=True)
        assert p.tag(0) == 0
    finally:
        p.close()


def test_no_host_arithmetic_left_in_the_device_paths():
    """Transfer counters: the Bluestein kernels, LPF of a complex device signal, AC coupling of a complex pulse and the
    empty polarisation of an EDFA are all made on the device (round-1 versions went through NumPy)."""
    gv(sps=16, R=10e9, N=128)
    rng = np.random.default_rng(5)
    x = _lib.DeviceArray.from_host((rng.standard_normal(3000) + 1j * rng.standard_normal(3000)) * 0.05, np.complex128)
    oa.devices._CHIRPS.clear()
    before = dict(_lib.TRANSFERS)
    y = oa.FIBER(optical_signal.from_device(x), length=2, h=1.0, beta_2=-20.0, gamma=1.0)          # chirp-z: kernels built on the device
    # (the operator D~ of the odd length; once more, in the other precision, when the one-launch engine of the complex64 line gave up and the general path ran)
    uploads = 2 if os.environ.get("SSFM_FUSED_PATIENCE_TICKS") == "-1" else 1
    assert {k: _lib.TRANSFERS[k] - before[k] for k in before} == {"h2d": uploads, "d2h": 0}
    e = oa.electrical_signal.from_device(x)
    before = dict(_lib.TRANSFERS)
    f = oa.LPF(e, BW=5e9)
    assert _lib.TRANSFERS == before and f._raw("signal").dtype == np.float64
    from scipy import signal as sg
    sos = sg.bessel(4, 5e9, "low", fs=gv.fs, norm="mag", output="sos")
    assert within(f.signal, sg.sosfiltfilt(sos, x.to_host().real), 1e-11)
    bits = rng.integers(0, 2, 128).astype(np.uint8)
    before = _lib.TRANSFERS["d2h"]
    v = oa.DAC(bits, pulse_shape="gaussian", c=0.7, coupling="AC")                                 # complex pulse, AC coupled
    assert _lib.TRANSFERS["d2h"] == before and v._raw("signal").dtype == np.complex128
    from oracle import transmitter_numpy as tx
    assert within(v.signal, tx.dac(bits, 16, gv.fs, pulse_shape="gaussian", c=0.7, coupling="AC"), 1e-12)
    one_pol = optical_signal.from_device(_lib.DeviceArray.from_host(rng.standard_normal(2048) + 0j, np.complex128))
    np.random.seed(1)
    before = _lib.TRANSFERS["d2h"]
    amp = oa.EDFA(one_pol, G=10, NF=5)
    assert _lib.TRANSFERS["d2h"] == before
    assert amp.signal.shape == (2, 2048) and not amp.signal[1].any()


# ----------------------------------------------------------------------- multi-rank path on real GPUs (RCCL)
def _run_dist_gpu(tmp_path, world, n_units):
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "_dist_gpu_worker.py"), str(tmp_path), str(n_units)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)          # fresh child processes: they initialise their own GPUs
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]


@pytest.mark.parametrize("world", [1, 2])
def test_propagate_channels_over_rccl_matches_single_process(tmp_path, world):
    """opticomlib_amd.dist.propagate_channels under torch.distributed.run with the nccl (= RCCL) backend: units sharded
    round-robin, results gathered in GPU memory with one collective, equal BIT FOR BIT to the same calls in this
    process.  world = 1 runs the same collectives (all_gather_into_tensor / gather on the zero-copy view of the plan's
    field buffer -- counted by dist.COLLECTIVES) on the single GPU of the test box; world = 2 needs two GPUs (skipped
    otherwise).  Fixed step (batched plan, uneven unit counts), FIBER + DBP to rank 0 only, adaptive
    (one by one), device-resident units."""
    import torch
    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs, {torch.cuda.device_count()} visible")
    sys_path_worker = os.path.join(os.path.dirname(os.path.abspath(__file__)))
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dist_gpu_worker", os.path.join(sys_path_worker, "_dist_gpu_worker.py"))
    w = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(w)
    n_units = 5
    _run_dist_gpu(tmp_path, world, n_units)
    from opticomlib_amd import dist as od
    f = w.fields_for(n_units)
    want_fixed = od.propagate_channels(f, w.DT, **w.FIXED)
    want_dbp = od.propagate_channels(f, w.DT, dbp=True, **w.FIXED)
    want_adapt = od.propagate_channels(f[:3], w.DT, **w.ADAPT)
    assert within(want_fixed[0], orc.fiber_c64(f[0], w.DT, **w.FIXED), kw=w.FIXED, what="oracle")  # and the single-process result is the oracle's
    for rank in range(world):
        got = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        for k in range(n_units):
            np.testing.assert_array_equal(got[f"fixed_{k}"], want_fixed[k])
            np.testing.assert_array_equal(got["fixed_dev"][k], want_fixed[k])
            if rank == 0:
                np.testing.assert_array_equal(got[f"dbp_{k}"], want_dbp[k])
        assert ("dbp_0" in got.files) == (rank == 0)
        for k in range(3):
            np.testing.assert_array_equal(got[f"adapt_{k}"], want_adapt[k])
        # the gathers were real RCCL collectives on device memory -- with ONE rank too (no world-size shortcut)
        assert got["collectives"][0] >= 4 and got["collectives"][1] >= 3, got["collectives"]


def test_host_threads_on_the_same_plans():
    """Several host threads calling FIBER / BPF / PD with the SAME shapes share the cached plans: every device function
    holds its plan's lock for the whole set_field ... get_field sequence, so the results equal the single-threaded ones
    (tools/thread_check.py; ctypes releases the GIL during the calls)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "thread_check.py")], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr[-2000:]


def test_filter_input_shorter_than_the_padding_is_a_value_error():
    gv(sps=16, R=10e9)
    with pytest.raises(ValueError, match="padlen"):                  # SciPy's own exception for the same call
        oa.LPF(np.ones(10), BW=1e9)
    with pytest.raises(ValueError, match="padlen"):
        oa.BPF(optical_signal(np.ones(12, complex)), BW=1e9)


def test_adaptive_capture_goes_to_the_host_in_blocks_and_api_order():
    """return_steps with the adaptive step: the capture is taken through ssfm_adaptive_begin / _run / _finish in blocks
    (64 snapshots at this size), so a run of ~200 steps crosses several block boundaries; snapshots, z and the final
    field equal those of the same run without capture, the memory follows the steps taken (not max_steps), and the three
    entry points refuse to be called out of order."""
    gv(**workloads.BENCH_GV)
    n = 1 << 10
    a = workloads.qpsk_field(n, seed=11, power_w=20e-3)
    kw = dict(length=12, phi_max=0.004, **workloads.SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    steps = len(z) - 1
    assert steps > 100 and A_z.shape == (steps + 1, 2, n) and A_z.dtype == np.complex64
    assert A_z.base is None or A_z.base.nbytes == A_z.nbytes       # a compact array: nothing of max_steps + 1 fields is kept alive
    np.testing.assert_array_equal(A_z[0], a.astype(np.complex64))
    y = oa.FIBER(optical_signal(a), **kw).signal
    # (capture runs the chunked engine step by step, the plain run of a plan this small is one launch: two engines, the bound of the run's step count)
    assert within(A_z[-1], y, steps=steps, what="adaptive capture against the plain adaptive run")
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    assert abs(len(zr) - len(z)) <= 1 and within(A_z[-1], Ar[-1], steps=steps, what=f"oracle adaptive ({steps} vs {len(zr) - 1} steps)")
    k = min(len(z), len(zr)) // 2
    np.testing.assert_allclose(z[:k], zr[:k], rtol=2e-4)
    assert within(A_z[70], Ar[70], steps=70, what="oracle adaptive, snapshot 70 (beyond the first block boundary)")
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        lib = _lib.load()
        import ctypes as C
        st, dn = C.c_int64(0), C.c_int(0)
        assert lib.ssfm_adaptive_run(p._h, 4, None, C.byref(st), C.byref(dn)) == 5                      # SSFM_ERR_STATE: no run begun
        assert lib.ssfm_adaptive_finish(p._h, C.byref(st), None) == 5
        assert lib.ssfm_adaptive_begin(p._h, 1.3, 12.0, 0.004, 0, 1 << 16, 0) == 5                      # no operator yet
        p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13))
        p.set_field(a)
        assert lib.ssfm_adaptive_begin(p._h, 1.3, 12.0, 0.004, 0, 1 << 16, 0) == 0
        blk = _lib.host_empty((4, 2, n), np.complex64)
        assert lib.ssfm_adaptive_run(p._h, 4, blk.ctypes.data_as(C.c_void_p), C.byref(st), C.byref(dn)) == 5   # capture was not announced
        assert lib.ssfm_adaptive_run(p._h, 10, None, C.byref(st), C.byref(dn)) == 0 and st.value == 10 and dn.value == 0
        assert lib.ssfm_adaptive_run(p._h, 1 << 16, None, C.byref(st), C.byref(dn)) == 0 and dn.value == 1 and st.value == steps
        zz = np.zeros(st.value + 1)
        assert lib.ssfm_adaptive_finish(p._h, C.byref(st), zz.ctypes.data_as(C.POINTER(C.c_double))) == 0
        np.testing.assert_array_equal(zz, z)
        np.testing.assert_array_equal(p.get_field(), A_z[-1])   # budgeted runs take the same steps as the step-by-step capture run (both the chunked engine)
        with pytest.raises(oa.SsfmError, match="max_steps=5 reached"):
            p.set_field(a)
            p.propagate_adaptive(1.3, 12.0, 0.004, False, max_steps=5)
    finally:
        p.close()


def test_one_launch_adaptive_run_of_any_length_gives_up_cleanly(monkeypatch):
    """With no patience for the other row's maximum the one-launch adaptive engine of n <= 2048 stores nothing and the run is queued step by step: the
    result is then the general path's, bit for bit.  (The knob is read when a plan is made: the cached plans are released first.  No patience means
    that the first look must find the other row's word: when the two rows' workgroups happen to run in step it does, the engine finishes and the result
    is the complex64 line's -- within the tolerance, not the same bits; the plan tells which happened, and a give-up must be seen within ten tries.)"""
    gv(**workloads.BENCH_GV)
    x = optical_signal(workloads.qpsk_field(1 << 11, seed=5, power_w=8e-3)[:, :200])
    kw = dict(length=8.0, phi_max=0.004, **workloads.SMF)
    monkeypatch.setenv("SSFM_FUSED_PATIENCE_TICKS", "-1")
    gave_up = 0
    for attempt in range(10):
        oa.devices.release_plans()
        monkeypatch.setenv("SSFM_CHIRP_SMALL", "0")
        ref = oa.FIBER(x, **kw).signal
        monkeypatch.setenv("SSFM_CHIRP_SMALL", "1")
        y = oa.FIBER(x, **kw).signal
        info = oa.devices.get_plan(512, 2, _lib.C64, 0).last_run_info()
        if info["fell_back"]:
            gave_up += 1
            np.testing.assert_array_equal(y, ref)
            break
        if info["engine"] != "chirp_small_adaptive":       # the one-launch engine is off in this environment (the knob suite's SSFM_SMALL=0, SSFM_CHIRP_LOOP=python)
            np.testing.assert_array_equal(y, ref)
            return
        assert within(y, ref, TOL_100, what="one-launch adaptive chirp-z engine against the complex128 line")
    assert gave_up == 1


# ----------------------------------------------------------------------- rows of more than 2^22 samples: split plans (round 6, csrc/ssfm_split.hpp)
@pytest.mark.parametrize("log2n,npol,prec", [(21, 1, "c64"), (22, 2, "c64"), (21, 2, "c128")])
def test_split_plans_at_small_size_against_the_direct_engine_and_the_oracle(log2n, npol, prec, monkeypatch):
    """A row of N = R M samples as R sub-sequences of M = 2^20 through the plan's own kernels plus one pointwise launch across them (decimation in time: the
    nonlinear step stays pointwise).  SSFM_SPLIT_ABOVE=20 makes plans of 2^21 / 2^22 samples split (R = 2 / 4), where the direct two-kernel engine and -- at
    2^21 -- the oracle are there to compare with: fixed steps, an adaptive run (five launches per step; launches queued behind the end of the run must leave
    the field alone), every-step snapshots, device-to-device transfers in natural time order, DM; the run info names the engine."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    P, cd, rt = (_lib.C64, np.complex64, np.float32) if prec == "c64" else (_lib.C128, np.complex128, np.float64)
    a = workloads.qpsk_field(n, seed=50 + log2n, n_pol=2, power_w=5e-3)[:npol].astype(cd)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, P)
    hs = np.array([0.25, 0.25, 0.25, 0.125], dtype=rt)
    res = {}
    for name, above in (("split", "20"), ("direct", None)):
        monkeypatch.delenv("SSFM_SPLIT_ABOVE", raising=False)
        if above:
            monkeypatch.setenv("SSFM_SPLIT_ABOVE", above)
        p = _lib.Plan(n, npol, P)
        try:
            p.set_linear_operator(D)
            p.set_field(a)
            np.testing.assert_array_equal(p.get_field(), a)                    # in and out again: natural time order whatever the plan keeps inside
            p.propagate_fixed(1.3, hs)
            fixed = p.get_field()
            eng_fixed = p.last_run_info()["engine"]
            p.propagate_fixed(1.3, hs[:2])                                     # a second run on the resident field (no conversion in between)
            twice = p.get_field()
            p.set_field(a)
            steps, z, _ = p.propagate_adaptive(1.3, 1.0, 0.004, False)
            adapt = p.get_field()
            eng_adapt = p.last_run_info()["engine"]
            p.set_field(a)
            snaps = np.array(p.propagate_fixed(1.3, hs[:2], snapshots=True))
            dev = _lib.DeviceArray((npol, n), cd, 0)
            p.get_field_device(dev.ptr)                                        # device to device, natural order
            p.set_field_device(dev.ptr)
            back = p.get_field()
            dm = None
            if P == _lib.C128:
                p.set_field(a)
                p.apply_dispersion(gv.dt, -150.0e-24)
                dm = p.get_field()
            res[name] = dict(fixed=fixed, twice=twice, adapt=adapt, steps=steps, z=np.asarray(z), snaps=snaps, back=back, dm=dm, engines=(eng_fixed, eng_adapt))
        finally:
            p.close()
    s, d = res["split"], res["direct"]
    assert s["engines"] == ("split", "split_adaptive") and d["engines"][0] == "two_kernel", (s["engines"], d["engines"])
    tol2 = tol_at(4) if P == _lib.C64 else 1e-12
    assert within(s["fixed"], d["fixed"], tol2, steps=4, what="split plan against the direct engine")
    assert within(s["twice"], d["twice"], tol2, steps=6, what="split plan against the direct engine, second run")
    assert s["steps"] == d["steps"] and s["steps"] >= 2
    np.testing.assert_allclose(s["z"], d["z"], rtol=2e-6 if P == _lib.C64 else 1e-12)
    assert within(s["adapt"], d["adapt"], tol2, steps=s["steps"], what="split plan against the direct engine, adaptive")
    assert s["snaps"].shape == (3, npol, n) and np.array_equal(s["snaps"][0], a) and np.array_equal(s["snaps"][2], s["back"])
    assert within(s["snaps"], d["snaps"], tol2, steps=2, what="split plan against the direct engine, every-step snapshots")
    if P == _lib.C128:
        assert within(s["dm"], d["dm"], 1e-13, what="split plan against the direct engine, DM")
        assert within(s["dm"], orc.dm_c128(a, gv.dt, -150.0)[0], 1e-12, what="oracle, DM")
    if log2n == 21:
        x = a[0] if npol == 1 else a
        if P == _lib.C64:
            ref = orc.fiber_c64(x, gv.dt, length=0.875, h=0.25, **workloads.SMF)
            assert within(s["fixed"].reshape(ref.shape), ref, steps=4, what="oracle, 2^21 as a split plan")
        else:
            ref = orc.fiber_c128(x, gv.dt, length=0.875, h=0.25, **workloads.SMF)
            assert within(s["fixed"].reshape(ref.shape), ref, TOL_C128, steps=4, what="float64 restatement, 2^21 as a split plan")


_BIG = {}


def _big_field(log2n, seed, npol, power):
    key = (log2n, seed, npol)
    if key not in _BIG:
        _BIG.clear()                                                           # (one at a time: 2^24 x 2 complex128 is 0.5 GiB of host memory)
        _BIG[key] = workloads.qpsk_field(1 << log2n, seed=seed, n_pol=npol, power_w=power)
    return _BIG[key]


def test_two_to_the_23_against_the_oracle_fixture(golden_dir):
    """2^23 samples, one polarisation (R = 8): FIBER over four fixed steps and DBP of the result (reference semantics: not the identity) against the committed
    strided fixture of the ORACLE's run (tests/golden/make_big_strided.py: every 4099th sample, the power); the chunked `every` capture of a split plan."""
    g = np.load(os.path.join(golden_dir, "big_strided.npz"))
    st = int(g["stride"])
    gv(**workloads.BENCH_GV)
    b = _big_field(23, 2323, 1, 6e-3)[0]
    kw = dict(length=2.0, h=0.5, **workloads.SMF)
    y = oa.FIBER(optical_signal(b), **kw)
    assert y.engine == "split" and y.signal.shape == b.shape and y.signal.dtype == np.complex64
    assert within(y.signal[::st], g["fixed23_samples"], kw=kw, what="oracle fixture, 2^23 x 1, 4 steps")
    np.testing.assert_allclose(np.mean(np.abs(y.signal.astype(np.complex128)) ** 2), float(g["fixed23_power"]), rtol=1e-5)
    x = oa.DBP(y, **kw)
    assert within(x.signal[::st], g["dbp23_samples"], steps=8, what="oracle fixture, 2^23 x 1, FIBER + DBP")
    z, A_z = oa.FIBER(optical_signal(b), return_steps=True, every=3, **kw)
    assert list(z) == [0.0, 1.5, 2.0] and A_z.shape == (3,) + b.shape and np.array_equal(A_z[0], b.astype(np.complex64))
    assert within(A_z[-1], y.signal, tol_at(4), steps=4, what="a split plan's `every` capture (a call per stride) against the plain run")
    with pytest.raises(_lib.SsfmError, match="not for plans of more than"):
        oa.devices.get_plan(1 << 23, 1, _lib.C64, 0).propagate_fixed_capture(1.3, np.full(4, 0.5, np.float32), every=2)
    oa.devices.release_plans()


def test_two_to_the_24_dual_polarisation_against_the_oracle_fixture(golden_dir):
    """The largest field: 2^24 samples x 2 polarisations (R = 16; 256 MiB in complex64).  Four fixed steps and an adaptive run (the reference's default) against the
    ORACLE's strided fixture; then the size-independent properties over 100 steps: the energy follows the float32 attenuation factor (every other operator is
    unitary), the polarisations stay independent (bit for bit the single-polarisation run), and the complex64 run agrees with the complex128 run."""
    g = np.load(os.path.join(golden_dir, "big_strided.npz"))
    st = int(g["stride"])
    gv(**workloads.BENCH_GV)
    a = _big_field(24, 2424, 2, 4e-3)
    kw = dict(length=1.0, h=0.25, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw)
    assert y.engine == "split" and y.signal.shape == a.shape
    assert within(y.signal[:, ::st], g["fixed24_samples"], kw=kw, what="oracle fixture, 2^24 x 2, 4 steps")
    np.testing.assert_allclose(np.mean(np.abs(y.signal.astype(np.complex128)) ** 2, axis=-1), g["fixed24_power"], rtol=1e-5)
    del y
    ya = oa.FIBER(optical_signal(a), length=0.5, phi_max=0.002, **workloads.SMF)
    nz = len(g["adapt24_z"]) - 1
    assert ya.engine == "split_adaptive"
    assert within(ya.signal[:, ::st], g["adapt24_samples"], steps=nz, what=f"oracle fixture, 2^24 x 2, adaptive ({nz} steps)")
    del ya
    kw = dict(length=12.5, h=0.125, **workloads.SMF)                           # 100 of C2's steps
    y = oa.FIBER(optical_signal(a), **kw).signal
    e_in = np.sum(np.abs(a) ** 2, axis=-1)
    e_out = np.sum(np.abs(y.astype(np.complex128)) ** 2, axis=-1)
    att = np.exp(np.complex64(-np.float32(0.2 / 4.343) / 2) * np.float32(0.125)).real
    np.testing.assert_allclose(e_out / e_in, float(att) ** 200, rtol=2e-5)
    y0 = oa.FIBER(optical_signal(a[0]), **kw).signal
    np.testing.assert_array_equal(y0, y[0])
    del y0
    y128 = oa.FIBER(optical_signal(a), precision="complex128", **kw).signal
    # a cross-precision PROPERTY, not the parity bound (that is the fixtures above and test_two_to_the_23_long_run...): the complex128 run rounds no
    # coefficient to float32 and this distance is the complex64 arithmetic's own noise floor against float64, which SURVEY.md 8(c) puts at 5e-6 after 100
    # steps at 2^16 samples and allows x 4 for at 2^20 (= 2e-5); 2^24 samples are four more butterfly layers (x sqrt(24 / 20)) and a maximum over 16 x the
    # samples -- held to 2 x tol(100) = 4e-5 (measured 2.3e-5, profiles/r06_parity_margins.txt)
    assert within(y, y128, 2 * tol_at(100), kw=kw, what="complex64 against complex128, 2^24 x 2, 100 steps (noise floor against float64)")
    del y128
    d = oa.DM(optical_signal(a[0][: 1 << 23]), D=-120.0).signal                # DM of a split plan (complex128) against the oracle's transform
    assert within(d, orc.dm_c128(a[0][: 1 << 23], gv.dt, -120.0)[0], 1e-12, what="oracle, DM of 2^23 samples")
    oa.devices.release_plans()
    _BIG.clear()


def test_two_to_the_23_long_run_against_the_oracle_fixture(golden_dir):
    """Parity of a split plan over a LONG run: 100 of C2's steps (length 12.5 km, h = 0.125 km) on the 2^23-sample field against the ORACLE's run of the same
    (tests/golden/make_big_strided.py long: 5 minutes on one core) -- every 4099th sample within tol(100) = 2e-5, the power."""
    g = np.load(os.path.join(golden_dir, "big_strided_100.npz"))
    st = int(g["stride"])
    gv(**workloads.BENCH_GV)
    b = _big_field(23, 2323, 1, 6e-3)[0]
    kw = dict(length=12.5, h=0.125, **workloads.SMF)
    y = oa.FIBER(optical_signal(b), **kw)
    assert y.engine == "split" and steps_of(kw) == 100
    assert within(y.signal[::st], g["samples"], kw=kw, what="oracle fixture, 2^23 x 1, 100 steps")
    np.testing.assert_allclose(np.mean(np.abs(y.signal.astype(np.complex128)) ** 2), float(g["power"]), rtol=1e-4)
    oa.devices.release_plans()
    _BIG.clear()


def test_full_size_length_that_is_not_a_power_of_two_against_the_oracle_fixture(golden_dir):
    """The reference's PRBS-16 word at 16 samples per bit -- (2^16 - 1) * 16 = 1 048 560 samples per polarisation, dual-pol -- through the chirp-z line that keeps complex64
    values between float64 passes (round 6), against the ORACLE's run of the same (tests/golden/make_anyn_strided.py): 100 of C2's steps, and the adaptive run with its z log."""
    g = np.load(os.path.join(golden_dir, "anyn_strided.npz"))
    st, n = int(g["stride"]), int(g["n"])
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=1616, n_pol=2, power_w=2e-3)
    kw = dict(length=12.5, h=0.125, **workloads.SMF)
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert y.dtype == np.complex64 and y.shape == (2, n) and steps_of(kw) == 100
    assert within(y[:, ::st], g["fixed_samples"], kw=kw, what="oracle fixture, 1048560 x 2, 100 steps")
    np.testing.assert_allclose(np.mean(np.abs(y.astype(np.complex128)) ** 2, axis=-1), g["fixed_power"], rtol=1e-4)
    kwa = dict(length=10.0, phi_max=0.002, **workloads.SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kwa)
    zr = g["adapt_z"]
    assert len(z) == len(zr)
    np.testing.assert_allclose(z, zr, rtol=2e-5)
    steps = len(zr) - 1
    assert within(A_z[-1][:, ::st], g["adapt_samples"], steps=steps, what=f"oracle fixture, 1048560 x 2, adaptive ({steps} steps)")
    np.testing.assert_allclose(np.mean(np.abs(A_z[-1].astype(np.complex128)) ** 2, axis=-1), g["adapt_power"], rtol=1e-4)
    del A_z
    ya = oa.FIBER(optical_signal(a), **kwa).signal                       # (the whole run from C: the same bits as a step at a time)
    assert within(ya[:, ::st], g["adapt_samples"], steps=steps, what="oracle fixture, adaptive, one call")
    oa.devices.release_plans()


# ----------------------------------------------------------------------- adaptive runs with a capture that keeps the run's engine (round 6)
@pytest.mark.parametrize("log2n,npol,prec", [(14, 2, "c64"), (18, 2, "c64"), (20, 2, "c64"), (16, 2, "c128")])
def test_adaptive_capture_keeps_the_engine_and_every_snapshot_is_a_plain_run_stopped_there(log2n, npol, prec):
    """ssfm_adaptive_set_capture (the reference's own consumer of return_steps runs FIBER with h = None, devices.py:2342): the run keeps its
    engine -- two launches per step, fused, where the plan has it -- and a capture step adds one launch.  The z log is the plain run's bit for bit, the end
    field is the plain run's bit for bit, a capture AT the last step is that end field bit for bit (the capture's launch and the run's last launch apply the
    same half rotation to the same data), and every snapshot agrees with the field a plain run leaves when it is stopped after that many steps -- a budgeted run,
    which takes the launch-per-pass engine (END and BEGIN apart where the fused kernel merges their rotations): two engines of this library, half the tolerance."""
    n = 1 << log2n
    gv(**workloads.BENCH_GV)
    P, cd = (_lib.C64, np.complex64) if prec == "c64" else (_lib.C128, np.complex128)
    a = workloads.qpsk_field(n, seed=90 + log2n, n_pol=2, power_w=10e-3)[:npol].astype(cd)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, P)
    p = _lib.Plan(n, npol, P)
    try:
        p.set_linear_operator(D)
        p.set_field(a)
        steps, z, _ = p.propagate_adaptive(1.3, 6.0, 0.004, False)
        plain_end, plain_engine = p.get_field(), p.last_run_info()["engine"]
        assert steps > 30
        every = 7
        p.set_field(a)
        s2, z2, taken, fields = p.propagate_adaptive_capture(1.3, 6.0, 0.004, every=every, capacity=steps // every + 2)
        info = p.last_run_info()
        one_launch = plain_engine in ("medium_adaptive", "small_adaptive")      # (a plan whose plain run is ONE launch: the capture takes the launch-per-pass engine)
        assert s2 == steps
        if one_launch:
            np.testing.assert_allclose(z2, z, rtol=5e-6)
            assert within(p.get_field(), plain_end, steps=steps, what="adaptive capture run (launch per pass) against the plain run (one launch)")
            z, plain_end = z2, p.get_field()
        else:
            assert np.array_equal(z2, z) and info["engine"] == plain_engine, (info, plain_engine)
            np.testing.assert_array_equal(p.get_field(), plain_end)
        assert list(taken) == list(range(every, steps + 1, every)) and fields.shape == (len(taken), npol, n)
        for k in (0, len(taken) // 2, len(taken) - 1):
            s_ = int(taken[k])
            p.set_field(a)
            lib = _lib.load()
            st, dn = _lib._I64(0), _lib._I(0)
            _lib._check(lib.ssfm_adaptive_begin(p._h, 1.3, 6.0, 0.004, 0, 1 << 16, 0), "begin")
            _lib._check(lib.ssfm_adaptive_run(p._h, s_, None, _lib.C.byref(st), _lib.C.byref(dn)), "run")           # a plain run stopped after s_ steps
            zb = np.zeros(st.value + 1)
            _lib._check(lib.ssfm_adaptive_finish(p._h, _lib.C.byref(st), zb.ctypes.data_as(_lib.C.POINTER(_lib._D))), "finish")
            assert st.value == s_
            np.testing.assert_allclose(zb, z[: s_ + 1], rtol=5e-6)               # (the launch-per-pass engine finds the same step sizes to the rounding of a maximum)
            stopped = p.get_field()
            if np.array_equal(fields[k], stopped):
                continue
            assert within(fields[k], stopped, 0.5 * tol_at(s_) if prec == "c64" else 1e-12, steps=s_, what=f"adaptive capture against a plain run stopped at step {s_}")
        # a list of step numbers instead of a stride
        want = np.array([1, 2, steps // 2, steps - 1, steps], dtype=np.int64)
        p.set_field(a)
        s3, z3, taken3, fields3 = p.propagate_adaptive_capture(1.3, 6.0, 0.004, steps=want)
        assert s3 == steps and np.array_equal(z3, z) and list(taken3) == list(want)
        np.testing.assert_array_equal(fields3[-1], plain_end)                                   # the capture at the last step is the end field
        if steps // 2 % every == 0:
            np.testing.assert_array_equal(fields3[2], fields[steps // 2 // every - 1])
    finally:
        p.close()


ADAPT_SEAMS_LENGTH = 20.0        # km: the field and link of the test above, lengthened until the run takes 80 ... 400 steps


def test_adaptive_capture_at_the_seams_of_its_ring():
    """An adaptive run of 2^14 x 2 complex64 samples that captures EVERY step: a chunk's snapshots fill one half of the ring (32 slots: ssfm_capture.hpp
    CapCursor), so a run of more than 64 steps fills a half, the other, and the first again behind the wait for its transfers.  All steps are taken in
    order, the last snapshot is the end field bit for bit, the snapshots at multiples of 7 are those of an every = 7 capture bit for bit (the same engine,
    the same launches), a capacity of 5 stops the capture and not the run, and a list reaches the list's own cut (four snapshots, 64 steps)."""
    n = 1 << 14
    gv(**workloads.BENCH_GV)
    a = workloads.qpsk_field(n, seed=90 + 14, n_pol=2, power_w=10e-3).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, _lib.C64)
    L = ADAPT_SEAMS_LENGTH
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(D)
        p.set_field(a)
        steps, _, _ = p.propagate_adaptive(1.3, L, 0.004, False)
        print(f"adaptive run over {L} km: {steps} steps")
        assert 80 <= steps <= 400 and steps > 2 * 32
        p.set_field(a)
        s1, z1, taken, fields = p.propagate_adaptive_capture(1.3, L, 0.004, every=1, capacity=steps)
        end = p.get_field()
        assert s1 == steps and list(taken) == list(range(1, steps + 1)) and fields.shape == (steps, 2, n)
        np.testing.assert_array_equal(fields[-1], end)
        p.set_field(a)
        s7, z7, taken7, fields7 = p.propagate_adaptive_capture(1.3, L, 0.004, every=7, capacity=steps // 7 + 2)
        assert s7 == steps and np.array_equal(z7, z1) and list(taken7) == list(range(7, steps + 1, 7))
        np.testing.assert_array_equal(fields7, fields[6::7])
        np.testing.assert_array_equal(p.get_field(), end)
        p.set_field(a)
        s5, z5, taken5, fields5 = p.propagate_adaptive_capture(1.3, L, 0.004, every=1, capacity=5)
        assert s5 == steps and np.array_equal(z5, z1) and list(taken5) == [1, 2, 3, 4, 5]
        np.testing.assert_array_equal(p.get_field(), end)
        want = np.array([1, 2, 3, 4, 5, 70, steps], dtype=np.int64)
        p.set_field(a)
        sl, zl, takenl, _ = p.propagate_adaptive_capture(1.3, L, 0.004, steps=want)
        assert sl == steps and np.array_equal(zl, z1) and list(takenl) == list(want)
    finally:
        p.close()


def test_fiber_adaptive_return_steps_with_a_stride_and_with_positions(golden_dir):
    """FIBER(h=None, return_steps=True, every=k / z_list=[...]) through the host mirror: the golden adaptive vector's z log reproduced and sub-sampled, the
    snapshots those of the every-step capture (the reference's return_steps), the positions picked as the first step that reaches each z."""
    case = CASES["kat1_adaptive_2pol"]
    g = np.load(os.path.join(golden_dir, "kat1_adaptive_2pol.npz"))
    x = _signal(case)
    kw = dict(case["kw"])
    z_all, A_all = oa.FIBER(x, return_steps=True, **kw)                       # every step (three launches per step, the host waits per step)
    assert abs(len(z_all) - len(g["z"])) <= 1
    m = min(len(z_all), len(g["z"])) - 1
    np.testing.assert_allclose(z_all[:m], g["z"][:m], rtol=2e-4)
    S = len(z_all) - 1
    z5, A5 = oa.FIBER(x, return_steps=True, every=5, **kw)
    keep = list(range(0, S, 5)) + [S]
    np.testing.assert_array_equal(z5, z_all[keep])
    assert A5.shape == (len(keep),) + A_all.shape[1:] and A5.dtype == np.complex64
    assert within(A5, A_all[keep], 0.5 * tol_at(S), steps=S, what="adaptive strided capture against the every-step capture")
    assert within(A5[-1], g["out"], steps=S, what="golden out, adaptive strided capture")
    zl = [0.0, 0.3, float(z_all[7]), 5.0, 9.999, 10.0, 12.0]
    zp, Ap = oa.FIBER(x, return_steps=True, z_list=zl, **kw)
    idx = [int(min(np.searchsorted(z_all, v, side="left"), S)) for v in zl]
    assert idx[0] == 0 and idx[2] == 7 and idx[-1] == S and idx[-2] == S
    np.testing.assert_array_equal(zp, z_all[idx])
    assert within(Ap, A_all[idx], 0.5 * tol_at(S), steps=S, what="adaptive capture at given z against the every-step capture")


def test_a_rated_pair_of_lane_streams_outlives_its_plan(monkeypatch):
    """Round 6: rating a fresh pair of lane streams costs ~7 ms of probe launches per two-lane plan, and what it finds out is a property
    of the streams.  A two-lane plan that ends with good lanes hands its pair to the process's pool; the next two-lane plan on the device takes it with its
    rating: no rating at its creation (the process-wide count stands still), the same step time, the same bits -- and lane_health still watches its runs."""
    import time
    for k in ("SSFM_LANES", "SSFM_LANE_POOL_OFF", "SSFM_E", "SSFM_EF"):
        monkeypatch.delenv(k, raising=False)
    oa.devices.release_plans()
    gv(**workloads.BENCH_GV)
    n = 1 << 20
    a = workloads.qpsk_field(n, seed=4).astype(np.complex64)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    hs = np.full(200, 0.125, np.float32)
    outs, infos, created = [], [], []
    for k in range(4):
        t0 = time.perf_counter()
        p = _lib.Plan(n, 2, _lib.C64)
        created.append(time.perf_counter() - t0)
        try:
            assert p.lanes == 2
            p.set_linear_operator(D); p.set_field(a)
            p.propagate_fixed(1.3, hs); p.synchronize()
            t = None
            for rep in range(3):              # (the best of three: a box that is still waking up is slow once)
                t0 = time.perf_counter(); p.propagate_fixed(1.3, hs); p.synchronize(); el = time.perf_counter() - t0
                t = el if t is None else min(t, el)
            p.set_field(a); p.propagate_fixed(1.3, hs)
            outs.append(p.get_field())
            info = p.last_run_info()
            info["step_us"] = t / hs.size * 1e6
            infos.append(info)
        finally:
            p.close()
    assert [i["lanes_from_pool"] for i in infos[1:]] == [True, True, True], infos
    assert infos[3]["lane_ratings_total"] == infos[0]["lane_ratings_total"], infos               # no plan after the first rated anything
    assert infos[3]["lane_pairs_reused"] >= infos[0]["lane_pairs_reused"] + 3
    assert all(i["lanes"] == 2 and not i["lanes_dropped"] and i["lane_last_us"] > 0 for i in infos), infos
    assert max(i["step_us"] for i in infos) < 1.35 * min(i["step_us"] for i in infos), infos
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])
    print(f"plan creation: {created[0] * 1e3:.1f} ms with a rating, {min(created[1:]) * 1e3:.1f} ms with a pooled pair")


def test_scalar_log_of_a_capture_against_the_oracle():
    """The per-step scalars of ssfm_propagate_fixed_capture (mean and maximum of |A|^2 of every row after every step, accumulated inside the column kernels) against the
    ORACLE's every-step fields -- round 5 checked the log against the library's own snapshots only."""
    gv(**workloads.BENCH_GV)
    n = 1 << 14
    a = workloads.qpsk_field(n, seed=33, n_pol=2, power_w=4e-3)
    kw = dict(length=23 * 0.25, h=0.25, **workloads.SMF)
    zr, Ar = orc.fiber_c64(a, gv.dt, return_steps=True, **kw)
    want_power = np.mean(np.abs(Ar.astype(np.complex128)) ** 2, axis=-1)          # (steps + 1, 2)
    want_peak = np.max(np.abs(Ar.astype(np.complex128)) ** 2, axis=-1)
    p = _lib.Plan(n, 2, _lib.C64)
    try:
        p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13))
        p.set_field(a.astype(np.complex64))
        cap = p.propagate_fixed_capture(1.3, np.full(23, 0.25, np.float32), every=23, scalars=True)
    finally:
        p.close()
    assert cap["power"].shape == want_power.shape == (24, 2)
    np.testing.assert_allclose(cap["power"], want_power, rtol=2e-5)                # (the log sums |A|^2 in float32; the fields themselves agree to 2e-5 of the peak)
    np.testing.assert_allclose(cap["peak"], want_peak, rtol=1e-4)
    assert within(cap["fields"][-1], Ar[-1], kw=kw, what="oracle, the capture run's end field")


def test_split_plans_with_odd_row_counts_and_through_the_sharded_entry_point(monkeypatch):
    """Split plans whose rows do not pair into two lanes (three rows: one lane), a single row, and the batched plan behind dist.propagate_channels (four rows of two
    independent fields) -- each row against the same row propagated alone on the direct engine (SSFM_SPLIT_ABOVE=20: 2^21 samples as two sub-sequences)."""
    from opticomlib_amd import dist as od
    gv(**workloads.BENCH_GV)
    n = 1 << 21
    f = np.stack([workloads.qpsk_field(n, seed=70 + k, n_pol=2, power_w=3e-3) for k in range(2)]).astype(np.complex64)      # (2 fields, 2 pols, n)
    rows = f.reshape(4, n)
    hs = np.full(3, 0.25, np.float32)
    D = oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13)
    monkeypatch.delenv("SSFM_SPLIT_ABOVE", raising=False)
    want = []
    for r in rows[:3]:
        p = _lib.Plan(n, 1, _lib.C64)
        try:
            p.set_linear_operator(D); p.set_field(r.reshape(1, n)); p.propagate_fixed(1.3, hs)
            want.append(p.get_field()[0])
            assert p.last_run_info()["engine"] == "two_kernel"
        finally:
            p.close()
    monkeypatch.setenv("SSFM_SPLIT_ABOVE", "20")
    oa.devices.release_plans()
    for batch in (3, 1):
        p = _lib.Plan(n, batch, _lib.C64)
        try:
            p.set_linear_operator(D); p.set_field(rows[:batch]); p.propagate_fixed(1.3, hs)
            got = p.get_field()
            info = p.last_run_info()
            assert info["engine"] == "split" and info["lanes"] == 1, info
        finally:
            p.close()
        for k in range(batch):
            assert within(got[k], want[k], tol_at(3), steps=3, what=f"split plan of {batch} row(s), row {k}, against the direct engine")
    outs = od.propagate_channels(f, gv.dt, length=0.75, h=0.25, **workloads.SMF)
    assert within(outs[0], np.stack(want[:2]), tol_at(3), steps=3, what="split plans behind dist.propagate_channels against the direct engine")
    back = od.propagate_channels(f[:1], gv.dt, dbp=True, length=0.75, h=0.25, **workloads.SMF)                               # FIBER + DBP on a resident split plan
    ref = orc.dbp_c64(orc.fiber_c64(f[0], gv.dt, length=0.75, h=0.25, **workloads.SMF), gv.dt, length=0.75, h=0.25, **workloads.SMF)
    assert within(back[0], ref, steps=6, what="oracle FIBER + DBP, 2^21 x 2 as split plans")
    oa.devices.release_plans()
