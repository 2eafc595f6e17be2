"""``FIBER(coupling="manakov", pmd=...)`` without a GPU: the yardstick itself (tests/manakov_pmd_numpy.py) -- its unitaries, its sign and size of the
differential delay, that it is the plain Manakov restatement without PMD, that its sections add up to the DGD statistics of the waveplate model --,
that every row of tests/test_manakov_pmd_gpu.py is well conditioned and tells the PMD line from the plain one, the argument refusals (raised before
any device call) and the ABI."""
import os

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, devices, workloads
from opticomlib_amd.accuracy import tol
from opticomlib_amd.typing import gv, optical_signal

import manakov_numpy as mk
import manakov_pmd_numpy as pk
from margins import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMF = workloads.SMF


def _field(k, power_w=10e-3):
    gv(**workloads.BENCH_GV)
    return workloads.qpsk_field(1 << k, seed=100 + k, power_w=power_w)


def test_sections_are_special_unitary_and_repeat():
    U = devices.pmd_sections(7, 1000)
    assert U.shape == (1000, 2, 2) and U.dtype == np.complex128
    assert np.max(np.abs(U @ np.conj(np.swapaxes(U, 1, 2)) - np.eye(2))) < 1e-15
    assert np.max(np.abs(np.linalg.det(U) - 1)) < 1e-15
    assert np.array_equal(U, devices.pmd_sections(7, 1000))
    assert np.array_equal(U, pk.sections(7, 1000))                                   # (the yardstick's own copy of the recipe)
    assert np.array_equal(U[:40], devices.pmd_sections(7, 40))                       # (a longer draw starts with the shorter one: adaptive reruns)
    assert np.max(np.abs(U[:40] - devices.pmd_sections(8, 40))) > 0.1
    assert np.array_equal(U[:, 1, 0], -np.conj(U[:, 0, 1])) and np.array_equal(U[:, 1, 1], np.conj(U[:, 0, 0]))


def test_a_pure_delay_moves_row_0_back_and_row_1_forward():
    """dt = 1.953125 ps: tau = 11.71875 sqrt(1) = 6 dt, so row 0 is three samples late and row 1 three samples early."""
    a = _field(8)
    assert abs(gv.dt * 1e12 - 1.953125) < 1e-12
    y = pk.pmd_c128(a, gv.dt, length=1, h=1.0, pmd=11.71875, pmd_scatter=False)
    assert np.max(np.abs(y[0] - np.roll(a[0], 3))) < 1e-13 and np.max(np.abs(y[1] - np.roll(a[1], -3))) < 1e-13
    y = pk.pmd_c64(a, gv.dt, length=1, h=1.0, pmd=11.71875, pmd_scatter=False)
    assert y.dtype == np.complex64 and relmax(y[0], np.roll(a[0], 3)) < tol(1) and relmax(y[1], np.roll(a[1], -3)) < tol(1)


@pytest.mark.parametrize("run", [dict(length=10.3, h=0.5), dict(length=10, phi_max=0.05), dict(hs=mk.SCHEDULE_ROW[1]), dict(length=10, phi_max=0.05, max_steps=4),
                                 dict(length=3, gamma=0.0)])
def test_without_pmd_it_is_the_plain_restatement(run):
    a = _field(10)
    kw = {**SMF, **run}
    for plain, with_pmd in ((mk.manakov_c128, pk.pmd_c128), (mk.manakov_c64, pk.pmd_c64)):
        z, A_z = plain(a, gv.dt, return_steps=True, **kw)
        zp, Ap = with_pmd(a, gv.dt, return_steps=True, pmd=0.0, pmd_scatter=False, **kw)
        assert np.array_equal(z, zp) and np.array_equal(A_z, Ap) and Ap.dtype == A_z.dtype
        y, zy = with_pmd(a, gv.dt, return_z=True, pmd=0.0, pmd_scatter=False, **kw)
        assert np.array_equal(y, A_z[-1]) and np.array_equal(zy, z)


def test_dgd_statistics_of_equal_sections():
    """40 sections of 0.5 km at D_p = 0.1: the rms DGD over 64 seeds and 41 frequencies is D_p sqrt(L) within 10 % (the waveplate model's
    Maxwellian; 1.026 of it here)."""
    dp, hs = 0.1, [0.5] * 40
    ws = np.linspace(-0.3, 0.3, 41)
    dgd = np.array([[pk.jones_dgd(dp, hs, Us, w0) for w0 in ws] for Us in (pk.sections(seed, len(hs)) for seed in range(64))])
    ratio = np.sqrt(np.mean(dgd ** 2)) / (dp * np.sqrt(sum(hs)))
    assert 0.9 < ratio < 1.1, ratio
    # (and the restatement's line IS that Jones matrix: without dispersion, loss and nonlinearity a tone comes out as T(w) applied to it)
    gv(**workloads.BENCH_GV)
    n, m = 256, 5
    w0 = 2 * np.pi * m / (n * gv.dt) * 1e-12
    tone = np.exp(2j * np.pi * m * np.arange(n) / n)
    a = np.stack([0.6 * tone, 0.8j * tone])
    y = pk.pmd_c128(a, gv.dt, hs=hs, pmd=dp, pmd_seed=3)
    T = np.eye(2, dtype=complex)
    for h_, U in zip(hs, pk.sections(3, len(hs))):
        T = np.diag([np.exp(-0.5j * w0 * dp * np.sqrt(h_)), np.exp(0.5j * w0 * dp * np.sqrt(h_))]) @ U @ T
    assert np.max(np.abs(y - T @ a)) < 1e-12


ROWS = [(8, 40), (12, 40), (14, 25)]


@pytest.mark.parametrize("scatter", [True, False])
@pytest.mark.parametrize("k, steps", ROWS)
def test_gpu_rows_are_well_conditioned_and_see_the_pmd(k, steps, scatter):
    """complex64 and complex128 restatements lie within half the GPU bound of each other (2.6e-6, 3.2e-6, 2.5e-6 against 1e-5 and more), and PMD at
    D_p = 1 moves the field by more than 0.1 of the peak (1.5-1.9; 0.5-1.1 without scattering)."""
    a = _field(k)
    kw = dict(length=steps * 0.5, h=0.5, **SMF)
    y128 = pk.pmd_c128(a, gv.dt, pmd=1.0, pmd_seed=5, pmd_scatter=scatter, **kw)
    y64 = pk.pmd_c64(a, gv.dt, pmd=1.0, pmd_seed=5, pmd_scatter=scatter, **kw)
    assert y64.dtype == np.complex64
    assert relmax(y64, y128) < 0.5 * tol(steps)
    assert relmax(y128, mk.manakov_c128(a, gv.dt, **kw)) > 0.1


def test_adaptive_restatement_takes_the_plain_steps():
    """A unitary leaves P as it is and a delay moves it: the step sizes follow the field, the count stays the plain run's within a step."""
    k, length, phi_max = mk.ADAPTIVE_ROWS[2]
    a = _field(k)
    kw = dict(length=length, phi_max=phi_max, **SMF)
    _, z = mk.manakov_c128(a, gv.dt, return_z=True, **kw)
    y, zp = pk.pmd_c128(a, gv.dt, return_z=True, pmd=1.0, pmd_seed=5, **kw)
    assert abs(len(z) - len(zp)) <= 1 and zp[-1] == length
    y64, z64 = pk.pmd_c64(a, gv.dt, return_z=True, pmd=1.0, pmd_seed=5, **kw)
    assert abs(len(z64) - len(zp)) <= 1 and z64[-1] == length
    # (a budget stops the loop where the full run's steps are)
    yb, zb = pk.pmd_c128(a, gv.dt, return_z=True, pmd=1.0, pmd_seed=5, max_steps=4, **kw)
    assert len(zb) == 5 and np.array_equal(zb, zp[:5])


def test_argument_refusals_need_no_device():
    gv(**workloads.BENCH_GV)
    two = optical_signal(np.ones((2, 4096), complex))
    kw = dict(length=1, h=0.5, gamma=1.3)
    with pytest.raises(ValueError, match="pmd needs coupling='manakov'"):
        oa.FIBER(two, pmd=0.1, **kw)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "a lot"):
        with pytest.raises(ValueError, match="pmd must be a finite coefficient >= 0"):
            oa.FIBER(two, coupling="manakov", pmd=bad, **kw)
    for extra in (dict(pmd_seed=3), dict(pmd_scatter=False), dict(pmd_seed=3, pmd_scatter=False)):
        with pytest.raises(ValueError, match="pmd_seed and pmd_scatter belong to pmd="):
            oa.FIBER(two, coupling="manakov", **extra, **kw)
        with pytest.raises(ValueError, match="pmd_seed and pmd_scatter belong to pmd="):
            oa.FIBER(two, **extra, **kw)
        with pytest.raises(ValueError, match="DBP takes no pmd"):
            oa.DBP(two, coupling="manakov", **extra, **kw)
    for pmd in (0.0, 0.1):
        with pytest.raises(ValueError, match="DBP takes no pmd"):
            oa.DBP(two, coupling="manakov", pmd=pmd, **kw)
        with pytest.raises(ValueError, match="DBP takes no pmd"):
            oa.DBP(two, pmd=pmd, **kw)
    # (the shape checks of coupling="manakov" come first as ever)
    with pytest.raises(ValueError, match="not supported for a field of shape"):
        oa.FIBER(optical_signal(np.ones(4096, complex)), coupling="manakov", pmd=0.1, **kw)


def test_the_entry_point_is_declared_bound_and_exported():
    import re
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    assert "SSFM_API int ssfm_manakov_pmd_propagate(" in hdr and "ssfm_manakov_pmd_propagate" in _lib.SYMBOLS
    assert re.search(r"#define SSFM_ABI_VERSION 3\b", hdr)
    lib = _lib.load()
    assert lib.ssfm_manakov_pmd_propagate.argtypes == _lib.SYMBOLS["ssfm_manakov_pmd_propagate"][1]
    # (the plain entry point's arguments, then dp, the quaternions with their count, and w)
    assert _lib.SYMBOLS["ssfm_manakov_pmd_propagate"][1][:13] == _lib.SYMBOLS["ssfm_manakov_propagate"][1]
    assert len(_lib.SYMBOLS["ssfm_manakov_pmd_propagate"][1]) == 17
    names = set(subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split())
    assert "ssfm_manakov_pmd_propagate" in names
    m = re.search(r"SSFM_ENGINE_MANAKOV_PMD_LINE = (\d+)", hdr)
    assert m and int(m.group(1)) == len(_lib.ENGINES) - 1 and _lib.ENGINES[int(m.group(1))] == "manakov_pmd_line"
    assert hasattr(_lib.Plan, "manakov_pmd_propagate") and callable(devices.pmd_sections)
