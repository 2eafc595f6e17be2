"""``FIBER(coupling="manakov")`` without a GPU: the yardstick itself (tests/manakov_numpy.py) against the scalar oracle and against the one property the
scalar model does not have -- invariance under a fixed polarisation rotation --, that every parameter row of the GPU test tells the two models apart,
the validation (raised before any device call) and the ABI; and for every row of tests/test_manakov_edges_gpu.py what makes it worth a GPU run: the
``hs=`` / ``max_steps=`` loops of the yardstick are its ``h=`` loop, the high-power rows are well conditioned and reach the phase range they are there
for, and the snapshot and schedule rows would see the mistakes they look for."""
import os

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, dist, workloads
from opticomlib_amd.accuracy import TOL_C128, tol as accuracy_tol
from opticomlib_amd.typing import gv, optical_signal
from oracle import ssfm_numpy as orc

import manakov_numpy as mk
from margins import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _field(k, power_w=10e-3):
    gv(**workloads.BENCH_GV)
    return workloads.qpsk_field(1 << k, seed=100 + k, power_w=power_w)


@pytest.mark.parametrize("h", [0.5, None])
def test_restatement_is_the_scalar_oracle_for_one_polarisation(h):
    """A[1] = 0, kappa = 1: the coupled power is |A[0]|^2 and row 0 is the scalar fibre (0 in complex64, 4e-15 in complex128)."""
    a = _field(10)
    a[1] = 0
    kw = dict(length=10, h=h, phi_max=0.05, **workloads.SMF)
    y, z = mk.manakov_c64(a, gv.dt, kappa=1.0, return_z=True, **kw)
    zr, Ar = orc.fiber_c64(a[0], gv.dt, return_steps=True, **kw)
    assert y.dtype == np.complex64 and np.array_equal(z, zr)
    assert relmax(y[0], Ar[-1]) < TOL_C128 and not y[1].any()
    y = mk.manakov_c128(a, gv.dt, kappa=1.0, **kw)
    assert relmax(y[0], orc.fiber_c128(a[0], gv.dt, **kw)) < TOL_C128 and not y[1].any()


@pytest.mark.parametrize("k, length, h", [(10, 20, 0.5), (8, 100, 0.1), (10, 20, None)])
def test_restatement_commutes_with_a_polarisation_rotation(k, length, h):
    """manakov(U A) = U manakov(A) for a fixed unitary U (<= 2e-14 up to 1000 steps); the per-polarisation model breaks it by more than 1e-2."""
    a = _field(k)
    U = mk.unitary(0.7, 0.4)
    kw = dict(length=length, h=h, phi_max=0.05, **workloads.SMF)
    assert relmax(mk.manakov_c128(U @ a, gv.dt, **kw), U @ mk.manakov_c128(a, gv.dt, **kw)) < TOL_C128
    assert relmax(orc.fiber_c128(U @ a, gv.dt, **kw), U @ orc.fiber_c128(a, gv.dt, **kw)) > 1e-2


@pytest.mark.parametrize("k, steps", mk.FIXED_ROWS)
def test_fixed_rows_of_the_gpu_test_tell_the_models_apart(k, steps):
    a = _field(k)
    kw = dict(length=steps * 0.5, h=0.5, **workloads.SMF)
    assert len(oa.devices.step_schedule(kw["length"], 0.5)[0]) == steps
    assert relmax(mk.manakov_c64(a, gv.dt, **kw), orc.fiber_c64(a, gv.dt, **kw)) > 1e-2


@pytest.mark.parametrize("k, length, phi_max", mk.ADAPTIVE_ROWS)
def test_adaptive_rows_of_the_gpu_test_tell_the_models_apart(k, length, phi_max):
    a = _field(k)
    kw = dict(length=length, phi_max=phi_max, **workloads.SMF)
    assert relmax(mk.manakov_c64(a, gv.dt, **kw), orc.fiber_c64(a, gv.dt, **kw)) > 1e-2


# ---- the rows of tests/test_manakov_edges_gpu.py: what makes each of them worth a GPU run
NEG_SMF = {name: -v for name, v in workloads.SMF.items()}


def _per_polarisation_c64(a, **kw):
    """The reference's model on a schedule ``hs=`` that ``orc.fiber_c64`` does not take: each row alone with ``kappa = 1`` is its scalar fibre (above)."""
    x, y = np.array(a), np.array(a)
    x[1], y[0] = 0, 0
    return np.stack([mk.manakov_c64(x, gv.dt, kappa=1.0, **kw)[0], mk.manakov_c64(y, gv.dt, kappa=1.0, **kw)[1]])


@pytest.mark.parametrize("k", [mk.CLAMPED_ROW[0], mk.SCHEDULE_ROW[0]])
def test_an_explicit_schedule_is_the_fixed_step_run(k):
    """``hs=`` with the schedule of ``h = 0.5`` over 10.3 km -- 20 steps and a clamped one of 0.3 km -- is the ``h=`` run bit for bit, field and z, in
    both precisions: the two new arguments' loop is the old one."""
    _, length, h, steps = mk.CLAMPED_ROW
    a = _field(k)
    for fn, prec in ((mk.manakov_c64, _lib.C64), (mk.manakov_c128, _lib.C128)):
        hs, z = oa.devices.step_schedule(length, h, prec)
        assert len(hs) == steps and abs(float(hs[-1]) - 0.3) < 1e-6 and np.all(hs[:-1] == 0.5)
        zs, As = fn(a, gv.dt, hs=hs, return_steps=True, **workloads.SMF)
        zh, Ah = fn(a, gv.dt, length=length, h=h, return_steps=True, **workloads.SMF)
        assert np.array_equal(zs, zh) and np.array_equal(zs, np.asarray(z, dtype=np.float64)) and np.array_equal(As, Ah)
        y, zy = fn(a, gv.dt, hs=hs, return_z=True, **workloads.SMF)
        assert np.array_equal(y, As[-1]) and np.array_equal(zy, zs)


def test_clamped_schedule_and_backward_rows_tell_the_models_apart():
    k, length, h, _ = mk.CLAMPED_ROW
    kw = dict(length=length, h=h, **workloads.SMF)
    assert relmax(mk.manakov_c64(_field(k), gv.dt, **kw), orc.fiber_c64(_field(k), gv.dt, **kw)) > 1e-2
    k, hs = mk.SCHEDULE_ROW
    a = _field(k)
    assert len(set(hs)) > 2                                   # (more sizes than the line has table slots)
    assert relmax(_per_polarisation_c64(a, length=3, h=0.5, **workloads.SMF), orc.fiber_c64(a, gv.dt, length=3, h=0.5, **workloads.SMF)) == 0
    assert relmax(mk.manakov_c64(a, gv.dt, hs=hs, **workloads.SMF), _per_polarisation_c64(a, hs=hs, **workloads.SMF)) > 1e-2
    k, length, phi_max, h, steps = mk.BACKWARD_ROW
    a = _field(k)
    for hh in (None, h):
        kw = dict(length=length, h=hh, phi_max=phi_max, **NEG_SMF)
        y, z = mk.manakov_c64(a, gv.dt, return_z=True, **kw)
        assert relmax(y, orc.fiber_c64(a, gv.dt, **kw)) > 1e-2
        if hh is None:                                         # (12 steps; complex64 and complex128 1.3e-6 apart)
            y128, z128 = mk.manakov_c128(a, gv.dt, return_z=True, **kw)
            assert len(z) - 1 == len(z128) - 1 == steps and relmax(y, y128) < accuracy_tol(steps) / 2


def test_snapshot_and_schedule_rows_see_what_they_are_there_for():
    """What the GPU rows would measure if the line were wrong in the way they look for, on the restatement: a snapshot taken behind the NEXT step's
    opening half rotation as well is 1e-2 from the step's own field, and one step of the schedule taken at the size the other slot holds (0.25 km
    for 0.5 km) moves the end field by 3e-2 -- both beyond 100 tol."""
    k, length, h, steps = mk.CLAMPED_ROW
    z, A_z = mk.manakov_c128(_field(k), gv.dt, length=length, h=h, return_steps=True, **workloads.SMF)
    g = workloads.SMF["gamma"] * mk.KAPPA
    for i in (1, steps - 1):
        opened = A_z[i] * np.exp(1j * (h / 2) * g * (np.abs(A_z[i]) ** 2).sum(axis=0))
        assert relmax(opened, A_z[i]) > 100 * accuracy_tol(steps)
    k, hs = mk.SCHEDULE_ROW
    stale = list(hs)
    assert stale[5] == 0.5 and stale[4] == 0.25
    stale[5] = 0.25
    a = _field(k)
    assert relmax(mk.manakov_c128(a, gv.dt, hs=stale, **workloads.SMF), mk.manakov_c128(a, gv.dt, hs=hs, **workloads.SMF)) > 100 * accuracy_tol(len(hs))


@pytest.mark.parametrize("k, length, phi_max", mk.SNAPSHOT_ADAPTIVE_ROWS)
def test_adaptive_snapshot_rows_tell_the_models_apart(k, length, phi_max):
    a = _field(k)
    kw = dict(length=length, phi_max=phi_max, **workloads.SMF)
    assert relmax(mk.manakov_c64(a, gv.dt, **kw), orc.fiber_c64(a, gv.dt, **kw)) > 1e-2


@pytest.mark.parametrize("k", sorted(set(mk.SIZE_ROWS["complex64"]) - {19, 20, 21, 22}))
def test_size_rows_tell_the_models_apart(k):
    """Two steps of 0.5 km: 1.8e-2 at every size (the rows above 2^16 are the same field statistics; their restatement takes seconds)."""
    a = _field(k)
    kw = dict(length=1, h=0.5, **workloads.SMF)
    assert len(oa.devices.step_schedule(1, 0.5)[0]) == 2
    assert relmax(mk.manakov_c64(a, gv.dt, **kw), orc.fiber_c64(a, gv.dt, **kw)) > 100 * accuracy_tol(2)


@pytest.mark.parametrize("k, power_w, steps, precisions", mk.PHASE_ROWS)
def test_phase_rows_are_well_conditioned(k, power_w, steps, precisions):
    """The rows that reach the larger-phase branches of ``rotate_all``: the phase per pass is where the row wants it, the restatement's own complex64
    result is within half the bound of its complex128 result where the row runs in complex64 (1.3e-6 at 0.3 W, 9.3e-6 at 3 W; 6e-5 ... 1.3e-4 at
    30 W, which is why that row is complex128 only), and a 1e-15 relative perturbation of the input moves the complex128 result by less than
    TOL_C128 / 10 (2.3e-12 at 30 W)."""
    a = _field(k, power_w)
    kw = dict(length=steps * 0.5, h=0.5, **workloads.SMF)
    phase = 0.5 * workloads.SMF["gamma"] * mk.KAPPA * (np.abs(a) ** 2).sum(axis=0).max()
    lo, hi = {0.3: (2.0 ** -5, 0.78), 3.0: (0.78, 65000.0), 30.0: (0.78 * 10, 65000.0)}[power_w]
    assert lo < phase <= hi
    y128 = mk.manakov_c128(a, gv.dt, **kw)
    if "complex64" in precisions:
        assert relmax(mk.manakov_c64(a, gv.dt, **kw), y128) < accuracy_tol(steps) / 2
    else:
        assert relmax(mk.manakov_c64(a, gv.dt, **kw), y128) > accuracy_tol(steps)           # (no complex64 row: it would compare two roundings)
    nudged = a * (1 + 1e-15 * np.random.default_rng(7).standard_normal(a.shape))
    assert relmax(mk.manakov_c128(nudged, gv.dt, **kw), y128) < TOL_C128 / 10


def test_unit_row_reaches_the_double_reduction():
    """One step of 0.5 km at 2e5 W: the opening half rotation alone turns most samples by more than 65000 rad in float32, and the same call with
    ``gamma_alone`` turns none by more than 2^-5 (the table transform alone)."""
    u = mk.UNIT_ROW
    P = (np.abs(_field(u["k"], u["power_w"]).astype(np.complex64)) ** 2).sum(axis=0)
    assert P.dtype == np.float32
    half = np.float32(0.5) * np.float32(u["h"])
    g = np.float32(u["gamma"]) * np.float32(mk.KAPPA)
    assert np.mean(half * (g * P) > 65000.0) > 0.5
    g = np.float32(u["gamma_alone"]) * np.float32(mk.KAPPA)
    assert g > 0 and (np.float32(u["h"]) * (g * P)).max() < 2.0 ** -5


def test_max_steps_stops_the_restatement():
    k, length, phi_max, max_steps, full = mk.BUDGET_ROW
    a = _field(k)
    kw = dict(length=length, phi_max=phi_max, **workloads.SMF)
    for fn in (mk.manakov_c64, mk.manakov_c128):
        z, A = fn(a, gv.dt, return_steps=True, **kw)
        zb, Ab = fn(a, gv.dt, return_steps=True, max_steps=max_steps, **kw)
        assert len(z) - 1 == full and len(zb) - 1 == max_steps and zb[-1] < length
        assert np.array_equal(zb, z[: max_steps + 1]) and np.array_equal(Ab, A[: max_steps + 1])
        y, zy = fn(a, gv.dt, return_z=True, max_steps=max_steps, **kw)
        assert np.array_equal(y, A[max_steps]) and np.array_equal(zy, zb)
        assert np.array_equal(fn(a, gv.dt, return_steps=True, max_steps=full + 5, **kw)[1], A)


@pytest.mark.parametrize("k, steps", mk.DARK_ROWS)
def test_dark_rows_are_the_scalar_oracle(k, steps):
    a = _field(k)
    a[1] = 0
    for h in (0.5, None):
        kw = dict(length=steps * 0.5, h=h, phi_max=0.05, **workloads.SMF)
        y = mk.manakov_c64(a, gv.dt, kappa=1.0, **kw)
        assert relmax(y[0], orc.fiber_c64(a[0], gv.dt, **kw)) < TOL_C128 and not y[1].any()
        # (and the row is no linear run: without the nonlinearity row 0 ends somewhere else)
        assert relmax(y[0], orc.fiber_c64(a[0], gv.dt, **dict(kw, gamma=0.0, h=0.5))) > 1e-2


def test_validation_needs_no_device():
    gv(**workloads.BENCH_GV)
    two = optical_signal(np.ones((2, 4096), complex))
    kw = dict(length=1, h=0.5, gamma=1.3)
    for fn in (oa.FIBER, oa.DBP):
        with pytest.raises(ValueError, match="coupling must be None"):
            fn(two, coupling="xpm", **kw)
        with pytest.raises(ValueError, match="not supported for a field of shape"):
            fn(optical_signal(np.ones(4096, complex)), coupling="manakov", **kw)
        for n in (4000, 128) + ((1 << 23,) if fn is oa.FIBER else ()):
            with pytest.raises(ValueError, match=f"not supported for {n} samples"):
                fn(optical_signal(np.ones((2, n), np.complex64)), coupling="manakov", **kw)
        for kappa in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="not supported for kappa"):
                fn(two, coupling="manakov", kappa=kappa, **kw)
        with pytest.raises(ValueError, match="kappa belongs to"):
            fn(two, kappa=1.0, **kw)
    with pytest.raises(ValueError, match="does not support coupling"):
        dist.propagate_channels(np.ones((1, 2, 4096), complex), gv.dt, coupling="manakov", **kw)
    assert oa.devices.MANAKOV_KAPPA == 8.0 / 9.0


def test_the_entry_point_is_declared_bound_and_exported():
    import re
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    assert "SSFM_API int ssfm_manakov_propagate(" in hdr and "ssfm_manakov_propagate" in _lib.SYMBOLS
    assert re.search(r"#define SSFM_ABI_VERSION 3\b", hdr)
    lib = _lib.load()
    assert lib.ssfm_manakov_propagate.argtypes == _lib.SYMBOLS["ssfm_manakov_propagate"][1]
    names = set(subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split())
    assert "ssfm_manakov_propagate" in names
    m = re.search(r"SSFM_ENGINE_MANAKOV_LINE = (\d+)", hdr)
    assert m and _lib.ENGINES[int(m.group(1))] == "manakov_line"
    assert "manakov.hip" in open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()
