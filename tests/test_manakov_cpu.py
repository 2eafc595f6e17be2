"""``FIBER(coupling="manakov")`` without a GPU: the yardstick itself (tests/manakov_numpy.py) against the scalar oracle and against the one property the
scalar model does not have -- invariance under a fixed polarisation rotation --, that every parameter row of the GPU test tells the two models apart,
the validation (raised before any device call) and the ABI."""
import os

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, dist, workloads
from opticomlib_amd.accuracy import TOL_C128
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
