"""``FIBER / DBP(coupling="manakov")`` on the GPU (``-m gpu``) against the NumPy restatement of tests/manakov_numpy.py: fixed step at the smallest plan and
one row per route of the plan's table transform, both precisions; the adaptive rule; snapshots and the independence of the result from how far ahead
of the device's step control the steps are queued; invariance under a polarisation rotation; DBP; and the default path on a plan the Manakov line has
used.  Bounds: ``accuracy.tol(steps)`` in complex64, ``TOL_C128`` in complex128 (1e-7 for the adaptive complex128 end field, as the scalar adaptive
runs); every comparison is recorded through ``margins.within`` (profiles/manakov_margins.txt)."""
import functools

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, devices, workloads
from opticomlib_amd.accuracy import TOL_C128
from opticomlib_amd.typing import gv, optical_signal

import manakov_numpy as mk
from margins import within

pytestmark = pytest.mark.gpu

SMF = workloads.SMF
PRECISIONS = ["complex64", "complex128"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


@pytest.fixture(autouse=True)
def _grid():
    gv(**workloads.BENCH_GV)


@functools.lru_cache(maxsize=None)
def _field(k):
    a = workloads.qpsk_field(1 << k, seed=100 + k, power_w=10e-3)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _reference(k, precision, length, h, phi_max=0.01, kappa=None):
    """(end field, z) of the restatement, computed once per row and left as it is."""
    fn = mk.manakov_c64 if precision == "complex64" else mk.manakov_c128
    kw = {} if kappa is None else {"kappa": kappa}
    y, z = fn(_field(k), gv.dt, length=length, h=h, phi_max=phi_max, return_z=True, **SMF, **kw)
    y.flags.writeable = False
    return y, z


def _bound(precision, steps):
    return TOL_C128 if precision == "complex128" else None          # (None: margins.within takes tol(steps))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k, steps", mk.FIXED_ROWS)
def test_fixed_step_against_the_restatement(k, steps, precision):
    a = _field(k)
    ref, _ = _reference(k, precision, steps * 0.5, 0.5)
    out = oa.FIBER(optical_signal(a), length=steps * 0.5, h=0.5, precision=precision, coupling="manakov", **SMF)
    assert out.engine == "manakov_line"
    y = out.signal
    assert y.dtype == np.dtype(precision) and y.shape == a.shape
    assert within(y, ref, _bound(precision, steps), steps=steps, what=f"manakov restatement, {precision}, 2^{k} x 2")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_resident_input_and_kappa_one(precision):
    k, steps = 12, 40
    a = _field(k)
    kw = dict(length=steps * 0.5, h=0.5, precision=precision, coupling="manakov", **SMF)
    host = oa.FIBER(optical_signal(a), **kw).signal
    dev = _lib.DeviceArray.from_host(np.asarray(a, dtype=precision), np.dtype(precision))
    res = oa.FIBER(optical_signal.from_device(dev), **kw)
    assert isinstance(res._raw("signal"), _lib.DeviceArray)                    # (the result stays in GPU memory)
    assert np.array_equal(res.signal, host)
    ref, _ = _reference(k, precision, steps * 0.5, 0.5, kappa=1.0)
    y = oa.FIBER(optical_signal(a), kappa=1.0, **kw).signal
    assert within(y, ref, _bound(precision, steps), steps=steps, what=f"manakov restatement, kappa = 1, {precision}")
    # (kappa matters: a ninth of the nonlinear phase of 20 km at 20 mW in both polarisations is some 1e-2 rad)
    assert np.max(np.abs(y - host)) / np.max(np.abs(host)) > 1e-3


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k, length, phi_max", mk.ADAPTIVE_ROWS)
def test_adaptive_against_the_restatement(k, length, phi_max, precision):
    a = _field(k)
    ref, zr = _reference(k, precision, length, None, phi_max)
    kw = dict(length=length, phi_max=phi_max, precision=precision, coupling="manakov", **SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    assert abs(len(z) - len(zr)) <= 1
    assert abs(z[-1] - length) < 1e-4 and np.all(np.diff(z) > 0)
    steps = len(z) - 1
    bound = 1e-7 if precision == "complex128" else None
    assert within(A_z[-1], ref, bound, steps=steps, what=f"manakov restatement, adaptive, {precision} ({steps} vs {len(zr) - 1} steps)")
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert np.array_equal(y, A_z[-1])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h", [0.5, None])
def test_snapshots_and_chunks(h, precision):
    """The last snapshot is the plain run's output bit for bit; `every` and `z_list` pick among the full list's snapshots; the adaptive result does not
    depend on how many steps are queued between two looks at the step control."""
    k = 12
    a = _field(k)
    kw = dict(length=20, h=h, phi_max=0.05, precision=precision, coupling="manakov", **SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    steps = len(z) - 1
    assert steps == 40 if h else abs(steps - 15) <= 1
    assert np.array_equal(A_z[0], np.asarray(a, dtype=precision))
    y = oa.FIBER(optical_signal(a), **kw).signal
    assert np.array_equal(A_z[-1], y)
    assert np.all(np.abs(A_z[1:] - A_z[:-1]).max(axis=(1, 2)) > 0)            # (every snapshot is a step of its own)
    z7, A7 = oa.FIBER(optical_signal(a), return_steps=True, every=7, **kw)
    idx = _lib.every_index(steps, 7)
    assert np.array_equal(z7, z[idx]) and np.array_equal(A7, A_z[idx])
    z_list = [0.0, 3.3, 7.25, 12.0, 100.0]
    zl, Al = oa.FIBER(optical_signal(a), return_steps=True, z_list=z_list, **kw)
    idx = devices._keep_indices(z, len(z), None, z_list)
    assert idx[0] == 0 and idx[-1] == steps and np.array_equal(zl, z[idx]) and np.array_equal(Al, A_z[idx])
    if h is None:
        plan = devices.get_plan(1 << k, 2, devices._precision_code(precision))
        rt = plan.rdtype
        g = float(rt(rt(SMF["gamma"]) * rt(devices.MANAKOV_KAPPA)))
        with plan.lock:
            for chunk in (1, 3, 64):
                plan.set_field(np.asarray(a, dtype=precision))
                s, zc = plan.manakov_propagate(g, None, length=20.0, phi_max=0.05, chunk=chunk)
                assert s == steps and np.array_equal(zc, z), chunk
                assert np.array_equal(plan.get_field(), y), chunk


@pytest.mark.parametrize("precision", PRECISIONS)
def test_commutes_with_a_polarisation_rotation(precision):
    k, steps = 12, 40
    a = _field(k)
    U = mk.unitary(0.7, 0.4)
    kw = dict(length=steps * 0.5, h=0.5, precision=precision, **SMF)
    rotated_in = oa.FIBER(optical_signal(U @ a), coupling="manakov", **kw).signal
    rotated_out = U @ oa.FIBER(optical_signal(a), coupling="manakov", **kw).signal.astype(np.complex128)
    assert within(rotated_in, rotated_out, _bound(precision, steps), steps=steps, what=f"FIBER(U A) against U FIBER(A), {precision}")
    # the per-polarisation default does not commute with it
    y1 = oa.FIBER(optical_signal(U @ a), **kw).signal
    y2 = U @ oa.FIBER(optical_signal(a), **kw).signal.astype(np.complex128)
    assert np.max(np.abs(y1 - y2)) / np.max(np.abs(y2)) > 1e-2


@pytest.mark.parametrize("h", [0.5, None])
def test_dbp_is_fiber_with_negated_operators(h):
    a = _field(12)
    kw = dict(length=10, h=h, phi_max=0.05, coupling="manakov")
    back = oa.DBP(optical_signal(a), **kw, **SMF).signal
    fwd = oa.FIBER(optical_signal(a), **kw, **{name: -v for name, v in SMF.items()}).signal
    assert np.array_equal(back, fwd)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_default_path_after_a_manakov_run(precision):
    """coupling=None on a plan the Manakov line has used -- its table slots overwritten, their tags cleared -- gives what it gave before, bit for bit:
    the fused engines of the power-of-two plan, and the chirp-z line whose convolution tables live in the slots of the same plan (2 x 3000 samples run
    on the complex128 plan of 2 x 8192 points)."""
    a = _field(13)
    kw = dict(length=5, h=0.5, precision=precision, **SMF)
    odd = np.ascontiguousarray(a[:, :3000])
    before = oa.FIBER(optical_signal(a), **kw).signal
    before_odd = oa.FIBER(optical_signal(odd), **kw).signal
    before_adaptive = oa.FIBER(optical_signal(a), length=5, phi_max=0.05, precision=precision, **SMF).signal
    for p in PRECISIONS:
        oa.FIBER(optical_signal(a), length=5, h=0.5, precision=p, coupling="manakov", **SMF)
        oa.FIBER(optical_signal(a), length=5, phi_max=0.05, precision=p, coupling="manakov", **SMF)
    assert np.array_equal(oa.FIBER(optical_signal(odd), **kw).signal, before_odd)
    assert np.array_equal(oa.FIBER(optical_signal(a), **kw).signal, before)
    assert np.array_equal(oa.FIBER(optical_signal(a), length=5, phi_max=0.05, precision=precision, **SMF).signal, before_adaptive)
