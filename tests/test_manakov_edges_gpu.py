"""The Manakov line (csrc/manakov.hip, ``devices._fiber_manakov``, ``Plan.manakov_propagate``) on the GPU (``-m gpu``) at the branches that
tests/test_manakov_gpu.py leaves alone, against the NumPy restatement of tests/manakov_numpy.py.  What each group of rows is there for:

1. ``test_every_snapshot_fixed_step`` -- ``uc`` / ``phc`` of ``k_manakov_point``: a snapshot between two steps is the closing half rotation ALONE, code
   that no plain run uses (a snapshot taken behind the opening rotation as well, or with the wrong step's half size, differs from the restatement's
   ``A_z[i]`` by the nonlinear phase of half a step, 1e-2).  10.3 km at h = 0.5 ends on a clamped step of 0.3 km: the second table slot, another
   ``hh_prev`` / ``hh_next`` pair in the fused pass, and with ``every=4`` the last snapshot's slot ``ceil(21 / 4) - 1``.
2. ``test_every_snapshot_adaptive`` -- the same for the device's own step sizes (``ManakovCtl::h_prev`` / ``h``) and the slot arithmetic of the
   adaptive path (``ctl->steps``, ``snap_every``, the last step closed in state 1).
3. ``test_schedule_of_several_sizes`` -- ``slot = 1 - last_slot`` in ``manakov_run``: a table is remade in the slot the step before did not use; a
   schedule with repeats, a reuse after eviction and an immediate repeat multiplies by a stale table if that rule or the ``memcmp`` lookup is wrong.
4. ``test_phase_ranges`` / ``test_huge_phases_stay_unit_rotations`` -- ``rotate_all`` in this kernel's W = 4 (complex64) and W = 2 (complex128)
   instantiations beyond its first branch: ``sincos_tiny`` (<= 0.78 rad, 0.3 W), Cody-Waite / the library ``sincos`` (6.4 rad, 3 W; 64 rad, 30 W,
   complex128) and the double reduction above 65000 rad (2e5 W), where only the modulus says anything.
5. ``test_sizes`` -- the grid-stride loops: ``k_manakov_mktab`` wraps from 2^21, ``k_manakov_point<double>`` at 2^22, and every plan size between
   2^9 and 2^22 that the other file skips takes ``mktab``'s table through another layout of the plan's permuted ``D~``.
6. ``test_backward`` -- g < 0 against the restatement (``|g|`` in the control kernel, the sign of every phase), not against the kernel itself.
7. ``test_step_budget`` -- ``steps >= max_steps`` in ``k_manakov_control``: state 1 with z < L, the hand-over to the result buffer, and a
   ``ManakovCtl`` that must not leak into the next run.
8. ``test_one_polarisation_dark`` / ``test_zero_field`` -- the tie to the scalar engines (A[1] = 0, kappa = 1 is the scalar fibre of A[0]) and
   ``max P = 0``: h = inf, clamped to the length.
9. ``test_argument_checks`` -- every refusal of ``ssfm_manakov_propagate`` that returns before a launch, with the field left as it was.

Fields: ``workloads.qpsk_field(1 << k, seed=100 + k, power_w=...)`` (10 mW unless the row states a power).  Bounds: ``accuracy.tol(steps)`` in complex64,
``TOL_C128`` in complex128 with a fixed step, 1e-7 with the adaptive one; every comparison goes through ``margins.within`` and is recorded
(profiles/manakov_margins.txt).  tests/test_manakov_cpu.py shows for every row, without a GPU, that its reference is well conditioned and that it tells
the Manakov model from the per-polarisation one."""
import functools

import numpy as np
import pytest

import opticomlib_amd as oa
from opticomlib_amd import _lib, devices, workloads
from opticomlib_amd.accuracy import TOL_C128, tol
from opticomlib_amd.typing import gv, optical_signal
from oracle import ssfm_numpy as orc

import manakov_numpy as mk
from margins import record, within
from test_manakov_gpu import _grid, _need_gpu  # noqa: F401  (the module's autouse fixtures: a GPU is there, BENCH_GV is the grid)

pytestmark = pytest.mark.gpu

SMF = workloads.SMF
NEG_SMF = {name: -v for name, v in SMF.items()}
PRECISIONS = ["complex64", "complex128"]


@functools.lru_cache(maxsize=None)
def _field(k, power_w=mk.POWER_W):
    a = workloads.qpsk_field(1 << k, seed=100 + k, power_w=power_w)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=1)
def _large_field(k):
    """(the fields of the size rows: only the row that is running keeps its own)"""
    return _field.__wrapped__(k)


def _frozen(*arrays):
    for x in arrays:
        x.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _reference(precision, k, power_w=mk.POWER_W, backward=False, **run):
    """``(z, A_z)`` of the restatement on the SMF (negated: ``backward``), every step kept; computed once per row and left as it is."""
    gv(**workloads.BENCH_GV)
    fn = mk.manakov_c64 if precision == "complex64" else mk.manakov_c128
    return _frozen(*fn(_field(k, power_w), gv.dt, return_steps=True, **run, **(NEG_SMF if backward else SMF)))


@functools.lru_cache(maxsize=1)
def _size_reference(precision, k):
    gv(**workloads.BENCH_GV)
    fn = mk.manakov_c64 if precision == "complex64" else mk.manakov_c128
    return _frozen(fn(_large_field(k), gv.dt, length=1, h=0.5, **SMF))[0]


def _bound(precision, adaptive=False):
    if precision == "complex64":
        return None                                                   # (margins.within takes tol(steps))
    return 1e-7 if adaptive else TOL_C128


def _same_z(z, zr, precision):
    """Fixed step: both sides add the same float32 steps in complex64 (exactly equal); 1e-12 in complex128."""
    assert len(z) == len(zr)
    if precision == "complex64":
        assert np.array_equal(z, zr)
    else:
        assert np.max(np.abs(np.asarray(z) - np.asarray(zr))) <= 1e-12


def _each_within(got, want, steps_of, bound, what):
    """Every snapshot on its own -- ``got[j]`` against ``want[j]`` after ``steps_of[j]`` steps --, so that a failure names the step."""
    assert len(got) == len(want) == len(steps_of)
    bad = [s for y, r, s in zip(got, want, steps_of) if not within(y, r, bound, steps=max(int(s), 1), what=f"{what}, step {int(s)}")]
    assert not bad, f"{what}: the snapshots of steps {bad} miss the bound"


def _plan(k, precision, fibre=SMF):
    """The two-row plan of 2^k samples with the fibre's linear operator staged as ``_fiber_manakov`` stages it, and ``g`` as it computes it."""
    prec = devices._precision_code(precision)
    plan = devices.get_plan(1 << k, 2, prec)
    f = devices._Fibre.of(1.0, fibre["alpha"], fibre["beta_2"], fibre["beta_3"], fibre["gamma"], 0.01, 0.5, float(gv.dt), prec)
    tag = devices._tag("fibre", f.dt, float(f.alpha), float(f.beta_2), float(f.beta_3))
    with plan.lock:
        if plan.tag(0) != tag:
            plan.set_linear_operator(f.operator(plan.n))
            plan.set_tag(0, tag)
    rt = plan.rdtype
    return plan, float(rt(rt(fibre["gamma"]) * rt(devices.MANAKOV_KAPPA)))


def _snaps(plan, count, fill=None):
    if fill is None:
        return _lib.DeviceArray((count, 2, plan.n), plan.cdtype, plan.device)
    return _lib.DeviceArray.from_host(np.full((count, 2, plan.n), fill, dtype=plan.cdtype), plan.cdtype, plan.device)


def _host(plan, snaps):
    plan.synchronize()
    return np.array(snaps.to_host())


# ---- 1. every snapshot, fixed step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_snapshot_fixed_step(precision):
    k, length, h, steps = mk.CLAMPED_ROW
    a = _field(k)
    zr, Ar = _reference(precision, k, length=length, h=h)
    assert len(zr) == steps + 1
    bound = _bound(precision)
    kw = dict(length=length, h=h, precision=precision, coupling="manakov", **SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    _same_z(z, zr, precision)
    assert A_z.dtype == np.dtype(precision) and np.array_equal(A_z[0], np.asarray(a, dtype=precision))
    _each_within(A_z[1:], Ar[1:], range(1, steps + 1), bound, f"snapshot against the restatement, h = {h} over {length} km, {precision}")
    assert np.array_equal(oa.FIBER(optical_signal(a), **kw).signal, A_z[-1])

    z4, A4 = oa.FIBER(optical_signal(a), return_steps=True, every=4, **kw)
    idx = _lib.every_index(steps, 4)
    assert idx == [0, 4, 8, 12, 16, 20, 21] and np.array_equal(z4, z[idx])
    _each_within(A4[1:], Ar[idx[1:]], idx[1:], bound, f"snapshot against the restatement, every = 4, {precision}")
    assert np.array_equal(A4, A_z[idx])

    z_list = [0, 3.3, 10.2, 10.3, 50]
    zl, Al = oa.FIBER(optical_signal(a), return_steps=True, z_list=z_list, **kw)
    idx = devices._keep_indices(z, len(z), None, z_list)
    assert idx == [0, 7, 21, 21, 21] and np.array_equal(zl, z[idx])
    assert np.array_equal(Al[0], A_z[0])
    _each_within(Al[1:], Ar[idx[1:]], idx[1:], bound, f"snapshot against the restatement, z_list, {precision}")
    assert np.array_equal(Al, A_z[idx])


# ---- 2. every snapshot, adaptive
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k, length, phi_max", mk.SNAPSHOT_ADAPTIVE_ROWS)
def test_every_snapshot_adaptive(k, length, phi_max, precision):
    a = _field(k)
    zr, Ar = _reference(precision, k, length=length, phi_max=phi_max)
    bound = _bound(precision, adaptive=True)
    kw = dict(length=length, phi_max=phi_max, precision=precision, coupling="manakov", **SMF)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, **kw)
    steps = len(z) - 1
    assert abs(len(z) - len(zr)) <= 1
    shorter = min(len(z), len(zr))
    stop = shorter if len(z) == len(zr) else shorter - 1              # (the final entry is left out when the counts differ)
    compared = list(range(1, stop))
    assert len(compared) >= steps - 1                                 # (at most one snapshot, the last, is excluded)
    assert np.array_equal(A_z[0], np.asarray(a, dtype=precision)) and z[0] == 0
    assert np.max(np.abs(z[compared] - zr[compared])) <= 1e-4
    _each_within(A_z[compared], Ar[compared], compared, bound, f"adaptive snapshot against the restatement, 2^{k}, {precision}")

    z4, A4 = oa.FIBER(optical_signal(a), return_steps=True, every=4, **kw)
    idx = _lib.every_index(steps, 4)
    assert np.array_equal(z4, z[idx]) and len(A4) == len(idx)
    kept = [(j, i) for j, i in enumerate(idx) if 0 < i < stop]
    assert len(kept) >= len(idx) - 2                                  # (the input and at most the last one are not compared)
    _each_within(A4[[j for j, _ in kept]], Ar[[i for _, i in kept]], [i for _, i in kept], bound,
                 f"adaptive snapshot against the restatement, every = 4, 2^{k}, {precision}")
    assert np.array_equal(A4, A_z[idx])


# ---- 3. schedules of several sizes
@pytest.mark.parametrize("precision", PRECISIONS)
def test_schedule_of_several_sizes(precision):
    k, hs = mk.SCHEDULE_ROW
    hs = list(hs)
    n_steps = len(hs)
    x = np.asarray(_field(k), dtype=precision)
    zr, Ar = _reference(precision, k, hs=tuple(hs))
    bound = _bound(precision)
    plan, g = _plan(k, precision)
    with plan.lock:
        plan.set_field(x)
        s, z = plan.manakov_propagate(g, hs)
        end = np.array(plan.get_field())
        assert s == n_steps and z is None
        assert within(end, Ar[-1], bound, steps=n_steps, what=f"schedule of {len(set(hs))} sizes against the restatement, {precision}")

        every_step = _snaps(plan, n_steps, fill=np.nan)
        plan.set_field(x)
        assert plan.manakov_propagate(g, hs, snaps=every_step, every=1)[0] == n_steps
        S1 = _host(plan, every_step)
        _each_within(S1, Ar[1:], range(1, n_steps + 1), bound, f"schedule of {len(set(hs))} sizes, snapshot against the restatement, {precision}")
        assert np.array_equal(S1[-1], end)
        assert np.array_equal(plan.get_field(), end)                  # (the same schedule twice on one plan: identical bits)

        idx = _lib.every_index(n_steps, 2)[1:]
        assert idx == [2, 4, 6, 8, 9]
        every_other = _snaps(plan, len(idx), fill=np.nan)
        plan.set_field(x)
        assert plan.manakov_propagate(g, hs, snaps=every_other, every=2)[0] == n_steps
        S2 = _host(plan, every_other)
        assert np.array_equal(S2, S1[[i - 1 for i in idx]])
        assert np.array_equal(plan.get_field(), end)


# ---- 4. the phase ranges of rotate_all
@pytest.mark.parametrize("k, power_w, steps, precision", [(k, p, s, precision) for k, p, s, precisions in mk.PHASE_ROWS for precision in precisions])
def test_phase_ranges(k, power_w, steps, precision):
    a = _field(k, power_w)
    _, Ar = _reference(precision, k, power_w, length=steps * 0.5, h=0.5)
    y = oa.FIBER(optical_signal(a), length=steps * 0.5, h=0.5, precision=precision, coupling="manakov", **SMF).signal
    assert y.dtype == np.dtype(precision) and np.isfinite(y).all()
    assert within(y, Ar[-1], _bound(precision), steps=steps, what=f"manakov restatement at {power_w} W, {precision}, 2^{k} x 2")


def test_huge_phases_stay_unit_rotations():
    """Above 65000 rad one float32 ulp of the phase is 4e-3 rad and no value comparison means anything; what the source claims of its double
    reduction is "still a unit rotation".  One step without a linear operator: the modulus moves by no more than 4 times what the same plan's table
    transform alone (the same call, gamma so small that no phase exceeds 2^-5) moves it."""
    u = mk.UNIT_ROW
    a = _field(u["k"], u["power_w"])
    x = np.asarray(a, dtype=np.complex64)
    kw = dict(length=u["h"], h=u["h"], alpha=0.0, beta_2=0.0, beta_3=0.0, precision="complex64", coupling="manakov")
    peak = float(np.max(np.abs(x)))

    def modulus_error(gamma):
        y = oa.FIBER(optical_signal(a), gamma=gamma, **kw).signal
        assert y.dtype == np.complex64 and np.isfinite(y).all()
        return float(np.max(np.abs(np.abs(y).astype(np.float64) - np.abs(x).astype(np.float64)))) / peak

    alone = modulus_error(u["gamma_alone"])
    turned = modulus_error(u["gamma"])
    record("|out| - |in| of the table transform alone, complex64", 1, alone, tol(1))
    record("|out| - |in| behind phases above 65000 rad, bound = 4 x the table transform alone", 1, turned, 4 * alone)
    assert alone < tol(1)
    assert turned < 4 * alone


# ---- 5. sizes
@pytest.mark.parametrize("k, precision", [(k, p) for k in sorted(set(sum(map(tuple, mk.SIZE_ROWS.values()), ()))) for p in PRECISIONS if k in mk.SIZE_ROWS[p]])
def test_sizes(k, precision):
    a = _large_field(k)
    ref = _size_reference(precision, k)
    out = oa.FIBER(optical_signal(a), length=1, h=0.5, precision=precision, coupling="manakov", **SMF)
    assert out.engine == "manakov_line"
    y = out.signal
    assert y.dtype == np.dtype(precision) and y.shape == a.shape
    assert within(y, ref, _bound(precision), steps=2, what=f"manakov restatement, two steps, {precision}, 2^{k} x 2")


# ---- 6. backward
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("adaptive", [True, False])
def test_backward(adaptive, precision):
    k, length, phi_max, h, ref_steps = mk.BACKWARD_ROW
    a = _field(k)
    run = dict(length=length, phi_max=phi_max) if adaptive else dict(length=length, h=h)
    zr, Ar = _reference(precision, k, backward=True, **run)
    kw = dict(precision=precision, coupling="manakov", **run, **SMF)
    z, A_z = oa.DBP(optical_signal(a), return_steps=True, **kw)
    steps = len(z) - 1
    if adaptive:
        assert len(zr) - 1 == ref_steps and abs(len(z) - len(zr)) <= 1
        assert abs(z[-1] - length) < 1e-4 and np.all(np.diff(z) > 0)
    else:
        _same_z(z, zr, precision)
    assert within(A_z[-1], Ar[-1], _bound(precision, adaptive), steps=steps,
                  what=f"DBP against the restatement on the negated fibre, {'adaptive' if adaptive else f'h = {h}'}, {precision} ({steps} vs {len(zr) - 1} steps)")
    assert np.array_equal(oa.DBP(optical_signal(a), **kw).signal, A_z[-1])


# ---- 7. the step budget
@pytest.mark.parametrize("precision", PRECISIONS)
def test_step_budget(precision):
    k, length, phi_max, max_steps, ref_steps = mk.BUDGET_ROW
    x = np.asarray(_field(k), dtype=precision)
    run = dict(length=float(length), phi_max=phi_max)
    plan, g = _plan(k, precision)
    with plan.lock:
        plan.set_field(x)
        full_steps, z_full = plan.manakov_propagate(g, None, **run)
        end = np.array(plan.get_field())
        assert abs(full_steps - ref_steps) <= 1 and full_steps > max_steps
        every_step = _snaps(plan, full_steps, fill=np.nan)
        plan.set_field(x)
        s, z = plan.manakov_propagate(g, None, snaps=every_step, every=1, **run)
        full = _host(plan, every_step)
        assert s == full_steps and np.array_equal(z, z_full) and np.array_equal(full[-1], end) and np.array_equal(plan.get_field(), end)

        plan.set_field(x)
        s, z = plan.manakov_propagate(g, None, max_steps=max_steps, **run)
        assert s == max_steps and z[-1] < length
        assert np.array_equal(z, z_full[: max_steps + 1])
        assert np.array_equal(plan.get_field(), full[max_steps - 1])            # (test 2 ties the full run's snapshots to the restatement)

        two = _snaps(plan, 2, fill=np.nan)
        plan.set_field(x)
        s, z = plan.manakov_propagate(g, None, max_steps=max_steps, snaps=two, every=4, **run)
        assert s == max_steps and np.array_equal(z, z_full[: max_steps + 1])
        assert np.array_equal(_host(plan, two), full[[3, max_steps - 1]])       # (steps 4 and 6)
        assert np.array_equal(plan.get_field(), full[max_steps - 1])

        plan.set_field(x)                                                       # (no stale ManakovCtl: a full run behind it is what it was)
        s, z = plan.manakov_propagate(g, None, **run)
        assert s == full_steps and np.array_equal(z, z_full) and np.array_equal(plan.get_field(), end)


# ---- 8. one polarisation dark
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("k, steps", mk.DARK_ROWS)
def test_one_polarisation_dark(k, steps, adaptive, precision):
    a = np.array(_field(k))
    a[1] = 0
    run = dict(length=steps * 0.5, phi_max=0.05) if adaptive else dict(length=steps * 0.5, h=0.5)
    z, A_z = oa.FIBER(optical_signal(a), return_steps=True, precision=precision, coupling="manakov", kappa=1.0, **run, **SMF)
    taken = len(z) - 1
    assert taken == steps if not adaptive else taken >= 2
    y = A_z[-1]
    assert y.shape == a.shape and not y[1].any()
    scalar = oa.FIBER(optical_signal(a[0]), precision=precision, **run, **SMF).signal
    oracle = (orc.fiber_c64 if precision == "complex64" else orc.fiber_c128)(a[0], gv.dt, **run, **SMF)
    bound = _bound(precision, adaptive)
    how = "adaptive" if adaptive else "h = 0.5"
    assert within(y[0], scalar, bound, steps=taken, what=f"row 0 of a dark second row, kappa = 1, against the scalar FIBER, {how}, {precision}, 2^{k}")
    assert within(y[0], oracle, bound, steps=taken, what=f"row 0 of a dark second row, kappa = 1, against the scalar oracle, {how}, {precision}, 2^{k}")
    assert within(scalar, oracle, bound, steps=taken, what=f"the scalar FIBER against the scalar oracle, {how}, {precision}, 2^{k}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_field(precision):
    """max P = 0: h = phi_max / 0 = inf, clamped to the length -- one step, and nothing but zeros."""
    zero = np.zeros((2, 1 << 12), dtype=np.complex128)
    kw = dict(length=20, phi_max=0.05, precision=precision, coupling="manakov", **SMF)
    z, A_z = oa.FIBER(optical_signal(zero), return_steps=True, **kw)
    assert np.array_equal(z, [0.0, 20.0])
    assert A_z.shape == (2, 2, 1 << 12) and np.isfinite(A_z).all() and not A_z.any()
    y = oa.FIBER(optical_signal(zero), **kw).signal
    assert np.isfinite(y).all() and not y.any()


# ---- 9. the argument checks of the entry point
@pytest.mark.parametrize("precision", PRECISIONS)
def test_argument_checks(precision):
    k = 10
    n = 1 << k
    x = np.asarray(_field(k), dtype=precision)
    adaptive = dict(length=20.0, phi_max=0.05)

    def refused(plan, field, message, *args, **kw):
        with pytest.raises(_lib.SsfmError, match=message):
            plan.manakov_propagate(*args, **kw)
        assert np.array_equal(plan.get_field(), field), message

    for rows in (1, 4):
        other = devices.get_plan(n, rows, devices._precision_code(precision))
        f = np.ascontiguousarray(np.resize(x, (rows, n)))
        with other.lock:
            other.set_field(f)
            refused(other, f, rf"a plan of two rows \(the polarisations\) is needed, this one has {rows}", 1.0, [0.5])

    plan, g = _plan(k, precision)
    with plan.lock:
        plan.set_field(x)
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            refused(plan, x, r"step 1 is \S+ km \(must be positive and finite\)", g, [0.5, bad, 0.5])
        refused(plan, x, r"9 steps, every 2: more than 4 snapshots", g, [0.5] * 9, snaps=_snaps(plan, 4), every=2)
        refused(plan, x, r"chunk = -1", g, None, chunk=-1, **adaptive)
        refused(plan, x, r"chunk = -1", g, [0.5], chunk=-1)
        refused(plan, x, r"an adaptive run needs length > 0, phi_max > 0 and g != 0 \(length = 20, phi_max = 0\.05, g = 0\)", 0.0, None, **adaptive)
        refused(plan, x, r"an adaptive run needs length > 0, phi_max > 0 and g != 0 \(length = 0,", g, None, length=0.0, phi_max=0.05)
        refused(plan, x, r"an adaptive run needs length > 0, phi_max > 0 and g != 0 \(length = 20, phi_max = 0,", g, None, length=20.0, phi_max=0.0)
        refused(plan, x, r"max_steps = 0", g, None, max_steps=0, **adaptive)
        assert plan.manakov_propagate(g, []) == (0, None)
        assert np.array_equal(plan.get_field(), x)
        # and the plan is as good as before: a run behind the refusals is the run of a fresh field
        _, Ar = _reference(precision, k, hs=mk.SCHEDULE_ROW[1])
        assert plan.manakov_propagate(g, list(mk.SCHEDULE_ROW[1]))[0] == len(mk.SCHEDULE_ROW[1])
        assert within(plan.get_field(), Ar[-1], _bound(precision), steps=len(mk.SCHEDULE_ROW[1]), what=f"a schedule behind the refused calls, {precision}")
