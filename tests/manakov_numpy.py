"""NumPy restatement of ``FIBER(coupling="manakov")``.  TEST INFRASTRUCTURE.

The reference's split-step loop (``devices.py:1172-1196``, restated in ``oracle/ssfm_numpy.py``) with ONE line changed: the nonlinear operator
of both polarisations is ``1j * g * (|A[0]|^2 + |A[1]|^2)`` with ``g = gamma * kappa`` instead of each row's own ``1j * gamma * |A|^2``.
Coefficients, the linear operator, the stale ``N^`` over a step, ``z`` and the step rule are the oracle's: ``manakov_c64`` keeps every
coefficient, ``h`` and ``z`` in float32 and the field in complex64 (NumPy >= 2 does not promote), ``manakov_c128`` is the float64 twin.
With ``A[1] = 0`` and ``kappa = 1`` both are the scalar oracle of ``A[0]`` (tests/test_manakov_cpu.py).
"""
import numpy as np

from oracle import ssfm_numpy as orc

F32 = np.float32
KAPPA = 8.0 / 9.0


def _step(A, D, g, h_):
    """One symmetric step with the stale, shared N^ (``orc.ssfm_step_c64`` with the coupled power)."""
    P = np.abs(A[0]) ** 2 + np.abs(A[1]) ** 2
    N_hat = 1j * g * P
    A = A * np.exp(h_ / 2 * N_hat)
    A = np.fft.fft(A)
    A = A * np.exp(D * h_)
    A = np.fft.ifft(A)
    A = A * np.exp(h_ / 2 * N_hat)
    return A


def _max_gp(A, g):
    return (np.abs(g) * (np.abs(A[0]) ** 2 + np.abs(A[1]) ** 2)).max()


def _result(A, zs, As, return_z, return_steps):
    if return_steps:
        return np.array(zs), np.array(As)
    return (A, np.array(zs)) if return_z else A


def manakov_c64(field, dt, length=0.0, alpha=0.0, beta_2=0.0, beta_3=0.0, gamma=0.0, phi_max=0.01, h=None, kappa=KAPPA, return_z=False,
                return_steps=False, hs=None, max_steps=None):
    """``field``: (2, N).  Returns the complex64 end field; with ``return_z`` ``(field, z float64 (S+1,))``; with ``return_steps``
    ``(z, A_z (S+1, 2, N))``.  ``hs``: an explicit list of step sizes, taken in order as float32 values, ``z`` their float32 sum -- no clamping,
    ``length`` and ``h`` are ignored (``Plan.manakov_propagate(g, hs)``).  ``max_steps``: the loop stops after that many steps even when
    ``z < length`` (the step budget of the device's control kernel)."""
    c = orc._Coeffs32(length, alpha, beta_2, beta_3, gamma, phi_max)
    g = np.array(c.gamma * np.array(kappa, dtype=F32), dtype=F32)
    A = np.asarray(field, dtype=np.complex64)
    assert A.ndim == 2 and A.shape[0] == 2
    D = orc.linear_operator_c64(A.shape[-1], dt, alpha, beta_2, beta_3)
    if hs is not None:
        z = np.array(0, dtype=F32)
        zs, As = [0.0], [A.copy()]
        for h_ in hs:
            h_ = np.array(h_, dtype=F32)
            z += h_
            A = _step(A, D, g, h_)
            assert A.dtype == np.complex64 and z.dtype == F32
            zs.append(float(z))
            if return_steps:
                As.append(A.copy())
        return _result(A, zs, As, return_z, return_steps)
    if h is None:
        if (c.beta_2 == 0 and c.beta_3 == 0) or c.gamma == 0:
            h_ = c.length
        else:
            h_ = c.phi_max / _max_gp(A, g)
    else:
        h_ = np.array(h, dtype=F32)
    h_ = np.array(min(h_, c.length), dtype=F32)
    z = np.array(0, dtype=F32)
    zs, As = [0.0], [A.copy()]
    adapt = h is None and not ((c.beta_2 == 0 and c.beta_3 == 0) or c.gamma == 0)
    while z < c.length:
        z += h_
        A = _step(A, D, g, h_)
        assert A.dtype == np.complex64
        zs.append(float(z))
        if return_steps:
            As.append(A.copy())
        if adapt:
            h_ = c.phi_max / _max_gp(A, g)
        h_ = np.array(min(h_, c.length - z), dtype=F32)
        if max_steps is not None and len(zs) - 1 >= max_steps:
            break
    return _result(A, zs, As, return_z, return_steps)


def manakov_c128(field, dt, length=0.0, alpha=0.0, beta_2=0.0, beta_3=0.0, gamma=0.0, phi_max=0.01, h=None, kappa=KAPPA, return_z=False,
                 return_steps=False, hs=None, max_steps=None):
    """The float64 twin (``orc.fiber_c128`` with the coupled power); ``hs`` and ``max_steps`` as above, the steps and ``z`` Python floats."""
    A = np.asarray(field, dtype=np.complex128)
    assert A.ndim == 2 and A.shape[0] == 2
    D = orc.linear_operator_c128(A.shape[-1], dt, alpha, beta_2, beta_3)
    g = float(gamma) * float(kappa)
    length = float(length)
    if hs is not None:
        z = 0.0
        zs, As = [0.0], [A.copy()]
        for h_ in hs:
            h_ = float(h_)
            z += h_
            A = _step(A, D, g, h_)
            zs.append(z)
            if return_steps:
                As.append(A.copy())
        return _result(A, zs, As, return_z, return_steps)
    adapt = h is None and not ((beta_2 == 0 and beta_3 == 0) or gamma == 0)
    if h is None:
        h_ = phi_max / _max_gp(A, g) if adapt else length
    else:
        h_ = float(h)
    h_ = min(h_, length)
    z = 0.0
    zs, As = [0.0], [A.copy()]
    while z < length:
        z += h_
        A = _step(A, D, g, h_)
        zs.append(z)
        if return_steps:
            As.append(A.copy())
        if adapt:
            h_ = phi_max / _max_gp(A, g)
        h_ = min(h_, length - z)
        if max_steps is not None and len(zs) - 1 >= max_steps:
            break
    return _result(A, zs, As, return_z, return_steps)


def unitary(theta=0.7, phi=0.4):
    """A fixed polarisation rotation: U = [[cos t, -sin t e^{-i p}], [sin t e^{i p}, cos t]]."""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s * np.exp(-1j * phi)], [s * np.exp(1j * phi), c]])


# the parameter rows of tests/test_manakov_gpu.py (here, so that the CPU test can show that every one of them tells the two models apart)
FIXED_ROWS = [(8, 40), (12, 40), (13, 25), (14, 25), (17, 12), (18, 8)]          # (k, steps) at h = 0.5: length = steps / 2
ADAPTIVE_ROWS = [(14, 30, 0.01), (14, 30, 0.05), (12, 20, 0.05)]                 # (k, length, phi_max)

# the parameter rows of tests/test_manakov_edges_gpu.py; tests/test_manakov_cpu.py shows of each what makes it worth running
POWER_W = 10e-3                                                                  # mean power per polarisation of every row that does not state one
CLAMPED_ROW = (12, 10.3, 0.5, 21)                                                # (k, length, h, steps): 20 steps of 0.5 km and one of 0.3 km
SNAPSHOT_ADAPTIVE_ROWS = [(12, 20, 0.05), (14, 30, 0.05)]                        # (k, length, phi_max)
SCHEDULE_ROW = (10, (0.5, 0.25, 0.5, 0.125, 0.25, 0.5, 0.3, 0.3, 0.5))           # (k, hs): repeats, a reuse after eviction, an immediate repeat
PHASE_ROWS = [(k, power_w, steps, precisions)                                    # at h = 0.5; the phase per pass is h g max P
              for power_w, steps, precisions in ((0.3, 4, ("complex64", "complex128")), (3.0, 3, ("complex64", "complex128")), (30.0, 2, ("complex128",)))
              for k in (8, 12)]
UNIT_ROW = dict(k=8, power_w=2e5, gamma=1.3, h=0.5, gamma_alone=1e-12)           # one step without a linear operator: phases above 65000 rad
SIZE_ROWS = {"complex64": (9, 10, 11, 15, 16, 19, 20, 21, 22), "complex128": (9, 11, 16, 20, 22)}     # k; two steps of 0.5 km
BACKWARD_ROW = (12, 10, 0.05, 0.5, 12)                                           # (k, length, phi_max, h, adaptive steps) of DBP
BUDGET_ROW = (12, 20, 0.05, 6, 15)                                               # (k, length, phi_max, max_steps, steps of the full run)
DARK_ROWS = [(12, 40), (14, 40)]                                                 # (k, steps) at h = 0.5, and adaptive over the same length
