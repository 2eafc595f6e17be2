"""NumPy restatement of ``FIBER(coupling="manakov", pmd=...)``: the Manakov-PMD equation in the coarse-step (waveplate) model, one section per
split step.  TEST INFRASTRUCTURE.

The loop of tests/manakov_numpy.py with two lines added to its step: behind the opening half rotation the unitary ``U_k`` of the step (not with
``pmd_scatter=False``), and in the linear operator the differential delay ``tau = D_p sqrt(h)``: row 0 is delayed by ``tau / 2``, row 1 advanced.
Coefficients, the stale ``N^``, ``z``, the single-step rule and the adaptive rule are that file's (a unitary leaves ``P`` as it is): ``pmd_c64``
keeps every coefficient, ``h``, ``tau`` and ``z`` in float32 and the field in complex64, ``pmd_c128`` is the float64 twin.  With ``pmd=0`` and
``pmd_scatter=False`` both are ``manakov_c64`` / ``manakov_c128`` bit for bit (tests/test_manakov_pmd_cpu.py).  ``sections`` is this file's own
copy of the recipe of ``devices.pmd_sections``."""
import numpy as np

from oracle import ssfm_numpy as orc

import manakov_numpy as mk

F32 = np.float32
MAX_STEPS = 1 << 17                 # the step budget of FIBER's adaptive run: as many unitaries are drawn, once


def sections(seed, count):
    """``(count, 2, 2)`` complex128, Haar on SU(2): a normal 4-vector per section scaled to unit length, ``a = q0 + 1j q1``, ``b = q2 + 1j q3``,
    ``U = [[a, b], [-conj(b), conj(a)]]``."""
    q = np.random.default_rng(seed).standard_normal((count, 4))
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    a, b = q[:, 0] + 1j * q[:, 1], q[:, 2] + 1j * q[:, 3]
    return np.stack([np.stack([a, b], axis=-1), np.stack([-np.conj(b), np.conj(a)], axis=-1)], axis=-2)


def _step(A, D, w, g, h_, dp, U):
    """One symmetric step: ``mk._step`` with the unitary behind the opening rotation and the per-row delay in the linear operator.  ``dp`` and ``h_``
    are 0-d arrays (or floats) of the run's real type, ``U`` a (2, 2) array of the field's type or None."""
    P = np.abs(A[0]) ** 2 + np.abs(A[1]) ** 2
    N_hat = 1j * g * P
    A = A * np.exp(h_ / 2 * N_hat)
    if U is not None:
        A = np.stack([U[0, 0] * A[0] + U[0, 1] * A[1],
                      U[1, 0] * A[0] + U[1, 1] * A[1]])
    A = np.fft.fft(A)
    tau = dp * np.sqrt(h_)
    A = np.stack([A[r] * np.exp(D * h_ + s_r * (-0.5j) * (w * tau)) for r, s_r in ((0, +1), (1, -1))])
    A = np.fft.ifft(A)
    A = A * np.exp(h_ / 2 * N_hat)
    return A


def _count_fixed(h_, length, zero):
    """Steps of the loop below with a step that only the clamp changes (a fixed ``h`` or the single step)."""
    z, count = zero.copy(), 0
    while z < length:
        z += h_
        count += 1
        h_ = min(h_, length - z)
    return count


def _run(ct, rt, field, dt, length, alpha, beta_2, beta_3, gamma, phi_max, h, kappa, return_z, return_steps, hs, max_steps, pmd, pmd_seed, pmd_scatter):
    c64 = ct == np.complex64
    real = (lambda v: np.array(v, dtype=F32)) if c64 else float
    A = np.asarray(field, dtype=ct)
    assert A.ndim == 2 and A.shape[0] == 2
    n = A.shape[-1]
    if c64:
        c = orc._Coeffs32(length, alpha, beta_2, beta_3, gamma, phi_max)
        g = np.array(c.gamma * np.array(kappa, dtype=F32), dtype=F32)
        D = orc.linear_operator_c64(n, dt, alpha, beta_2, beta_3)
        w = np.asarray(orc.angular_frequency(n, dt) * 1e-12, dtype=F32)
        L, phi, single = c.length, c.phi_max, bool((c.beta_2 == 0 and c.beta_3 == 0) or c.gamma == 0)
    else:
        g = float(gamma) * float(kappa)
        D = orc.linear_operator_c128(n, dt, alpha, beta_2, beta_3)
        w = orc.angular_frequency(n, dt) * 1e-12
        L, phi, single = float(length), phi_max, bool((beta_2 == 0 and beta_3 == 0) or gamma == 0)
    dp = real(pmd)
    zero = real(0)

    def unitaries(count):
        return sections(pmd_seed, count).astype(ct) if pmd_scatter else [None] * count

    def check(A, z):
        assert A.dtype == ct and (not c64 or z.dtype == F32)

    zs, As = [0.0], [A.copy()]
    if hs is not None:
        z = zero.copy() if c64 else 0.0
        for h_, U in zip(hs, unitaries(len(hs))):
            h_ = real(h_)
            z += h_
            A = _step(A, D, w, g, h_, dp, U)
            check(A, z)
            zs.append(float(z))
            if return_steps:
                As.append(A.copy())
        return mk._result(A, zs, As, return_z, return_steps)
    adapt = h is None and not single
    if h is None:
        h_ = phi / mk._max_gp(A, g) if adapt else L
    else:
        h_ = real(h)
    h_ = real(min(h_, L))
    budget = MAX_STEPS if max_steps is None else max_steps
    Us = unitaries(budget if adapt else _count_fixed(h_, L, np.array(0, dtype=F32) if c64 else np.array(0.0)))
    z = zero.copy() if c64 else 0.0
    while z < L:
        k = len(zs) - 1
        z += h_
        A = _step(A, D, w, g, h_, dp, Us[k])
        check(A, z)
        zs.append(float(z))
        if return_steps:
            As.append(A.copy())
        if adapt:
            h_ = phi / mk._max_gp(A, g)
        h_ = real(min(h_, L - z))
        if max_steps is not None and len(zs) - 1 >= max_steps:
            break
    return mk._result(A, zs, As, return_z, return_steps)


def pmd_c64(field, dt, length=0.0, alpha=0.0, beta_2=0.0, beta_3=0.0, gamma=0.0, phi_max=0.01, h=None, kappa=mk.KAPPA, return_z=False,
            return_steps=False, hs=None, max_steps=None, pmd=0.0, pmd_seed=0, pmd_scatter=True):
    """``mk.manakov_c64`` with PMD: ``pmd`` = D_p [ps/sqrt(km)], ``pmd_seed`` the seed of the sections (one per step: ``len(hs)``, the step count of a
    fixed ``h``, ``max_steps`` -- 2^17 when None -- of them for the adaptive rule), ``pmd_scatter=False``: no unitaries."""
    return _run(np.complex64, F32, field, dt, length, alpha, beta_2, beta_3, gamma, phi_max, h, kappa, return_z, return_steps, hs, max_steps,
                pmd, pmd_seed, pmd_scatter)


def pmd_c128(field, dt, length=0.0, alpha=0.0, beta_2=0.0, beta_3=0.0, gamma=0.0, phi_max=0.01, h=None, kappa=mk.KAPPA, return_z=False,
             return_steps=False, hs=None, max_steps=None, pmd=0.0, pmd_seed=0, pmd_scatter=True):
    """The float64 twin."""
    return _run(np.complex128, np.float64, field, dt, length, alpha, beta_2, beta_3, gamma, phi_max, h, kappa, return_z, return_steps, hs, max_steps,
                pmd, pmd_seed, pmd_scatter)


def jones_dgd(dp, hs, Us, w0=0.0, dw=1e-3):
    """DGD [ps] at ``w0`` [rad/ps] of the linear line alone: ``T(w) = prod_k diag(exp(-+ i w tau_k / 2)) U_k``, ``DGD = 2 sqrt|det dT/dw|`` (central
    difference; ``T`` is in SU(2), so ``dT/dw T^-1`` is traceless anti-Hermitian with eigenvalues ``+- i DGD / 2``)."""
    def T(w):
        M = np.eye(2, dtype=np.complex128)
        for h_, U in zip(hs, Us):
            tau = dp * np.sqrt(h_)
            M = np.diag([np.exp(-0.5j * w * tau), np.exp(+0.5j * w * tau)]) @ U @ M
        return M
    dT = (T(w0 + dw) - T(w0 - dw)) / (2 * dw)
    return 2.0 * np.sqrt(abs(np.linalg.det(dT)))
