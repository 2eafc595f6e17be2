"""tests/psd_numpy.py pinned without a GPU: the long-double Welch reference against SciPy on white noise, against the closed form of a
bin-centred complex exponential, and its bin subset against the full result; the bound's pieces against their definitions."""
import numpy as np
import pytest
import scipy.signal as sg

import psd_numpy as pn


def scipy_psd(x, nperseg):
    p = sg.welch(x, fs=1.0, nperseg=nperseg, scaling="spectrum", return_onesided=False, detrend=False)[1]
    return np.fft.fftshift(p, axes=-1)


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    pn._need_long_double()


def test_the_guard_fails_loudly_when_long_double_is_double(monkeypatch):
    monkeypatch.setattr(pn, "LD", np.float64)
    with pytest.raises(AssertionError, match="not an 80-bit type"):
        pn.welch_ref(np.ones(32), 16)


@pytest.mark.parametrize("nperseg", (1, 2, 5, 15, 16, 17, 100, 256))
@pytest.mark.parametrize("cplx", (False, True), ids=("real", "complex"))
def test_against_scipy_on_white_noise(nperseg, cplx):
    """SciPy's float64 estimate is within the bound's unit u T A_k of the reference (r of a few at the most), bin by bin."""
    rng = np.random.default_rng(100 + nperseg)
    for rows, n in ((1, nperseg), (3, 7 * nperseg + nperseg // 3)):
        x = rng.standard_normal((rows, n))
        if cplx:
            x = x + 1j * rng.standard_normal((rows, n))
        p, A, B = pn.welch_ref(x, nperseg)
        ps = scipy_psd(x, nperseg)
        assert p.dtype == np.longdouble and p.shape == ps.shape == A.shape and B.shape == (rows,)
        r = pn.scipy_r(ps, p, A, pn.depth(nperseg))
        assert r <= pn.R_SCIPY_MAX, (nperseg, rows, n, r)
        assert np.all(np.abs(ps - p) <= pn.bound(A, B, pn.depth(nperseg)))
        assert float(np.max(np.abs(ps - p) / p)) < 1e-13                       # and plainly: the float64 level, relative, in every bin
        A64, B64 = pn.welch_terms64(x, nperseg)
        assert np.allclose(A64, A.astype(np.float64), rtol=1e-9, atol=0) and np.allclose(B64, B.astype(np.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("L", (8, 16, 100, 101, 1024))
def test_a_bin_centred_exponential_has_three_bins(L):
    """x = exp(2 pi i q m / L): every segment is the same tone up to a phase, its Hann-windowed DFT is L/2 at bin q and -L/4 at q +- 1, so
    with scale = (2 / L)^2 the spectrum is 1/4 : 1 : 1/4 and zero elsewhere."""
    q = L // 8
    n = 4 * L + 3
    a = 2 * pn._pi() * ((q * np.arange(n)) % L).astype(np.longdouble) / L
    x = np.cos(a) + 1j * np.sin(a)
    p, A, B = pn.welch_ref(x, L)
    want = np.zeros(L, np.longdouble)
    o = (q + L // 2) % L
    want[o], want[o - 1], want[(o + 1) % L] = 1.0, 0.25, 0.25
    assert float(np.max(np.abs(p - want))) < 1e-17, float(np.max(np.abs(p - want)))
    assert abs(float(B) - 1.5 / L) < 1e-17                                      # sum w^2 = 3L/8, scale = 4 / L^2


def test_a_subset_of_bins_is_the_full_result_bit_for_bit():
    rng = np.random.default_rng(5)
    for L, n in ((17, 200), (64, 500), (100, 777)):
        x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
        p, A, B = pn.welch_ref(x, L)
        bins = np.array(sorted(rng.choice(L, size=min(L, 9), replace=False)))
        ps, As, Bs = pn.welch_ref(x, L, bins=bins)
        np.testing.assert_array_equal(ps, p[:, bins])
        np.testing.assert_array_equal(As, A[:, bins])
        np.testing.assert_array_equal(Bs, B)
        p1, A1, B1 = pn.welch_ref(x[1], L, bins=bins)                           # 1-D in, 1-D out
        np.testing.assert_array_equal(p1, p[1, bins])
        assert p1.shape == (bins.size,) and np.ndim(B1) == 0


def test_trailing_samples_are_dropped():
    rng = np.random.default_rng(6)
    x = rng.standard_normal(5 * 16 + 7)
    y = x.copy()
    y[5 * 16:] = 1e30
    np.testing.assert_array_equal(pn.welch_ref(x, 32)[0], pn.welch_ref(y, 32)[0])


def test_depth_per_route():
    assert pn.depth(1) == 1.0 and pn.depth(9) == 3.0
    assert pn.depth(16) == 4.0 and pn.depth(8192) == 13.0
    assert pn.depth(17) == 3 * 8 and pn.depth(128 + 1) == 3 * 9 and pn.depth(1000) == 3 * 11 and pn.depth(1 << 21) == 3 * 22
    assert pn.depth(16384) == 3 * 15


def test_k_is_four_times_scipys_worst_ratio():
    assert pn.K == int(np.ceil(4 * pn.R_SCIPY_MAX))


def test_f32_neighbours():
    ref = np.array([1.0, 1.0 + 2.0 ** -24, 1e-40, 3.0])
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    assert pn.f32_neighbours(np.array([one, up, 5.0, 3.0], np.float32), ref).all()          # (a subnormal reference is not judged)
    assert not pn.f32_neighbours(np.array([np.nextafter(up, np.float32(2))], np.float32), ref[:1]).any()
