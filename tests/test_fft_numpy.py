"""tests/fft_numpy.py on its own (no GPU): the closed forms against the long-double transform, the root table's symmetry, NumPy's own transforms
inside the derived bounds at the ratios first measured for them, and the sensitivity check of the table comparison carried out on the host."""
import os

import numpy as np
import pytest
import scipy.fft

import fft_numpy as fn
import margins

U_LD = 2.0 ** -64
# NumPy's worst distance from the long-double transform on these inputs at 2^8 ... 2^22, in units of L u ||x||_1 per bin and L u normwise, is about
# 0.6 for impulses, 0.15 for tones, 0.1 for white noise and 0.25 normwise (re-measured and recorded below); the derived bounds are > 10 x wider.


def numpy_fft(x, prec):
    x = x.astype(fn.CDTYPE[prec])
    X = np.fft.fft(x)
    if X.dtype != x.dtype:          # (a NumPy that widens complex64: the same pocketfft in single precision through SciPy)
        X = scipy.fft.fft(x)
    assert X.dtype == x.dtype
    return X


def ld_coeff(log2n):
    """Theorem 24.2 for the long-double transform itself (twiddles to 4 u)."""
    eta = 4 * U_LD + fn.gamma(4, U_LD) * (np.sqrt(2) + 4 * U_LD)
    return 1.01 * log2n * eta          # (first order: float64 cannot hold 1 + eta)


@pytest.mark.parametrize("log2n", [3, 8, 12, 16])
def test_root_table_symmetry(log2n):
    n = 1 << log2n
    w = fn.roots(n)
    assert w.dtype == fn.CLD and w[0] == 1 and w[n // 2] == -1 and w[n // 4] == -1j and w[3 * n // 4] == 1j
    m = np.arange(n)
    np.testing.assert_array_equal(w[(m + n // 4) % n], -1j * w)                 # quarter turns, exactly
    np.testing.assert_array_equal(w[(n - m) % n], np.conj(w))                   # conjugate symmetry, exactly
    np.testing.assert_array_equal(w[(n // 4 - m[: n // 8 + 1])].real, -w[m[: n // 8 + 1]].imag)      # the octant's mirror, exactly
    assert w[n // 8].real == -w[n // 8].imag
    assert float(np.max(np.abs(np.abs(w) ** 2 - 1))) <= 4 * U_LD
    a = 2 * fn.PI_LD * m.astype(fn.LD) / n                                         # and against cos / sin of the full angle
    assert float(np.max(np.abs(w - (np.cos(a) - 1j * np.sin(a))))) <= 8 * U_LD * np.pi


@pytest.mark.parametrize("log2n", [8, 12, 16])
def test_closed_form_against_long_double_transform(log2n):
    sh = fn.shape(log2n, fn.C64)
    n = sh["n"]
    for j in fn.impulse_positions(sh):
        X = fn.ld_fft_raw(fn.make_input(n, ("impulse", j)))
        assert float(np.max(np.abs(X - fn.impulse_spectrum(n, j)))) <= ld_coeff(log2n), j


def test_inputs_are_complex64_values_and_batches_differ():
    sh = fn.shape(10, fn.C128)
    names = fn.input_names(sh)
    assert 16 <= len(names) == len(set(names)) <= 19          # (N1 = N2 here: two positions coincide)
    for name in names:
        x = fn.make_input(sh["n"], name)
        np.testing.assert_array_equal(x, x.astype(np.complex64).astype(np.complex128))
    for rows in (1, 2, 3):
        bs = fn.batches(names, rows)
        assert all(len(b) == rows == len(set(b)) for b in bs) and {m for b in bs for m in b} == set(names)
    assert fn.input_names(fn.shape(18, fn.C64)) == [("impulse", 1), ("impulse", (1 << 17) - 1), ("impulse", (1 << 18) - 1),
                                                     ("tone", fn.tone_bins(fn.shape(18, fn.C64), False)[0]), ("white", 0)]


def test_shapes_follow_the_plan():
    s = fn.shape(8, fn.C64)
    assert (s["N1"], s["N2"], s["E"], s["Ef"], s["u16"], s["twn_compute"]) == (16, 16, 8, 8, False, False)
    s = fn.shape(20, fn.C64)
    assert (s["N1"], s["N2"], s["E"], s["Ef"], s["Q"], s["u16"], s["twn_compute"]) == (256, 4096, 16, 16, 256, True, True)
    assert s["radices"] == ((16, 16), (16, 16, 16)) and s["lam"] == 3 + 5 + 1
    s = fn.shape(20, fn.C128)
    assert (s["E"], s["Ef"], s["u16"], s["twn_compute"]) == (8, 16, False, True)
    s = fn.shape(22, fn.C64, (8, 8))
    assert (s["N1"], s["N2"], s["E"], s["Ef"]) == (512, 8192, 16, 16) and s["radices"] == ((8, 8, 8), (16, 16, 16, 2)) and s["lam"] == 5 + 6 + 1
    for L in range(8, 23):
        for prec in (fn.C64, fn.C128):
            for pair in fn.PAIRS:
                s = fn.shape(L, prec, pair)                 # (asserts that eta's surplus covers the additions)
                assert 1 < s["mu"] / s["u"] < 16 and 5 < s["eta"] / s["u"] < 24 and 3 <= s["lam"] <= L + 1, (L, prec, pair, s)
    assert 1.0 < fn.MU_CONST[fn.C64] / fn.U[fn.C64] < 1.3


@pytest.mark.parametrize("log2n", [8, 12, 16, 20, 22])
@pytest.mark.parametrize("prec", [fn.C64, fn.C128], ids=["c64", "c128"])
def test_numpy_within_the_derived_bounds(log2n, prec):
    sh = fn.shape(log2n, prec)
    n, u = sh["n"], sh["u"]
    own, plan = fn.numpy_coeff(log2n, prec), fn.fwd_coeff(sh)
    worst = {}
    for name in fn.input_names(sh):
        X = numpy_fft(fn.make_input(n, name), prec)
        pb, nw = fn.forward_errors(X, name, n, log2n * u)                 # in units of L u
        worst[name[0]] = max(worst.get(name[0], 0.0), pb)
        if nw is not None:
            worst["norm"] = max(worst.get("norm", 0.0), nw)
    for kind, r in worst.items():
        if os.environ.get("SSFM_MARGINS_FILE"):          # (recorded where a run asks for margins; a plain CPU run writes nothing into the tree)
            margins.record(f"numpy log2n={log2n} {'c64' if prec == fn.C64 else 'c128'} {kind} [|d| / (L u |x|_1), norm: / (L u |X|_2)]", None, r,
                           own / (log2n * u))
        assert r * log2n * u <= own, (kind, r)                             # theorem 24.2 for a radix-2 transform with rounded twiddles
        assert r * log2n * u <= plan / 3, (kind, r)                       # ... and well inside what the plan of this size is allowed
        print(f"numpy 2^{log2n} {'c64' if prec == fn.C64 else 'c128'} {kind}: {r:.3f} L u; radix-2 bound {own / (log2n * u):.2f}, plan {plan / (log2n * u):.2f}")


@pytest.mark.parametrize("prec", [fn.C64, fn.C128], ids=["c64", "c128"])
def test_one_exchanged_entry_fails_at_exactly_two_bins(prec):
    """The table comparison of the GPU tests on a host stand-in for the device (NumPy's transform in the plan's precision): green with the table as
    it is, and with two entries exchanged it fails at those two bins and nowhere else."""
    sh = fn.shape(12, prec)
    n, cd = sh["n"], fn.CDTYPE[prec]
    H, _ = fn.unit_table(n, fn.seed_of("table", n), prec)
    j = fn.impulse_positions(sh)[-1]
    x = fn.make_input(n, ("impulse", j)).astype(cd)
    bound = np.sqrt(n) * fn.back_coeff(sh, fn.tau_host(sh))             # ||x||_2 = 1
    apply = lambda G: (scipy.fft.ifft(scipy.fft.fft(x) * G)).astype(cd)
    bad, worst = fn.spectrum_violations(apply(H), H, j, bound)
    assert bad.size == 0 and worst < 1
    pair = fn.swap_pair(H, fn.seed_of("pair", n))
    assert abs(complex(H[pair[0]]) - complex(H[pair[1]])) >= 1
    bad, worst = fn.spectrum_violations(apply(fn.swapped(H, pair)), H, j, bound)
    assert sorted(bad.tolist()) == sorted(pair) and worst > 100
    # the circular shift: an exact expectation in the time domain
    s = 2 * int(np.random.default_rng(fn.seed_of("shift", n)).integers(0, n // 2)) + 1
    y = apply(fn.shift_table(n, s, prec))
    want = np.zeros(n)
    want[(j + s) % n] = 1
    assert float(np.max(np.abs(y - want))) <= fn.back_coeff(sh, fn.tau_host(sh))
