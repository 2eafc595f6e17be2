"""Long-double reference and derived error bounds for the four-step power-of-two transform of csrc/ssfm_kernels.hpp (k_time / k_freq over
csrc/wgfft.hpp) and for what comes back through its transfer tables.  No GPU.  Test infrastructure.

Reference.  `ld_fft` is scipy.fft.fft on np.clongdouble (u = 2^-64), cached (`Cache`); `roots(n)` is the long-double table w[m] = exp(-2 pi i m / n), built from
one octant and filled by exact symmetry, so that the spectrum of a unit impulse at j is the closed form w[(j k) % n], independent of any FFT.

Plan shapes (`shape`), restated from PlanT::init of csrc/ssfm_host.hip: n = N1 N2 with N1 = 2^min(L // 2, 8) up to 2^20 and 512 above; the column
pass holds E and the row pass Ef points per thread (SSFM_E / SSFM_EF, defaults by size and precision); Q = N2 / Ef orders the tables
(freq_tab_pos); complex64 plans with (N1 / E) % 4 == 0 use the 16-byte-unit layout; where that or complex128 holds (twn_compute) the inter-pass
twiddle is the product of an entry of twA and one of twB, otherwise one entry of the n-entry table twN.

Forward bound.  Every output bin is reached from every input sample along exactly one path of the butterfly graph, and every operation on
that path multiplies the path's contribution by (1 + delta): an addition by |delta| <= u, a multiplication by a twiddle w^ with |w^ - w| <= mu
by |delta| <= mu + sqrt(2) gamma_2 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., lemma 3.5 and theorem 24.2; the packed
fma forms of wgfft.hpp's cmul are inside it).  Theorem 24.2 charges a radix-2 stage -- one twiddle multiplication and one addition -- with
eta = mu + gamma_4 (sqrt(2) + mu).  The kernels are counted the same way, per multiplication a value really passes through:

  * a line pass of fft_nstages(len, E) Stockham stages (fft_radix): the stage twiddle of every stage but the first, and inside a radix-8 or
    radix-16 butterfly one more factor (W8 or W16 constants; a radix-4 or radix-2 butterfly multiplies by +-1, +-i only, exactly);
  * the inter-pass multiplication by W_n^(k1 n2), once.

That is Lambda (`lam`).  The additions of all L = log2 n butterfly layers are paid from eta's surplus over a bare multiplication:
Lambda eta >= Lambda (mu + sqrt(2) gamma_2) + L u is checked for every shape by `shape` itself (it holds because a radix-16 butterfly has four
layers of additions and at least one multiplication).  mu is the largest absolute error of a factor as the plan forms it:

  * table entries (line tables, twA, twB, twN): sincospi in float64, rounded once to T: u for complex64 (the float64 error is below 2^-50 and is
    added), 4u for complex128 (OCML documents sincospi to 2 ulp = 4u per component);
  * the radix constants of wgfft.hpp's RadixConst: complex128 correctly rounded (u); complex64 deliberately detuned pairs whose distance from
    the exact root is computed below from the literals (1.2 u at most);
  * twn_compute plans: fl(twA twB), |w^ - w| <= 2 mu_tab + mu_tab^2 + sqrt(2) gamma_2 (1 + mu_tab)^2.

Per bin |X^_k - X_k| <= ((1 + eta)^Lambda - 1) ||x||_1, and by theorem 24.2's argument ||X^ - X||_2 <= (Lambda eta / (1 - Lambda eta)) ||X||_2;
`fwd_coeff` returns (1 + eta)^Lambda - 1 >= Lambda eta for both.  Nothing here is fitted to what a device returns.

Back through an inverse transform.  y = ifft(H fft(x)) with |H_k| = 1: forward and inverse pass cost 2 Lambda eta, the table entry tau, the scaling
by 1 / n is exact (a power of two), so ||y^ - y||_2 <= ((1 + eta)^(2 Lambda) (1 + tau) - 1) ||x||_2 (`back_coeff`); m applications in a row compound to
(1 + that)^m - 1.  tau: a host table already in T costs u (it is rounded to T before it is scaled); exp(D~ h) formed on the device costs
u (1 + max |Im D~ h|) for the product D~ h in T seen through exp(i .), 3u for rounding cos, sin and exp's result, and for the FM_PHASE tables
the phase quantum 2 pi 2^-32 / 2 (complex64; k_make_phase_table) (`tau_device`).  In the frequency domain, transforming the returned field on the
host in long double, |Y^_k - H_k X_k| <= sqrt(n) ||y^ - y||_2 by Cauchy-Schwarz: loose for rounding errors, yet orders below the |H_a - H_b| >= 1
of one misplaced entry of a unit-modulus table on an impulse (every |X_k| = 1)."""
import zlib

import numpy as np
import scipy.fft

LD, CLD = np.longdouble, np.clongdouble
C64, C128 = 0, 1
U = {C64: 2.0 ** -24, C128: 2.0 ** -53}
CDTYPE = {C64: np.complex64, C128: np.complex128}
PI_LD = LD(4) * np.arctan(LD(1))
FULL_MAX_LOG2 = 16          # the full input list runs up to here; above, the short one
PAIRS = ((8, 8), (8, 16), (16, 8), (16, 16), None)       # (SSFM_E, SSFM_EF); None: both unset


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


class Cache(dict):
    """The last results of a slow function, oldest out first, held to `limit` bytes; the arrays are handed out read-only."""

    def __init__(self, limit):
        super().__init__()
        self.limit = limit

    def get_or(self, key, make):
        if key not in self:
            v = make()
            v.setflags(write=False)
            self[key] = v
            while sum(a.nbytes for a in self.values()) > self.limit and len(self) > 1:
                self.pop(next(iter(self)))
        return self[key]


_CACHE = Cache(1 << 30)          # roots, inputs and reference spectra together (a 2^22-point long-double spectrum is 128 MiB)


# ------------------------------------------------------------------------------------------- roots of unity and the long-double transform


def roots(n):
    """w[m] = exp(-2 pi i m / n), m < n, in long double (n a multiple of 8): one octant from cos / sin, the rest by exact symmetry."""
    if n % 8:
        raise ValueError(f"roots({n}): a multiple of 8")
    return _CACHE.get_or(("roots", n), lambda: _roots(n))


def _roots(n):
    e = n // 8
    a = 2 * PI_LD * np.arange(e + 1, dtype=LD) / LD(n)
    c, s = np.cos(a), np.sin(a)
    c[e] = s[e] = np.sqrt(LD(0.5))
    re, im = np.empty(n, LD), np.empty(n, LD)
    re[: e + 1], im[: e + 1] = c, -s
    re[e: 2 * e + 1], im[e: 2 * e + 1] = s[::-1], -c[::-1]           # m = n/4 - m': cos <-> sin
    for q in (1, 2, 3):                                               # w[m + n/4] = -i w[m]
        lo, hi = q * 2 * e, (q + 1) * 2 * e
        re[lo:hi], im[lo:hi] = im[lo - 2 * e: lo].copy(), -re[lo - 2 * e: lo]
    w = np.empty(n, CLD)
    w.real, w.imag = re, im
    return w


def roots64(n):
    """roots(n) rounded to complex128: for comparisons of complex64 results, whose bounds are nine orders above that rounding."""
    return _CACHE.get_or(("roots64", n), lambda: roots(n).astype(np.complex128))


def impulse_spectrum(n, j, ld=True):
    """The spectrum of a unit impulse at j: w[(j k) % n] (ld = False: from roots64)."""
    return (roots(n) if ld else roots64(n))[(np.arange(n, dtype=np.int64) * int(j)) % n]


def ld_fft_raw(x, inverse=False):
    x = np.asarray(x).astype(CLD)
    return scipy.fft.ifft(x, axis=-1) if inverse else scipy.fft.fft(x, axis=-1)


def ld_fft(n, name):
    """The long-double spectrum of make_input(n, name), cached per (n, input)."""
    return _CACHE.get_or(("ld_fft", n, name), lambda: ld_fft_raw(make_input(n, name)))


# ------------------------------------------------------------------------------------------- plan shapes and their bounds
def ilog2(v):
    return int(v).bit_length() - 1


def fft_nstages(L, E):
    return (1 if L <= 16 else 2 if L <= 256 else 3 if L <= 4096 else 4) if E == 16 else (ilog2(L) + 2) // 3


def fft_radix(L, s, E):
    if E == 16:
        return {16: (16,), 32: (8, 4), 64: (8, 8), 128: (16, 8), 256: (16, 16), 512: (8, 8, 8), 1024: (16, 8, 8), 2048: (16, 16, 8),
                4096: (16, 16, 16), 8192: (16, 16, 16, 2)}[L][s]
    return 8 if s < ilog2(L) // 3 else 1 << (ilog2(L) % 3)


def line_mults(L, E):
    """Multiplications by a rounded factor on the worst path through one line transform, and its radices."""
    rad = [fft_radix(L, s, E) for s in range(fft_nstages(L, E))]
    assert int(np.prod(rad)) == L, (L, E, rad)
    return sum((s > 0) + (r >= 8) for s, r in enumerate(rad)), rad


def _const_err_c64():
    """Largest distance of wgfft.hpp's float32 radix constants from the roots they stand for."""
    R2D, R2U = LD(np.float32(0.7071067690849304)), LD(np.float32(0.7071068286895752))
    cA, sA = LD(np.float32(0.9238795638084412)), LD(np.float32(0.3826833665370941))
    cB, sB = LD(np.float32(0.9238795042037964)), LD(np.float32(0.38268348574638367))
    r2, c8, s8 = np.sqrt(LD(0.5)), np.cos(PI_LD / 8), np.sin(PI_LD / 8)
    return float(max(np.hypot(R2D - r2, R2U - r2), np.hypot(R2D - r2, R2D - r2), np.hypot(cA - c8, sA - s8), np.hypot(cB - c8, sB - s8)))


MU_CONST = {C64: _const_err_c64(), C128: U[C128]}
MU_TAB = {C64: U[C64] + 2.0 ** -50, C128: 4 * U[C128]}


def gamma(k, u):
    return k * u / (1 - k * u)


def shape(log2n, prec, pair=None):
    """What PlanT::init decides for a direct plan of 2^log2n points, and the bound's mu, eta, Lambda for it."""
    L = int(log2n)
    k1 = min(L // 2, 8) if L <= 20 else 9
    N1, N2 = 1 << k1, 1 << (L - k1)
    if L > 20:
        E = Ef = 16
    elif pair is None:
        E, Ef = (8, 8) if L <= 17 else ((8 if prec == C128 else 16), 16)
    else:
        E, Ef = pair
    u = U[prec]
    u16 = prec == C64 and (N1 // E) % 4 == 0 and N1 // E >= 4
    twc = u16 or prec == C128
    mt = MU_TAB[prec]
    mu_pass = 2 * mt + mt * mt + np.sqrt(2) * gamma(2, u) * (1 + mt) ** 2 if twc else mt
    mu = max(mt, MU_CONST[prec], mu_pass)
    eta = mu + gamma(4, u) * (np.sqrt(2) + mu)
    m1, r1 = line_mults(N1, E)
    m2, r2 = line_mults(N2, Ef)
    lam = m1 + m2 + 1
    assert lam * eta >= lam * (mu + np.sqrt(2) * gamma(2, u)) + L * u, (L, prec, pair)       # the additions of all L layers are covered
    return dict(log2n=L, n=1 << L, prec=prec, N1=N1, N2=N2, E=E, Ef=Ef, Q=N2 // Ef, u16=u16, twn_compute=twc, u=u, mu=float(mu), eta=float(eta),
                lam=lam, radices=(tuple(r1), tuple(r2)))


def _finish(sh, L, lam, mu):
    u = sh["u"]
    eta = mu + gamma(4, u) * (np.sqrt(2) + mu)
    assert lam * eta >= lam * (mu + np.sqrt(2) * gamma(2, u)) + L * u, sh
    sh.update(log2n=L, n=1 << L, lam=lam, mu=float(mu), eta=float(eta))
    return sh


def small_shape(log2n, prec):
    """The one-workgroup engine (k_small): ONE line of n points, 16 points per thread for complex64 rows from 4096 points and 8 otherwise; no inter-pass factor."""
    n = 1 << log2n
    E = 16 if prec == C64 and n >= 4096 else 8
    lam, rad = line_mults(n, E)
    sh = dict(prec=prec, u=U[prec], N1=1, N2=n, E=E, Ef=E, Q=n // E, u16=False, twn_compute=False, radices=((), tuple(rad)))
    return _finish(sh, log2n, lam, max(MU_TAB[prec], MU_CONST[prec]))


def split_shape(log2n, prec, log2m=20):
    """A split plan (csrc/ssfm_split.hpp): R = 2^(log2n - log2m) sub-sequences on the direct plan of 2^log2m points; each direction adds the factor
    W_n^(a q) -- the product of two float64 table entries, rounded once to T -- and a radix-R butterfly across the sub-rows (one more constant from R = 8)."""
    sh = shape(log2m, prec)
    R = 1 << (log2n - log2m)
    mu_split = 2 * MU_TAB[C128] + np.sqrt(2) * gamma(2, U[C128]) + (U[C64] if prec == C64 else 0.0)
    sh["R"] = R
    return _finish(sh, log2n, sh["lam"] + 1 + (R >= 8), max(sh["mu"], mu_split))


def fwd_coeff(sh):
    """c with |X^_k - X_k| <= c ||x||_1 and ||X^ - X||_2 <= c ||X||_2."""
    le = sh["lam"] * sh["eta"]
    return float(max((1 + sh["eta"]) ** sh["lam"] - 1, le / (1 - le)))


def tau_host(sh):
    return sh["u"]


def tau_device(sh, max_phase, phase_table=False):
    """exp(D~ h) formed on the device from an operator whose largest |Im D~ h| is max_phase."""
    t = sh["u"] * (1 + max_phase) + 3 * sh["u"]
    if phase_table and sh["prec"] == C64:
        t += np.pi * 2.0 ** -32
    return float(t)


def back_coeff(sh, tau, times=1):
    """c with ||y^ - y||_2 <= c ||x||_2 after `times` applications of ifft(H fft(.)), |H| = 1; sqrt(n) c ||x||_2 bounds every bin of fft(y^ - y)."""
    one = (1 + fwd_coeff(sh)) ** 2 * (1 + tau)
    return float(one ** times - 1)


def numpy_coeff(log2n, prec):
    """The same bound for a textbook radix-2 transform with correctly rounded twiddles (theorem 24.2 itself): what NumPy's own FFT is held to."""
    u = U[prec]
    eta = u + gamma(4, u) * (np.sqrt(2) + u)
    return float((1 + eta) ** log2n - 1)


# ------------------------------------------------------------------------------------------- inputs
def impulse_positions(sh, full=True):
    n, N1, N2 = sh["n"], sh["N1"], sh["N2"]
    if not full:
        return [1, n // 2 - 1, n - 1]
    rng = np.random.default_rng(seed_of("impulse", n))
    pos = [0, 1, N1 - 1, N1, N1 + 1, N2 - 1, N2, n // 2 - 1, n // 2, n - 1] + [int(v) for v in rng.integers(0, n, 2)]
    return list(dict.fromkeys(pos))


def tone_bins(sh, full=True):
    n = sh["n"]
    seeded = int(np.random.default_rng(seed_of("tone", n)).integers(2, n - 1))
    if not full:
        return [seeded]
    return list(dict.fromkeys([0, 1, sh["N1"], n // 2, n - 1, seeded]))


def input_names(sh, full=None):
    """The inputs of one shape by name: ('impulse', j), ('tone', bin), ('white', 0)."""
    if full is None:
        full = sh["log2n"] <= FULL_MAX_LOG2
    return [("impulse", j) for j in impulse_positions(sh, full)] + [("tone", b) for b in tone_bins(sh, full)] + [("white", 0)]


def make_input(n, name):
    """One row of n complex128 values that complex64 holds exactly."""
    return _CACHE.get_or(("input", n, name), lambda: _make_input(n, name))


def _make_input(n, name):
    kind, p = name
    if kind == "impulse":
        x = np.zeros(n, np.complex64)
        x[p] = 1
    elif kind == "tone":
        x = np.exp(2j * np.pi * ((np.arange(n, dtype=np.int64) * int(p)) % n) / n).astype(np.complex64)
    elif kind == "white":
        rng = np.random.default_rng(seed_of("white", n, p))
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    else:
        raise ValueError(name)
    return x.astype(np.complex128)


def reference(n, name):
    """The exact spectrum of make_input(n, name): the closed form for an impulse, the long-double transform of the rounded samples otherwise."""
    return impulse_spectrum(n, name[1]) if name[0] == "impulse" else ld_fft(n, name)


def batches(names, rows):
    """The inputs dealt into batches of `rows` different members (the last one filled up from the front)."""
    out = []
    for i in range(0, len(names), rows):
        b = names[i: i + rows]
        out.append(b + names[: rows - len(b)] if len(b) < rows else b)
    return out


# ------------------------------------------------------------------------------------------- comparisons
def reference64(n, name):
    """reference(n, name) rounded to complex128 (tones and white noise cached: the rounding costs more than the comparison)."""
    if name[0] == "impulse":
        return impulse_spectrum(n, name[1], ld=False)
    return _CACHE.get_or(("ref64", n, name), lambda: ld_fft(n, name).astype(np.complex128))


def forward_errors(X, name, n, coeff):
    """(per-bin measured / bound, normwise measured / bound or None) of a computed spectrum X of make_input(n, name).  A complex64 spectrum is
    compared in float64 with the reference rounded to complex128: that rounding, 2^-53 |X_k|, is below 1e-9 of the complex64 bound."""
    X = np.asarray(X)
    if X.dtype == np.complex64:
        ref = reference64(n, name)
        d = np.abs(X.astype(np.complex128) - ref)
    else:
        ref = reference(n, name)
        d = np.abs(X.astype(CLD) - ref)
    l1 = 1.0 if name[0] == "impulse" else float(np.sum(np.abs(make_input(n, name))))
    per_bin = float(d.max() / (coeff * l1))
    if name[0] == "impulse":
        return per_bin, None
    return per_bin, float(np.sqrt(np.sum(d * d)) / (coeff * np.sqrt(np.sum(np.abs(ref) ** 2))))


def unit_table(n, seed, prec):
    """H_k = exp(i theta_k), theta uniform in [-pi, pi), rounded to the plan's type; (H, theta)."""
    theta = np.random.default_rng(seed).uniform(-np.pi, np.pi, n)
    return np.exp(1j * theta).astype(CDTYPE[prec]), theta


def shift_table(n, s, prec):
    """H_k = exp(-2 pi i k s / n) from the long-double roots, rounded to the plan's type."""
    return impulse_spectrum(n, s).astype(np.complex128).astype(CDTYPE[prec])


def swap_pair(H, seed):
    """A seeded pair (a, b) of bins with |H_a - H_b| >= 1."""
    rng = np.random.default_rng(seed)
    while True:
        a, b = (int(v) for v in rng.integers(0, H.size, 2))
        if a != b and abs(complex(H[a]) - complex(H[b])) >= 1:
            return a, b


def swapped(H, pair):
    G = H.copy()
    G[pair[0]], G[pair[1]] = H[pair[1]], H[pair[0]]
    return G


def expi(theta, times=1):
    """exp(i times theta) in long double."""
    a = LD(times) * np.asarray(theta).astype(LD)
    out = np.empty(a.shape, CLD)
    out.real, out.imag = np.cos(a), np.sin(a)
    return out


def spectrum_violations(y, H, j, bound):
    """Bins k at which the long-double spectrum of the returned field y misses H_k w[(j k) % n] by more than `bound`, and the worst measured / bound."""
    n = y.size
    want = impulse_spectrum(n, j) * np.asarray(H).astype(CLD)
    d = np.abs(ld_fft_raw(y) - want)
    return np.flatnonzero(d > bound), float(d.max() / bound)


def impulse_spectrum_any(n, j):
    """exp(-2 pi i j k / n) for any n: the argument reduced exactly in integers, cos / sin in long double."""
    a = 2 * PI_LD * ((np.arange(n, dtype=np.int64) * int(j)) % n).astype(LD) / LD(n)
    out = np.empty(n, CLD)
    out.real, out.imag = np.cos(a), -np.sin(a)
    return out
