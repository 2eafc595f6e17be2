"""The adaptive step rule h = phi_max / (|gamma| max|A|^2), restated in NumPy, with the fields and the faulty variants the step-size tests are built on
(tests/test_adaptive_steps_cpu.py, tests/test_adaptive_steps_gpu.py).  Test infrastructure.

RESTATEMENT.  adaptive_truth(a, dt, kw, precision) -> (z, A, where).  complex64: the problem tests/diag/fuzz_cases.truth_adaptive_f64 states -- float32
coefficients, the float32 step rule and float32 z accumulation, evaluated on the maximum of the FLOAT64 field, every transform, exponential and rotation in
float64.  complex128: the rule and z in float64, as oracle.ssfm_numpy.fiber_c128.  where[k] is the (row, sample) that holds the maximum after step k
(where[0]: of the input).  Any number of rows.

FIELDS.  Sums of Gaussian pulses (row, centre sample, width in samples, peak power in W, carrier offset in rad / sample, chirp) on a background that is
exactly zero, placed circularly.  A run on such a field is equivariant under a circular shift and under moving the pulse to another row, so the truth of a
static case is computed once per (n, precision) and serves every position and row (asserted on the CPU: the z logs differ by exactly 0.0).

THE FOUR CASES (sampling grid: 512 GHz, dt = 1.953125 ps; all with phi_max = 0.002, gamma = 1.3 / (W km); the figures are the CPU's, complex64 mode,
the same at every n to the digits shown -- tests/test_adaptive_steps_cpu.py asserts the conditions they stand for at every size the GPU file uses)
  decay    one pulse, width 16, 12 mW, alpha = 3.0 dB/km, SMF dispersion (beta_2 = -21.7, beta_3 = 0.13), length 0.70 km.
           5 steps, h = 0.1282 0.1401 0.1543 0.1717 0.1057 (the last one clamped: 0.547 of the 0.1932 the rule gave); the peak falls by 8.5 ... 11.2 % per
           step (7.0 % over the clamped one).  A slot that is never cleared, or a running maximum, gives steps that do not grow.
  growth   one pulse, width 12, 8 mW, chirp -2 (the field's phase is + chirp d^2 / (2 width^2); +2 broadens under beta_2 = -150, -2 compresses), alpha = 0,
           length 0.75 km.  5 steps, h = 0.1923 0.1724 0.1551 0.1402 0.0899 (clamped: 0.705 of 0.1275); the peak rises by 10.0 ... 11.6 % per step (6.4 %
           over the clamped one).  A stale or late maximum gives steps that are too long.
  travel   beta_2 = -500, alpha = 3.0.  Row 0: width 12, 12 mW, carrier offset 1.2 rad / sample, centred 40 samples before the end of the row: its peak walks
           20 ... 45 samples per step, crosses the wrap-around to sample 2 and goes on through several tiles, dispersing.  Row 1: width min(100, n / 16),
           10.8 mW (11.3 mW below width 50, where the pulse disperses itself), offset -0.6, centred at n / 2 + 5: it holds the maximum from the fourth step on,
           so three free steps follow the hand-over.  Length 1.5 km.  n = 4096: 8 steps, where = (0,4056) (0,4076) (0,2) (0,27) (1,2005) (1,1988) (1,1968)
           (1,1944) (1,1935); last step 0.311 of the rule's (0.168 at n = 256).  One-row shapes run row 0's pulse alone over 1.0 km: 6 steps, where = ...
           (0,56) (0,92) (0,137), last step 0.566 of the rule's.
  dark     all zeros: the rule gives h = inf, clamped to the length: one step, z = [0, L], the output exactly zero.

MUTANTS.  Variants of the restatement's maximum, by name (MUTANTS): what a reduction that is wrong in one of the ways the engines could be wrong would compute.
  row0         row 0 only                                  drop_tail    without the last C samples of every row
  drop_first   without sample 0                            drop_subseq  without the samples = r mod R (one sub-sequence of a split plan)
  padding      with a non-zero value past n counted        running      never reset: the maximum of all steps so far
  late1        the maximum of one step earlier             late2        of two steps earlier (the ping-pong slot of the wrong parity)
  f16          |A|^2 rounded to float16 before the maximum (any reduced-precision copy of the power)
  signed_gamma gamma instead of |gamma| (shows in a backward run)
Which case kills which mutant: the table in tests/test_adaptive_steps_cpu.py, filled from that file's own run."""
import functools

import numpy as np

from oracle import ssfm_numpy as orc

F32 = np.float32
C64, C128 = 0, 1
DT = 1.0 / (16 * 32e9)                  # workloads.BENCH_GV
U32, U64 = 2.0 ** -24, 2.0 ** -53
CUT = 6.0                               # a pulse is exactly zero beyond CUT widths from its centre (there: 1.5e-8 of its peak amplitude)
MUTANTS = ("row0", "drop_tail", "drop_first", "drop_subseq", "padding", "running", "late1", "late2", "f16", "signed_gamma")
MAX_STEPS = 64                          # a run the mutants send nowhere (signed_gamma: z falls) stops here


# ----------------------------------------------------------------------------------------------------------------- fields
def pulse_field(n, rows, pulses):
    """(rows, n) complex64: the sum of the Gaussian pulses (row, centre, width, peak power, carrier offset, chirp); every other sample exactly 0."""
    a = np.zeros((rows, n), np.complex128)
    k = np.arange(n)
    for row, centre, width, power, omega, chirp in pulses:
        d = ((k - int(centre) + n // 2) % n - n // 2).astype(np.float64)            # signed circular distance: a shift of the centre is np.roll, exactly
        u = d / float(width)
        v = np.sqrt(power) * np.exp(-0.5 * u * u) * np.exp(1j * (omega * d + 0.5 * chirp * u * u))
        v[np.abs(u) > CUT] = 0.0
        a[row] += v
    return a.astype(np.complex64)


DECAY = dict(kw=dict(length=0.70, alpha=3.0, beta_2=-21.7, beta_3=0.13, gamma=1.3, phi_max=0.002), pulse=(16, 12e-3, 0.0, 0.0))
GROWTH = dict(kw=dict(length=0.75, alpha=0.0, beta_2=-150.0, beta_3=0.0, gamma=1.3, phi_max=0.002), pulse=(12, 8e-3, 0.0, -2.0))
TRAVEL_KW = dict(length=1.5, alpha=3.0, beta_2=-500.0, beta_3=0.0, gamma=1.3, phi_max=0.002)


def travel_kw(rows):
    """(one row: the walking pulse alone, over 1.0 km -- at 1.5 its last step would be 0.94 of the rule's)"""
    return dict(TRAVEL_KW, length=1.5 if rows >= 2 else 1.0)

DARK_KW = dict(length=0.70, alpha=3.0, beta_2=-21.7, beta_3=0.13, gamma=1.3, phi_max=0.002)
STATIC = {"decay": DECAY, "growth": GROWTH}


def static_field(case, n, rows, row, centre):
    """The decay / growth pulse centred on sample `centre` of row `row`, the other rows dark."""
    return pulse_field(n, rows, [(row, centre) + STATIC[case]["pulse"]])


def travel_field(n, rows):
    w1 = min(100, n // 16)
    pulses = [(0, n - 40, 12, 12e-3, 1.2, 0.0)]
    if rows >= 2:
        pulses.append((1, n // 2 + 5, w1, 11.3e-3 if w1 < 50 else 10.8e-3, -0.6, 0.0))
    return pulse_field(n, rows, pulses)


# ----------------------------------------------------------------------------------------------------------------- the restatement
def _peak(P, mutant, hist, opt):
    """(the value the rule divides by, flat index of the true maximum).  hist: the true maxima of the earlier evaluations, the input's first."""
    idx = int(np.argmax(P))
    true = P.flat[idx]
    n = P.shape[-1]
    if mutant is None or mutant == "signed_gamma":
        v = true
    elif mutant == "row0":
        v = P[0].max()
    elif mutant == "drop_tail":
        v = P[:, : n - opt.get("C", 16)].max()
    elif mutant == "drop_first":
        v = P[:, 1:].max()
    elif mutant == "drop_subseq":
        v = P[:, np.arange(n) % opt.get("R", 2) != opt.get("r", 1)].max()
    elif mutant == "padding":
        v = max(true, opt.get("pad", 0.8) * (hist[0] if hist else true))             # a padding value of 0.8 of the input's peak power
    elif mutant == "running":
        v = max([true] + hist)
    elif mutant == "late1":
        v = hist[-1] if hist else true
    elif mutant == "late2":
        v = hist[-2] if len(hist) >= 2 else (hist[0] if hist else true)
    elif mutant == "f16":
        v = np.float64(P.astype(np.float16).max())
    else:
        raise ValueError(mutant)
    return v, idx


def adaptive_truth(a, dt, kw, precision=C64, mutant=None, info=None, **opt):
    """(z float64 (S + 1,), A complex128 (rows, n), where [(row, sample)] * (S + 1)) -- see the module's docstring.  `mutant`: one of MUTANTS, with its
    parameters C / R, r / pad in `opt`.  `info`, a dict, receives 'h_free' (the rule's step before the clamp, per step) and 'peak' (the true maximum at every
    evaluation)."""
    a = np.atleast_2d(np.asarray(a))
    rows, n = a.shape
    A = a.astype(np.complex64).astype(np.complex128)
    al, b2, b3 = kw.get("alpha", 0.0), kw.get("beta_2", 0.0), kw.get("beta_3", 0.0)
    if precision == C64:
        D = orc.linear_operator_c64(n, dt, al, b2, b3)
        g_r, phi, L = F32(kw.get("gamma", 0.0)), F32(kw.get("phi_max", 0.01)), F32(kw["length"])
        rt = F32
        lin_of = lambda h: np.exp((D * h).astype(np.complex64).astype(np.complex128))
    else:
        D = orc.linear_operator_c128(n, dt, al, b2, b3)
        g_r, phi, L = np.float64(kw.get("gamma", 0.0)), np.float64(kw.get("phi_max", 0.01)), np.float64(kw["length"])
        rt = np.float64
        lin_of = lambda h: np.exp(D * h)
    g = np.float64(g_r)
    g_rule = g_r if mutant == "signed_gamma" else np.abs(g_r)
    hist, peaks, free, where, zs = [], [], [], [], [0.0]

    def rule(A_, z_):
        P = np.abs(A_) ** 2
        v, idx = _peak(P, mutant, hist, opt)
        hist.append(P.flat[idx])
        peaks.append(float(P.flat[idx]))
        where.append((idx // n, idx % n))
        with np.errstate(divide="ignore", over="ignore"):
            hf = rt(phi / (g_rule * rt(v)))
        free.append(float(hf))
        return rt(min(hf, rt(L - z_)))

    z = rt(0)
    h = rule(A, z)
    while z < L and len(zs) <= opt.get("max_steps", MAX_STEPS):
        z = rt(z + h)
        hh = np.float64(rt(h / 2))
        lin = lin_of(h)
        rot = np.exp(1j * g * (np.abs(A) ** 2) * hh)
        A = A * rot
        A = np.fft.ifft(np.fft.fft(A, axis=-1) * lin, axis=-1)
        A = A * rot
        zs.append(float(z))
        h = rule(A, z)
    if info is not None:
        info.update(h_free=free[: len(zs) - 1], peak=peaks)
    return np.array(zs), A, where


@functools.lru_cache(maxsize=None)
def static_truth(case, n, precision, backward=False):
    """The truth of a static case, once per (n, precision): the pulse centred on sample 0 of a single row.  (z, A, where, info)"""
    kw = dict(STATIC[case]["kw"])
    if backward:
        kw["gamma"] = -kw["gamma"]
    info = {}
    z, A, where = adaptive_truth(static_field(case, n, 1, 0, 0), DT, kw, precision, info=info)
    z.flags.writeable = A.flags.writeable = False
    return z, A, where, info


@functools.lru_cache(maxsize=None)
def travel_truth(n, rows, precision):
    info = {}
    z, A, where = adaptive_truth(travel_field(n, min(rows, 2)), DT, travel_kw(rows), precision, info=info)
    z.flags.writeable = A.flags.writeable = False
    return z, A, where, info


def shifted(A, rows, row, centre):
    """The end field of static_truth moved to (row, centre) of a field of `rows` rows."""
    out = np.zeros((rows, A.shape[-1]), A.dtype)
    out[row] = np.roll(A[0], centre)
    return out


# ----------------------------------------------------------------------------------------------------------------- bounds
def z_distance(z, zt):
    """|z[k] - zt[k]| / zt[k] for k >= 1 (index 0 of the result is k = 1)."""
    z, zt = np.asarray(z, np.float64), np.asarray(zt, np.float64)
    return np.abs(z[1:] - zt[1:]) / zt[1:]


def z_bounds(steps, precision, oracle_off=0.0, tol_c128=1e-10):
    """The bound on z_distance per k = 1 ... steps.  z[1] is a pure function of the input: 5 roundings of the plan's real type (three in re^2 + im^2, two in the
    rule).  complex64, k >= 2: 4 x max(oracle_off, (5 + k) 2^-24) -- k 2^-24 is the float32 accumulation of z, oracle_off the distance of the reference's own
    complex64 run from the restatement, 4 the ratio the project's field bound (2e-5) keeps over the reference's noise floor (5e-6).  complex128: 2 TOL_C128
    (the maximum is 1-Lipschitz in the field and h is proportional to 1 / |A|^2)."""
    k = np.arange(1, steps + 1, dtype=np.float64)
    if precision == C64:
        b = 4.0 * np.maximum(oracle_off, (5.0 + k) * U32)
        b[0] = 5.0 * U32
    else:
        b = np.full(steps, 2.0 * tol_c128)
        b[0] = 5.0 * U64
    return b


def oracle_off(a, dt, kw, zt):
    """The relative z distance of the reference's own complex64 run (oracle.ssfm_numpy.fiber_c64) from the restatement, and its step count."""
    a = np.asarray(a)
    zr, _ = orc.fiber_c64(a[0] if a.shape[0] == 1 else a, dt, return_steps=True, **kw)
    if len(zr) != len(zt):
        return np.inf, len(zr) - 1
    return float(z_distance(zr, zt).max()), len(zr) - 1


# ----------------------------------------------------------------------------------------------------------------- the shapes the GPU file runs
# engine -> (knobs pinned at plan creation, [(precision, n, rows)]).  The smallest shapes that still reach each reduction (csrc/ssfm_route.hpp).
KNOBS = ("SSFM_E", "SSFM_EF", "SSFM_EF_FLY", "SSFM_SMALL", "SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_MEDIUM_SPLIT", "SSFM_ADAPT_FUSED", "SSFM_FORCE_FLY", "SSFM_PHASE_TABLE",
         "SSFM_SPLIT_ABOVE", "SSFM_SPLIT_LOG2M", "SSFM_LANES", "SSFM_FUSED_PATIENCE_TICKS", "SSFM_CHIRP_SMALL", "SSFM_CHIRP_HALF", "SSFM_CHIRP_LOOP")
BOTH = (C64, C128)
ENGINES = {
    "small_adaptive": (dict(SSFM_SMALL=1), [(p, 256, 1) for p in BOTH] + [(p, 256, 2) for p in BOTH] + [(p, 2048, 2) for p in BOTH] + [(C64, 4096, 1)]),
    "adaptive_3_launches": (dict(SSFM_SMALL=0, SSFM_ADAPT_FUSED=0, SSFM_MEDIUM_ADAPT=0), [(p, 1 << k, 2) for k in (8, 10, 14) for p in BOTH]),
    "adaptive_fused": (dict(SSFM_ADAPT_FUSED=1, SSFM_MEDIUM_ADAPT=0), [(p, n, r) for n, r in ((1 << 14, 1), (1 << 14, 2), (1 << 17, 1)) for p in BOTH]
                       + [(C64, 1 << 18, 2), (C64, 1 << 20, 2)]),
    "medium_adaptive": (dict(SSFM_ADAPT_FUSED=1, SSFM_MEDIUM=1, SSFM_MEDIUM_ADAPT=1), [(C64, 1 << 12, 2), (C64, 1 << 13, 1), (C64, 1 << 14, 4), (C64, 1 << 17, 1)]),
    "split_adaptive": (dict(SSFM_SPLIT_ABOVE=20), [(C64, 1 << 21, 1), (C64, 1 << 21, 2), (C128, 1 << 21, 1)]),
}
# the chirp-z lines (any length): line -> (knobs, precision of the caller, [n]); two rows each
CHIRP_LINES = {
    "chirp_small_c64": (dict(SSFM_CHIRP_SMALL=1, SSFM_SMALL=1), C64, [1000, 2048]),
    "chirp_medium_c64": (dict(SSFM_MEDIUM=1, SSFM_MEDIUM_ADAPT=1, SSFM_ADAPT_FUSED=1), C64, [2049, 65536]),
    "chirp_long_c64": (dict(), C64, [65537]),               # the complex128 plan's line of a complex64 caller: complex64 values between float64 passes from 2^18 points of line
    "chirp_line_c128": (dict(SSFM_CHIRP_SMALL=0), C128, [1000]),
}
SIZES = sorted({(n, r) for _, shapes in ENGINES.values() for _, n, r in shapes} | {(n, 2) for _, _, ns in CHIRP_LINES.values() for n in ns})


@functools.lru_cache(maxsize=None)
def case_oracle_off(case, n, rows):
    """oracle_off of a case at a size: (relative z distance of the reference's complex64 run from the restatement, its step count).  Static cases: one row (equivariance)."""
    if case in STATIC:
        return oracle_off(static_field(case, n, 1, 0, 0), DT, STATIC[case]["kw"], static_truth(case, n, C64)[0])
    rows = min(rows, 2)
    return oracle_off(travel_field(n, rows), DT, travel_kw(rows), travel_truth(n, rows, C64)[0])


def clear_caches():
    """Drop the cached truths (a few hundred MiB once the 2^20 and 2^21 rows have run)."""
    for f in (static_truth, travel_truth, case_oracle_off):
        f.cache_clear()
