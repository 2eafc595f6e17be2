"""A reference for the zero-phase SOS filter (csrc/sos_filter.hip) that is better than float64, and the per-sample error bound the GPU
tests hold the device to.  The checker of tests/test_sos_edges_gpu.py; pinned without a GPU by tests/test_sos_numpy.py.

The reference (`filtfilt_ref`).  SciPy's sosfiltfilt -- odd extension of 3 * ntaps samples on both sides, start state zi * (first sample) in
either direction -- in np.longdouble.  The cascade's impulse response and its zero-input responses come from one short serial long-double
recursion, run until every response is below 1e-26 of its peak; a pass is a long-double overlap-add convolution (scipy.fft, blocks of a few
response lengths, so that the convolution's own noise stays LOCAL to where the input is large) plus the zero-input response of the caller's
zi * x[0].  zi is taken as given, in double, as the device takes it.  `filtfilt_serial` is the plain long-double sample loop it is checked
against.

The bound (`bound`) is a per-sample array that depends on the filter, the input and the workgroup layout only -- never on a result under test.
u = 2^-53.  Parts:

 1. SERIAL ROUNDING.  Running-error analysis of the direct-form-II-transposed step of section s,
        o  = b0 x + z0            2 operations: |d o|  <= u (2 |b0 x| + |z0|)
        z0 = b1 x - a1 o + z1     4 operations: |d z0| <= u (3 |b1 x| + 3 |a1 o| + |z1|)
        z1 = b2 x - a2 o          3 operations: |d z1| <= u (2 |b2 x| + 2 |a2 o|)
    (a product rounds once, every sum rounds the magnitude of its terms once more; a zero coefficient adds nothing).  An error of o[n], of
    z0[n - 1] or of z1[n - 2] enters the recurrence of section s as one additive term at sample n, and reaches the output through
    c_s = 1 / A_s times the sections behind s.  So |error| <= sum_s |c_s| (*) I_s, I_s[n] = |d o|[n] + |d z0|[n - 1] + |d z1|[n - 2], with
    the magnitudes taken from a float64 run.  The rounded products zi * x[0] (one rounding each) go through the absolute zero-input
    responses, the rounded odd extension 2 x[0] - x[k] (one rounding) through |h|.  The backward pass adds the same over its own input, and
    what the forward pass left goes through |h| and, by the start state zi * y1[-1], through the zero-input responses once more.
    No free factor: SciPy's float64 sosfiltfilt sits at R_SCIPY_MAX of this term alone, worst sample over every filter and input of the GPU
    module (tests/test_sos_numpy.py measures it again on every run; profiles/sos_margins.txt has each case).

 2. SEAMS (layout = (wavefronts, chunk) given).  The device computes the start state of every chunk as M^j S_g + e_c from tables of matrix
    powers (build_tables) instead of carrying it.  `_tree` runs the device's combination in float64 -- chunk sums p_c = G x (chunk products
    and sums per element), six doubling steps of the wavefront scan, the carry over the wavefronts, the group totals,
    S_g = sum_d (M^group)^d T_(g-1-d) with the start state's image, the offsets M^lane and (M^64)^wave -- and takes from every operation
    y = y0 + A v the rounding it adds,
        r = |d A| |v| + (K + 1) u (|y0| + |A| |v|)        (K products, K sums, in any order, fused or not),
    from the sum over the look-back's terms ten more roundings of the terms' magnitudes (six shuffle steps, the wavefronts, the levels).
    |d A| is the table's own error: the float64 tables built as the host builds them (products of up to 64 matrices, level on level) against
    the same products in long double, doubled, plus one rounding of every element (the host's compiler may fuse differently).
    Every value of the combination is a part of the state at ONE chunk boundary, and the tables carry it on from there as the recurrence
    would: its rounding is a state error injected at that boundary, which reaches the output through the absolute zero-input responses
    |zo_q| from that sample on -- sum_q |zo_q| (*) R_q, R_q the roundings placed at the boundaries' samples -- exactly as an injection of
    part 1 goes through |c_s|.  (It is counted for every later chunk, those that never use the value included: an upper bound.)
    No product of magnitudes is carried from level to level, so the term holds ONE factor |A| |v| / |A v| of the operation that rounds.  In
    the direct-form-II-transposed basis the two states of a narrow section nearly cancel, and that factor is the conditioning of the chunked
    recurrence: the term is 1.1 to 7 times part 1 at Wn >= 0.07, about 20 times at 0.02, some 3000 times at 0.004.
 3. The backward pass of the device starts `grid - m` samples early on copies of y1[-1] (SosPass::mv): the start state zi * y1[-1] stays put
    there only as far as the rounded zi is the steady state.  |(A^k - 1)(zi - z_ss)| |y1[-1]|, computed in long double, goes through the
    zero-input responses from the row's end.
 4. TRUNCATION.  1e-40 times the magnitude of the totals behind the look-back depth (group_start_near drops them).
 5. FLOOR.  The reference's own error: F_REF times the error unit of its block convolutions, local to the block (see F_REF, _floor_pass).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.fft as sfft
import scipy.signal as sg

LD = np.longdouble
U = 2.0 ** -53
EPS_LD = float(np.finfo(LD).eps)
WAVE = 64
TAIL = 1e-26            # the responses are cut where they are below this part of their peak
DROP = 1e-40            # group_start_near: the powers of the group map it drops are below this in every element (sos_filter_impl.inc)

# SciPy's float64 sosfiltfilt against filtfilt_ref, as a fraction of the serial term alone, worst sample over every case of
# tests/test_sos_numpy.py::test_scipy_and_the_oracle_keep_the_serial_bound (measured 0.28, order 1 at Wn = 0.3 on the ramp; the test asserts every case below 1, this figure as the
# worst, and prints each case).  Nothing is scaled by it: the bound's operation counts are its only constants.
R_SCIPY_MAX = 0.35
# The reference's floor: |filtfilt_ref - filtfilt_serial| <= F_REF * eps_ld log2(N) ||h||_2 sqrt(N) * (largest |input| within one block of the
# N-point convolution and its neighbours) per pass (_floor_pass).  Measured worst 0.63 of that unit (tests/test_sos_numpy.py::
# test_reference_against_the_serial_loop prints every case and asserts the floor); F_REF = 4 x that, rounded up, fixed before any device was looked at.
F_REF = 3.0


def _need_long_double():
    assert EPS_LD <= 2.0 ** -63, f"np.longdouble is not an 80-bit type here (eps = {EPS_LD}): sos_numpy would be no reference"


def ntaps_of(sos):
    sos = np.asarray(sos)
    return 2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))


def edge_of(sos):
    return 3 * ntaps_of(sos)


def odd_ext(x, edge):
    return np.concatenate((2 * x[..., :1] - x[..., edge:0:-1], x, 2 * x[..., -1:] - x[..., -2:-(edge + 2):-1]), axis=-1)


# ------------------------------------------------------------------------------------------------ the cascade's responses
class Responses:
    """h: the cascade's impulse response; c[s]: that of 1 / A_s and the sections behind s; zo[q]: the output after a unit start state q
    (q = 2 * section + {0, 1}); all long double, length `len` (a multiple of 256)."""


@functools.lru_cache(maxsize=64)
def _responses_cached(key):
    sos = np.frombuffer(key, np.float64).reshape(-1, 6)
    ns = sos.shape[0]
    K = 2 * ns
    ncol = 1 + ns + K
    b0, b1, b2, a1, a2 = (np.tile(sos[:, j].astype(LD)[:, None], (1, ncol)) for j in (0, 1, 2, 4, 5))
    for s in range(ns):                                   # column 1 + s: an impulse enters the recurrence of section s
        col = 1 + s
        b0[:s, col] = 1; b1[:s, col] = 0; b2[:s, col] = 0; a1[:s, col] = 0; a2[:s, col] = 0
        b0[s, col] = 1; b1[s, col] = 0; b2[s, col] = 0
    z = np.zeros((ns, 2, ncol), LD)
    for q in range(K):
        z[q // 2, q % 2, 1 + ns + q] = 1
    x0 = np.zeros(ncol, LD)
    x0[:1 + ns] = 1
    zero = np.zeros(ncol, LD)
    out, peak, n = [], np.zeros(ncol, LD), 0
    while True:
        blk = np.empty((256, ncol), LD)
        for i in range(256):
            x = x0 if n == 0 else zero
            for s in range(ns):
                xn = x
                x = b0[s] * xn + z[s, 0]
                z[s, 0] = b1[s] * xn - a1[s] * x + z[s, 1]
                z[s, 1] = b2[s] * xn - a2[s] * x
            blk[i] = x
            n += 1
        out.append(blk)
        m = np.abs(blk).max(axis=0)
        peak = np.maximum(peak, m)
        if np.all(m <= TAIL * peak) or n >= (1 << 20):
            break
    r = np.concatenate(out, axis=0)
    R = Responses()
    R.len = r.shape[0]
    R.h = r[:, 0].copy()
    R.c = [r[:, 1 + s].copy() for s in range(ns)]
    R.zo = [r[:, 1 + ns + q].copy() for q in range(K)]
    R.h_abs = np.abs(R.h).astype(np.float64)
    R.c_abs = [np.abs(c).astype(np.float64) for c in R.c]
    R.zo_abs = np.stack([np.abs(c).astype(np.float64) for c in R.zo], axis=1)        # (len, K)
    return R


def responses(sos):
    _need_long_double()
    return _responses_cached(np.ascontiguousarray(sos, np.float64).tobytes())


# ------------------------------------------------------------------------------------------------ the reference
def _conv_ld(x, h):
    """x (*) h, the first len(x) samples, in long double by overlap-add: blocks of 3 response lengths, so an FFT's noise is that of its block."""
    n, lh = x.shape[-1], h.shape[0]
    nfft = sfft.next_fast_len(4 * lh, real=True)
    blk = nfft - lh + 1
    nb = -(-n // blk)
    xp = np.zeros(nb * blk, LD)
    xp[:n] = x
    H = sfft.rfft(h, nfft)
    Y = sfft.irfft(sfft.rfft(xp.reshape(nb, blk), nfft, axis=-1) * H, nfft, axis=-1)
    y = np.zeros(nb * blk + nfft, LD)
    for b in range(nb):                                    # (nb is small: a block is thousands of samples)
        y[b * blk:b * blk + nfft] += Y[b]
    return y[:n]


def _pass_ld(R, zi, x):
    y = _conv_ld(x, R.h)
    t = min(R.len, x.shape[0])
    for q, zq in enumerate(np.asarray(zi, np.float64).reshape(-1)):
        y[:t] += R.zo[q][:t] * (LD(zq) * x[0])
    return y


def _rows(x):
    """A real or complex array of any rank as 2-D real rows (complex rows become two), and how to put a result back."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    shape = x.shape
    x2 = x.reshape(-1, shape[-1])
    if cplx:
        x2 = np.stack((x2.real, x2.imag), axis=1).reshape(-1, shape[-1])

    def back(y):
        if cplx:
            y = y.reshape(-1, 2, shape[-1])
            return (y[:, 0] + 1j * y[:, 1]).reshape(shape)
        return y.reshape(shape)
    return np.ascontiguousarray(x2, np.float64), cplx, back


def forward_ref(sos, zi, row):
    """The padded forward pass of one real row, long double (what the backward pass runs over)."""
    R = responses(sos)
    return _pass_ld(R, zi, odd_ext(row.astype(LD), edge_of(sos)))


def filtfilt_ref(sos, zi, x):
    """sosfiltfilt(sos, x, axis=-1) with the start states zi * (first sample), long double (complex inputs: complex long double)."""
    R = responses(sos)
    edge = edge_of(sos)
    x2, cplx, back = _rows(x)
    if x2.shape[-1] <= edge:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % edge)
    out = np.empty(x2.shape, LD)
    for i, row in enumerate(x2):
        y1 = _pass_ld(R, zi, odd_ext(row.astype(LD), edge))
        y2 = _pass_ld(R, zi, y1[::-1])[::-1]
        out[i] = y2[edge:-edge]
    return back(out)


def sosfilt_serial(sos, x, z):
    """The plain sample loop in long double; z: (sections, 2) start state."""
    sos = np.asarray(sos, np.float64).astype(LD)
    z = np.array(z, LD)
    y = np.empty(x.shape[0], LD)
    for n in range(x.shape[0]):
        v = LD(x[n])
        for s in range(sos.shape[0]):
            xn = v
            v = sos[s, 0] * xn + z[s, 0]
            z[s, 0] = sos[s, 1] * xn - sos[s, 4] * v + z[s, 1]
            z[s, 1] = sos[s, 2] * xn - sos[s, 5] * v
        y[n] = v
    return y


def filtfilt_serial(sos, zi, row):
    """filtfilt_ref of one real row by the serial loop (small n only)."""
    edge = edge_of(sos)
    ext = odd_ext(np.asarray(row, np.float64).astype(LD), edge)
    zl = np.asarray(zi, np.float64).astype(LD)
    y1 = sosfilt_serial(sos, ext, zl * ext[0])
    y2 = sosfilt_serial(sos, y1[::-1], zl * y1[-1])[::-1]
    return y2[edge:-edge]


def dc_gain(sos):
    """The cascade's gain at frequency 0 of the coefficients as they are (rounded), long double."""
    s = np.asarray(sos, np.float64).astype(LD)
    return np.prod((s[:, 0] + s[:, 1] + s[:, 2]) / (1 + s[:, 4] + s[:, 5]))


# ------------------------------------------------------------------------------------------------ the bound: serial term
def _posconv(k, s):
    """(k (*) s)[:len(s)] for non-negative k, s -- as an UPPER bound: the kernel's tail below 1e-22 of its sum is replaced by its mass times
    max(s); the direct sum where it is cheap, else overlap-add in float64 with 1e-14 sum(k) max(s) for that transform's noise."""
    tot = float(k.sum())
    if tot == 0.0 or not s.any():
        return np.zeros_like(s)
    tail = np.cumsum(k[::-1])[::-1]
    keep = max(1, int(np.searchsorted(-tail, -1e-22 * tot)))
    dropped = float(tail[keep]) if keep < k.shape[0] else 0.0
    kk = k[:keep]
    smax = float(s.max())
    if kk.shape[0] * s.shape[0] <= 2e8:
        y = np.convolve(s, kk)[:s.shape[0]]
    else:
        y = np.maximum(sg.oaconvolve(s, kk)[:s.shape[0]], 0.0) + 1e-14 * tot * smax
    return y + dropped * smax


def _local_max(a, w):
    """max of a over [n - w, n + w], by blocks of w (an upper bound of it: three blocks)."""
    n = a.shape[0]
    nb = -(-n // w)
    p = np.zeros(nb * w)
    p[:n] = a
    bm = p.reshape(nb, w).max(axis=1)
    e = np.concatenate(([0.0], bm, [0.0]))
    return np.repeat(np.maximum(np.maximum(e[:-2], e[1:-1]), e[2:]), w)[:n]


def _serial_pass(sos, zi, R, seq, e_in, e_first):
    """Error bound of one pass over the real float64 sequence `seq` started from zi * seq[0]: its own roundings, the input's error bound
    e_in through |h|, and the start state's, |zi| e_first + u |zi seq[0]|, through the zero-input responses."""
    m = seq.shape[0]
    zi = np.asarray(zi, np.float64).reshape(-1, 2)
    err = _posconv(R.h_abs, e_in)
    xs = seq
    for s in range(sos.shape[0]):
        b0, b1, b2, _, a1, a2 = sos[s]
        o = sg.sosfilt(sos[s:s + 1], xs, zi=(zi[s] * seq[0])[None, :])[0]
        zp0 = o - b0 * xs                                       # z0[n - 1]
        zp1 = np.empty(m)                                       # z1[n - 1]
        zp1[:-1] = zp0[1:] - b1 * xs[:-1] + a1 * o[:-1]
        zp1[-1] = zp1[-2] if m > 1 else 0.0
        zp1[0] = zi[s, 1] * seq[0]
        e_o = U * (2 * np.abs(b0 * xs) + np.abs(zp0))
        e_z0 = U * (3 * np.abs(b1 * xs) + 3 * np.abs(a1 * o) + np.abs(zp1))
        e_z1 = U * (2 * np.abs(b2 * xs) + 2 * np.abs(a2 * o))
        inj = e_o.copy()
        inj[1:] += e_z0[:-1]
        inj[2:] += e_z1[:-2]
        err += _posconv(R.c_abs[s], inj)
        xs = o
    t = min(R.len, m)
    e_state = np.abs(zi.reshape(-1)) * e_first + U * np.abs(zi.reshape(-1) * seq[0])
    err[:t] += R.zo_abs[:t] @ e_state
    return err


def _floor_pass(R, zi, seq_abs, f_in):
    """The reference's own error in one pass: the input's through |h|; the block convolution's, F_REF times eps log2(N) ||h||_2 ||x||_2 of
    an N-point transform, the block's ||x||_2 taken as sqrt(N) times the largest input of the block and its neighbours; four roundings of the
    start state's zero-input response."""
    w = sfft.next_fast_len(4 * R.len, real=True)
    unit = EPS_LD * math.log2(w) * float(np.sqrt((R.h_abs ** 2).sum())) * math.sqrt(w)
    f = _posconv(R.h_abs, f_in) + F_REF * unit * _local_max(seq_abs, w)
    t = min(R.len, seq_abs.shape[0])
    f[:t] += 4 * EPS_LD * (R.zo_abs[:t] @ np.abs(np.asarray(zi, np.float64).reshape(-1))) * seq_abs[0]
    return f


# ------------------------------------------------------------------------------------------------ the bound: the device's seams
def _step_cols(sos, z, x, dt):
    """One sample of the cascade on column vectors (z: (NS, 2, cols)), in the host's operation order."""
    for s in range(sos.shape[0]):
        xn = x
        x = sos[s, 0] * xn + z[s, 0]
        z[s, 0] = sos[s, 1] * xn - sos[s, 4] * x + z[s, 1]
        z[s, 1] = sos[s, 2] * xn - sos[s, 5] * x
    return x


def _tables(sos, W, L, dt):
    """build_tables (csrc/sos_tables.hpp) in the type dt: the one-sample map A, P[level][j] = (M_level)^j, j = 0..64, and G."""
    ns = sos.shape[0]
    K = 2 * ns
    c = np.asarray(sos, np.float64).astype(dt)
    z = np.zeros((ns, 2, K), dt)
    for q in range(K):
        z[q // 2, q % 2, q] = 1
    A = None
    for i in range(L):
        _step_cols(c, z, np.zeros(K, dt), dt)
        if i == 0:
            A = z.reshape(K, K).copy()
    M = z.reshape(K, K).copy()                             # M[r, q]: state r after L steps from unit state q
    G = np.zeros((K, L), dt)
    z = np.zeros((ns, 2, 1), dt)
    for i in range(L):
        _step_cols(c, z, np.full(1, 1 if i == 0 else 0, dt), dt)
        G[:, L - 1 - i] = z.reshape(K)
    P = np.zeros((3, WAVE + 1, K, K), dt)
    for level in range(3):
        P[level, 0] = np.eye(K, dtype=dt)
        for j in range(WAVE):
            P[level, j + 1] = M @ P[level, j]
        M = P[level, WAVE].copy()
        if level == 0:
            Aw = M.copy()
            for _ in range(1, W):
                Aw = M @ Aw
            M = Aw
    return A, P, G


class Tables:
    pass


@functools.lru_cache(maxsize=64)
def _device_tables_cached(key, W, L):
    sos = np.frombuffer(key, np.float64).reshape(-1, 6)
    _, P64, G64 = _tables(sos, W, L, np.float64)
    A_ld, P_ld, G_ld = _tables(sos, W, L, LD)
    T = Tables()
    T.K = 2 * sos.shape[0]
    T.P, T.G = P64, G64
    T.dP = 2 * np.abs(P64 - P_ld).astype(np.float64) + U * np.abs(P64)
    T.dG = 2 * np.abs(G64 - G_ld).astype(np.float64) + U * np.abs(G64)
    T.A_ld = A_ld
    # the look-back depth as the host finds it (csrc/sos_route.hpp look_of_group_powers): 1 + the last d <= 64 whose (M^group)^d has an element at or above 1e-40
    T.look = 1
    for d in range(1, WAVE + 1):
        if not np.abs(P64[1, d]).max() < DROP:
            T.look = d + 1
    # the group powers by distance d = 64 a + b: value, magnitude as the device multiplies it (|P2[a]| |P1[b]|), error
    val, mag, err = [], [], []
    for d in range(WAVE * WAVE):
        a, b = divmod(d, WAVE)
        if a == 0:
            v, g, e = P64[1, b], np.abs(P64[1, b]), T.dP[1, b]
        else:
            v = P64[2, a] @ P64[1, b]
            g = np.abs(P64[2, a]) @ np.abs(P64[1, b])
            e = np.abs(P64[2, a]) @ T.dP[1, b] + T.dP[2, a] @ np.abs(P64[1, b]) + (T.K + 1) * U * g
        if d > 0 and g.max() < 1e-280:
            break
        val.append(v); mag.append(g); err.append(e)
    T.Pg, T.Pg_abs, T.Pg_err = np.array(val), np.array(mag), np.array(err)
    return T


def device_tables(sos, W, L):
    return _device_tables_cached(np.ascontiguousarray(sos, np.float64).tobytes(), int(W), int(L))


def look_of(sos, W, L):
    """SosLink::look as the host computes it for this filter and layout (before the dispatcher's `<= kNear` test)."""
    return device_tables(sos, W, L).look


def _mv(A, dA, v, y0=None):
    """(y, r) of y = y0 + A v on the last axis; r = |d A| |v| + (K + 1) u (|y0| + |A| |v|): the rounding this operation adds."""
    K = A.shape[-1]
    Aa, va = np.abs(A), np.abs(v)
    if A.ndim == 2:
        y, mag, r = v @ A.T, va @ Aa.T, va @ dA.T
    else:                                                  # one matrix per element of the axis before the last
        y, mag = np.einsum("...lrq,...lq->...lr", A, v), np.einsum("...lrq,...lq->...lr", Aa, va)
        r = np.einsum("...lrq,...lq->...lr", dA, va)
    if y0 is not None:
        y, mag = y + y0, mag + np.abs(y0)
    return y, r + (K + 1) * U * mag


def _tree(T, W, L, grid_seq, s0):
    """R[b], (chunks + 1, K): the roundings the device's combination adds to the state AT chunk boundary b (the start of chunk b), for the
    real sequence `grid_seq` over the whole chunk grid (a multiple of 64 W L samples) started from the state s0.  Every value of the
    combination is a part of the state at one boundary -- a chunk sum and a scan step's partial sum at the end of their chunk, a carry at
    the end of its wavefront, a group's start state at the group's start, a chunk's start state at that chunk's start -- and the tables carry
    it on from there as the recurrence itself would (to first order), so what it adds reaches the output as a state error at that boundary."""
    K = T.K
    group = WAVE * W
    nch = grid_seq.shape[0] // L
    ng = nch // group
    X = grid_seq.reshape(nch, L)
    R = np.zeros((nch + 1, K))
    p, r = _mv(T.G, T.dG, X)                               # chunk sums: L fused multiply-adds per element
    p, r = p.reshape(ng, W, WAVE, K), r.reshape(ng, W, WAVE, K)
    for k in range(6):                                     # the wavefront's scan: x_l += M^(2^k) x_(l - 2^k)
        d = 1 << k
        up = np.zeros_like(p)
        up[..., d:, :] = p[..., :-d, :]
        p, rk = _mv(T.P[0, d], T.dP[0, d], up, p)
        rk[..., :d, :] = 0                                 # (the first 2^k lanes add nothing)
        r = r + rk
    R[1:] += r.reshape(nch, K)                             # ... at the end of their chunk
    ex = np.zeros_like(p)
    ex[..., 1:, :] = p[..., :-1, :]
    tot = p[..., -1, :]                                    # (ng, W, K)
    M64, dM64 = T.P[0, WAVE], T.dP[0, WAVE]
    ws = np.zeros((ng, W + 1, K))
    wave_end = (np.arange(ng)[:, None] * W + np.arange(1, W + 1)[None, :]) * WAVE          # boundary behind wavefront w of group g
    for w in range(W):                                     # ws_(w+1) = M^64 ws_w + tot_w
        ws[:, w + 1], rw = _mv(M64, dM64, ws[:, w], tot[:, w])
        if w:
            R[wave_end[:, w]] += rw
    Ml, dMl = T.P[0, :WAVE], T.dP[0, :WAVE]                # (64, K, K)
    wsl = np.broadcast_to(ws[:, :W, None, :], (ng, W, WAVE, K))
    e_c, r_c = _mv(Ml, dMl, wsl, ex)
    if W == 1:
        r_c = np.zeros_like(r_c)                           # (one wavefront: no carry to add)
    # the group's start state: V = [s0, T_0, T_1, ...], S_g = sum_d Pg[d] V[g - d]
    V = np.concatenate((s0[None, :], ws[:-1, W]), axis=0)
    S, rS, mag = np.zeros((ng, K)), np.zeros((ng, K)), np.zeros((ng, K))
    rS[0] += U * np.abs(s0)                                # the products zi * x[0]
    for d in range(min(ng, T.Pg.shape[0])):
        v = V[:ng - d]
        S[d:] += v @ T.Pg[d].T
        m_d = np.abs(v) @ T.Pg_abs[d].T
        mag[d:] += m_d
        rS[d:] += np.abs(v) @ T.Pg_err[d].T + (K + 1) * U * m_d
    rS += 10 * U * mag
    # what the near look-back drops: the totals at distance >= look, times 1e-40 (every element of their power is below that)
    norm1 = np.concatenate(([0.0], np.cumsum(np.abs(V).sum(axis=1))))
    rS += DROP * norm1[np.maximum(np.arange(ng) + 1 - T.look, 0)][:, None]
    R[np.arange(ng) * group] += rS
    # the chunk's start state: (M^64)^wave S_g, then M^lane, plus e_c
    Sw = np.zeros((ng, W, K))
    Sw[:, 0] = S
    for w in range(1, W):
        Sw[:, w], rw = _mv(M64, dM64, Sw[:, w - 1])
        R[wave_end[:, w - 1]] += rw
    Swl = np.broadcast_to(Sw[:, :, None, :], (ng, W, WAVE, K))
    _, r_s = _mv(Ml, dMl, Swl, e_c)
    R[:nch] += (r_c + r_s).reshape(nch, K)
    return R


def _seam_pass(T, R, W, L, seq, s0, lead):
    """The seam term of one pass, per sample of `seq`: the pass runs over `lead` copies of seq[0] and then seq, on a grid of whole groups.
    A state error at boundary b shows from sample b L on through the zero-input responses -- in the chunks that do not use the value it
    came with, too: an upper bound."""
    group_len = WAVE * W * L
    total = lead + seq.shape[0]
    ng = -(-total // group_len)
    grid = np.zeros(ng * group_len)
    grid[:lead] = seq[0]
    grid[lead:total] = seq
    Rb = _tree(T, W, L, grid, s0)[:-1]                     # (chunks, K)
    out = np.zeros(grid.shape[0])
    for q in range(T.K):
        inj = np.zeros(grid.shape[0])
        inj[::L] = Rb[:, q]
        out += _posconv(R.zo_abs[:, q], inj)
    return out[lead:total]


def _ld_solve(Mx, b):
    """Gaussian elimination with partial pivoting in long double (K <= 8)."""
    Mx, b = Mx.copy(), b.copy()
    n = b.shape[0]
    for i in range(n):
        p = i + int(np.argmax(np.abs(Mx[i:, i])))
        if p != i:
            Mx[[i, p]] = Mx[[p, i]]
            b[[i, p]] = b[[p, i]]
        for r in range(i + 1, n):
            f = Mx[r, i] / Mx[i, i]
            Mx[r, i:] -= f * Mx[i, i:]
            b[r] -= f * b[i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - Mx[i, i + 1:] @ x[i + 1:]) / Mx[i, i]
    return x


def _early_start(sos, zi, T, lead):
    """|(A^lead - 1)(zi - z_ss)|: how far a state zi * v has moved after `lead` samples of the constant v, per unit of |v|."""
    K = T.K
    A = T.A_ld
    c = np.asarray(sos, np.float64).astype(LD)
    z = np.zeros((sos.shape[0], 2, 1), LD)
    _step_cols(c, z, np.ones(1, LD), LD)
    Bv = z.reshape(K)                                      # the state one unit sample leaves behind
    z_ss = _ld_solve(np.eye(K, dtype=LD) - A, Bv)
    Ak, base, k = np.eye(K, dtype=LD), A.copy(), int(lead)
    while k:
        if k & 1:
            Ak = base @ Ak
        base = base @ base
        k >>= 1
    d = np.asarray(zi, np.float64).reshape(-1).astype(LD) - z_ss
    return np.abs((Ak - np.eye(K, dtype=LD)) @ d).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the bound
def bound_row(sos, zi, row, layout=None, parts=False):
    """The per-sample bound for one real row.  layout = None: the serial term and the floor (what SciPy is held to);
    layout = (wavefronts, chunk): with the device's seam terms for that layout."""
    sos = np.ascontiguousarray(sos, np.float64)
    R = responses(sos)
    edge = edge_of(sos)
    n = row.shape[0]
    ext = odd_ext(row, edge)
    m = ext.shape[0]
    y1 = forward_ref(sos, zi, row).astype(np.float64)
    e_ext = np.zeros(m)
    e_ext[:edge] = U * np.abs(ext[:edge])
    e_ext[-edge:] = U * np.abs(ext[-edge:])
    ef = _serial_pass(sos, zi, R, ext, e_ext, 0.0)
    ff = _floor_pass(R, zi, np.abs(ext), np.zeros(m))
    seam = np.zeros(n)
    if layout is not None:
        W, L = layout
        T = device_tables(sos, W, L)
        zf = np.asarray(zi, np.float64).reshape(-1)
        ef = ef + _seam_pass(T, R, W, L, ext, zf * ext[0], 0)
    r = y1[::-1].copy()
    eb = _serial_pass(sos, zi, R, r, ef[::-1].copy(), float(ef[-1]))
    fb = _floor_pass(R, zi, np.abs(r), ff[::-1].copy())
    if layout is not None:
        group_len = WAVE * W * L
        lead = -(-m // group_len) * group_len - m
        sb = _seam_pass(T, R, W, L, r, zf * r[0], lead)
        t = min(R.len, m)
        sb[:t] += R.zo_abs[:t] @ (_early_start(sos, zi, T, lead) * abs(r[0]))
        eb = eb + sb
    total = (eb + fb)[::-1][edge:-edge]
    if parts:
        return total, fb[::-1][edge:-edge]
    return total


def bound(sos, zi, x, layout=None):
    """The per-sample bound in the shape of x; for complex x it holds for the real and for the imaginary part (a complex array whose parts are the two bounds)."""
    x2, cplx, back = _rows(x)
    return back(np.stack([bound_row(sos, zi, row, layout) for row in x2]))


def compare(got, sos, zi, x, layout=None):
    """(worst measured / bound, its flat index among the real rows' samples, the ratios as real rows) of `got` against filtfilt_ref."""
    ref = filtfilt_ref(sos, zi, x)
    g2, _, _ = _rows(np.asarray(got))
    r2, _, _ = _rows_ld(ref)
    x2, _, _ = _rows(x)
    ratio = np.empty(x2.shape)
    for i, row in enumerate(x2):
        d = np.abs(g2[i].astype(LD) - r2[i]).astype(np.float64)
        b = bound_row(sos, zi, row, layout)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio[i] = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), k, ratio


def _rows_ld(y):
    y = np.asarray(y)
    shape = y.shape
    y2 = y.reshape(-1, shape[-1])
    if np.iscomplexobj(y):
        y2 = np.stack((y2.real, y2.imag), axis=1).reshape(-1, shape[-1])
    return y2, None, None


# ------------------------------------------------------------------------------------------------ the inputs of both test modules
KINDS = ("walk", "const", "big", "tone", "impulse", "step", "ramp")
WNS = (0.3, 0.07, 0.02, 0.004)


def make_input(kind, n, seed, group_len=768, pos=None):
    """One real row.  walk: the suite's random walk; const; big: 1e6 + unit noise; tone: 0.9 Nyquist (the output is 1e-10 of it and less);
    impulse: a 1 at `pos`; step: 1e12 + unit noise up to one group before the end, unit noise behind; ramp."""
    rng = np.random.default_rng(seed)
    if kind == "walk":
        return rng.standard_normal(n).cumsum() * 0.05 + rng.standard_normal(n)
    if kind == "const":
        return np.full(n, 0.7353)
    if kind == "big":
        return 1e6 + rng.standard_normal(n)
    if kind == "tone":
        return np.cos(0.9 * np.pi * np.arange(n))
    if kind == "impulse":
        x = np.zeros(n)
        x[n // 2 if pos is None else pos] = 1.0
        return x
    if kind == "step":
        x = rng.standard_normal(n)
        x[:max(n - group_len, 1)] += 1e12
        return x
    if kind == "ramp":
        return 0.01 * np.arange(n) - 3.0
    raise ValueError(kind)


def planted_fault(sos, zi, row, seam, rel=1e-12):
    """(faulty result, the backward positions it touches) -- filtfilt_ref rounded to float64, plus what a backward-pass state that is off by
    `rel` of its magnitude at backward sample `seam` (of the padded row) adds: the zero-input response of that error from there on."""
    R = responses(sos)
    edge = edge_of(sos)
    y1 = forward_ref(sos, zi, row).astype(np.float64)
    r = y1[::-1].copy()
    m = r.shape[0]
    zf = sg.sosfilt(np.asarray(sos), r[:seam], zi=np.asarray(zi).reshape(-1, 2) * r[0])[1]          # the state in front of sample `seam`
    d = rel * np.abs(zf).reshape(-1)
    t = min(R.len, m - seam)
    add = np.zeros(m)
    add[seam:seam + t] = (np.stack([np.asarray(c[:t], np.float64) for c in R.zo], axis=1) @ d)
    good = filtfilt_ref(sos, zi, row).astype(np.float64)
    return good + add[::-1][edge:-edge], (m - 1 - seam) - edge          # ... and the output index of backward sample `seam`
