"""The coherent QAM receiver restated in NumPy float64 (opticomlib_amd/coherent.py, csrc/coherent.hip): the square Gray-mapped constellation, the
decisions, the blind phase search with its unwrap, the quarter-turn alignment and the error vector magnitude.  The yardstick of test_coherent_cpu.py
and test_coherent_gpu.py; it shares no code with the package.  Test infrastructure.

The window sums are direct: every s[k, b] is the sum of its own terms d[j, b] in ascending j (the outer loop runs over the offset j - k, so all k
take their j-th term in the same pass; for one k that is the plain loop over j).  Besides the results, `bps` returns what says whether an exact
comparison of integers with another float64 implementation is fair: each symbol's gap -- the relative distance between its two smallest sums -- and
the smallest distance of any rotated component, in units of a, to a decision boundary."""
import math

import numpy as np

ORDERS = (4, 16, 64, 256)


def bits_per_symbol(M):
    return {4: 2, 16: 4, 64: 6, 256: 8}[M]


def side(M):
    return {4: 2, 16: 4, 64: 8, 256: 16}[M]


def half_spacing(M):
    """a: the levels are a (2 g - (L - 1)); unit mean power over the M points."""
    return 1.0 / math.sqrt(2.0 * (M - 1) / 3.0)


def gray_decode(c):
    c = np.array(c, dtype=np.int64)
    s = c >> 1
    while np.any(s):
        c ^= s
        s >>= 1
    return c


def gray_encode(g):
    g = np.asarray(g, dtype=np.int64)
    return g ^ (g >> 1)


def _to_int(b):
    """rows of bits, MSB first -> integers"""
    v = np.zeros(b.shape[0], dtype=np.int64)
    for col in range(b.shape[1]):
        v = (v << 1) | (b[:, col] != 0)
    return v


def encode(bits, M):
    """bits (n k,) -> symbols (n,) complex128"""
    k, L, a = bits_per_symbol(M), side(M), half_spacing(M)
    b = np.asarray(bits).reshape(-1, k)
    gi, gq = gray_decode(_to_int(b[:, : k // 2])), gray_decode(_to_int(b[:, k // 2:]))
    return (a * (2 * gi - (L - 1)).astype(np.float64)) + 1j * (a * (2 * gq - (L - 1)).astype(np.float64))


def level(x, M):
    """decision of real components: clip(floor(x / (2 a) + L / 2), 0, L - 1)"""
    L, a = side(M), half_spacing(M)
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) / (2.0 * a) + L // 2), 0, L - 1).astype(np.int64)


def dec(z, M):
    """the constellation point of the two component decisions"""
    L, a = side(M), half_spacing(M)
    z = np.asarray(z, dtype=np.complex128)
    return a * (2 * level(z.real, M) - (L - 1)).astype(np.float64) + 1j * (a * (2 * level(z.imag, M) - (L - 1)).astype(np.float64))


def decode(z, M):
    """symbols (n,) -> bits (n k,) uint8"""
    k = bits_per_symbol(M)
    z = np.asarray(z, dtype=np.complex128)
    ci, cq = gray_encode(level(z.real, M)), gray_encode(level(z.imag, M))
    out = np.zeros((z.size, k), dtype=np.uint8)
    for b in range(k // 2):
        out[:, b] = (ci >> (k // 2 - 1 - b)) & 1
        out[:, k // 2 + b] = (cq >> (k // 2 - 1 - b)) & 1
    return out.ravel()


def constellation(M):
    k = bits_per_symbol(M)
    words = np.arange(M)
    bits = ((words[:, None] >> np.arange(k - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    return encode(bits.ravel(), M), bits


def boundary_distance(x, M):
    """distance of real components to the nearest decision boundary 2 a m, |m| <= L / 2 - 1, in units of a"""
    L, a = side(M), half_spacing(M)
    m = np.arange(-(L // 2 - 1), L // 2) * (2.0 * a)
    return np.min(np.abs(np.asarray(x, dtype=np.float64)[..., None] - m), axis=-1) / a


def phase_step(B):
    return np.pi / (2 * B)


def phase_table(B):
    """exp(-i phi_b), phi_b = (b - B / 2) pi / (2 B)"""
    return np.exp(-1j * ((np.arange(B) - B / 2) * phase_step(B)))


def window(k, W, n):
    """[lo, hi): the window of symbol k truncated at both ends of the row"""
    return max(0, k - W), min(n - 1, k + W) + 1


def jumps(bhat, B):
    """jump_k = -1 if 2 (b_k - b_(k-1)) > B, +1 if < -B, else 0; jump_0 = 0"""
    bhat = np.asarray(bhat, dtype=np.int64)
    d = np.diff(bhat, prepend=bhat[:1])
    return np.where(2 * d > B, -1, np.where(2 * d < -B, 1, 0)).astype(np.int64)


def unwrap(bhat, B):
    """u_k = b_k + B n_k, n_k the running sum of the jumps"""
    return np.asarray(bhat, dtype=np.int64) + B * np.cumsum(jumps(bhat, B))


def scale_of(y):
    """what brings a record to unit mean power"""
    y = np.asarray(y, dtype=np.complex128)
    return 1.0 / math.sqrt(float(np.mean(y.real * y.real + y.imag * y.imag)))


def window_sums(d, W):
    """s[k, b] = sum of d[j, b], max(0, k - W) <= j <= min(n - 1, k + W), each in ascending j"""
    n = d.shape[0]
    s = np.zeros_like(d)
    for off in range(-W, W + 1):
        lo, hi = max(0, -off), min(n, n - off)              # the k whose j = k + off lies in the row
        if lo < hi:
            s[lo:hi] += d[lo + off: hi + off]
    return s


def bps(y, M, B, W):
    """Blind phase search of one row y (n,) complex128 (already scaled).  Returns a dict: bhat, index (u), phase, symbols, sums, gap (n,), margin."""
    y = np.asarray(y, dtype=np.complex128)
    assert y.ndim == 1 and y.size >= 1 and B % 2 == 0 and 2 <= B <= 64 and 0 <= W <= 256
    r = y[:, None] * phase_table(B)[None, :]
    e = r - dec(r, M)
    d = e.real * e.real + e.imag * e.imag
    s = window_sums(d, W)
    bhat = np.argmin(s, axis=1).astype(np.int64)
    two = np.sort(s, axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    u = unwrap(bhat, B)
    phase = (u - B // 2).astype(np.float64) * phase_step(B)
    z = y * np.exp(-1j * phase)
    margin = min(float(boundary_distance(r.real, M).min()), float(boundary_distance(r.imag, M).min()),
                 float(boundary_distance(z.real, M).min()), float(boundary_distance(z.imag, M).min()))
    return {"bhat": bhat, "index": u.astype(np.int32), "phase": phase, "symbols": z, "sums": s, "gap": gap, "margin": margin}


def quarter_turns(z, ref):
    """q = argmax_t Re(i^-t sum z conj(ref)), t = 0 ... 3, the first on ties"""
    c = np.sum(np.asarray(z, dtype=np.complex128) * np.conj(ref))
    return int(np.argmax([(c * (-1j) ** t).real for t in range(4)]))


def turn(z, q):
    z = np.asarray(z, dtype=np.complex128)
    return [z, z.imag - 1j * z.real, -z, -z.imag + 1j * z.real][q % 4]


def evm(z, ref):
    e = np.asarray(z, dtype=np.complex128) - ref
    return math.sqrt(float(np.sum(e.real * e.real + e.imag * e.imag)) / float(np.sum(np.asarray(ref).real ** 2 + np.asarray(ref).imag ** 2)))


def receive(field, sps, M, B, W, instant=None, ref=None):
    """The whole receiver on one row of a field: x[instant::sps], unit mean power, BPS, the optional alignment, the decisions."""
    instant = sps // 2 if instant is None else instant
    x = np.asarray(field)[instant::sps].astype(np.complex128)
    y = x * scale_of(x)
    out = bps(y, M, B, W)
    z, q = out["symbols"], None
    if ref is not None:
        q = quarter_turns(z, ref)
        z = turn(z, q)
    out.update(symbols=z, quarter_turns=q, bits=decode(z, M), evm=evm(z, ref if ref is not None else dec(z, M)), scale=scale_of(x))
    return out


def noisy_record(n, M, snr_db, seed, lw=1e-4, ramp=3.0):
    """A seeded test record: n random symbols, Wiener phase noise of variance `lw` per symbol plus a linear ramp of `ramp` rad over the record,
    white Gaussian noise at `snr_db`.  Returns (y, symbols, bits, theta)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n * bits_per_symbol(M)).astype(np.uint8)
    s = encode(bits, M)
    theta = np.cumsum(rng.standard_normal(n) * math.sqrt(lw)) + np.linspace(0.0, ramp, n)
    sigma = math.sqrt(10 ** (-snr_db / 10) / 2)
    y = s * np.exp(1j * theta) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return y, s, bits, theta
