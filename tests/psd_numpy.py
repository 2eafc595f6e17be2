"""A reference for Welch's PSD that is better than float64: SciPy's layout (periodic Hann window, ``noverlap = nperseg // 2``, trailing samples
dropped, ``scaling='spectrum'``, mean over the segments, fftshift) restated in ``np.longdouble`` with a direct DFT, and the per-bin error
bound the GPU tests hold the device to.  The checker of tests/test_psd_edges_gpu.py; pinned without a GPU by tests/test_psd_numpy.py.

The bound.  An L-point float64 transform leaves every bin of segment s within ``d_s = K u T ||v_s||_2`` of the exact value (v_s: the windowed
segment, u = 2^-53, T: the depth of the route's sums), so ``| |X + e|^2 - |X|^2 | <= 2 |X| d + d^2`` and the averaged spectrum is within

    bound_k = K u T A_k + (K u T)^2 B,      A_k = scale / nseg * sum_s 2 |X_sk| ||v_s||_2,      B = scale / nseg * sum_s ||v_s||_2^2.

T = log2 L for the line kernel (route 1), sqrt(P) for the direct DFT (route 2: a sum of P terms, by Cauchy-Schwarz), 3 log2 M for the chirp-z
route (three M-point transforms with the chirp products).
"""
from __future__ import annotations

import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# K: SciPy's own float64 Welch (pocketfft), measured against welch_ref on every input of tests/test_psd_edges_gpu.py, sits at
# r = max_k |p_scipy - p_ref| / (u T A_k) <= R_SCIPY_MAX (tools/psd_bound_survey.py, no GPU involved; profiles/psd_margins.txt has every
# case's r).  p_scipy is SciPy's float64 spectrum of every segment averaged in long double: its float64 mean over tens of thousands of segments
# adds up to thousands of u of its own on equal terms, which says nothing about a transform.  The largest r, 8.13, is the tone's own bin at
# L = 8192 in one segment (there u T A_k is a third of one rounding of p_k, so r counts the roundings of the square and the scale); white noise
# and the tone's floor sit at 0.1 ... 2.  K = ceil(4 r_max): the factor 4 is for a transform that is not pocketfft's -- another radix plan,
# twiddles rounded into a table -- and was fixed before the device was looked at.  A device ratio above 1 is a finding, not a reason to raise K.
R_SCIPY_MAX = 8.133
K = 33


def _need_long_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble is not an 80-bit type here (eps = {np.finfo(LD).eps}): psd_numpy would be no reference"


def _pi():
    return LD(4) * np.arctan(LD(1))


def hann_ld(L: int) -> np.ndarray:
    """scipy.signal.get_window('hann', L) (periodic) in long double; [1] for L = 1."""
    if L == 1:
        return np.ones(1, LD)
    return LD(0.5) - LD(0.5) * np.cos(2 * _pi() * np.arange(L, dtype=LD) / LD(L))


def layout(n: int, L: int):
    """(step, nseg) of SciPy's segmenting."""
    step = L - L // 2
    return step, (n - L // 2) // step


def shifted_bins(L: int) -> np.ndarray:
    """Natural DFT bin of every fftshifted output position: out[o] = in[(o + L - L // 2) % L]."""
    return (np.arange(L) + (L - L // 2)) % L


def _segments(x, L):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    rows, n = x.shape
    step, nseg = layout(n, L)
    assert nseg >= 1
    idx = (np.arange(nseg) * step)[:, None] + np.arange(L)[None, :]
    return x, rows, nseg, idx


def welch_ref(x, nperseg: int, bins=None):
    """(p, A, B) of the rows of ``x`` ((n,) or (rows, n), real or complex, any float type; widened exactly to long double):

    p[r, j]  the Welch estimate at fftshifted output position ``bins[j]`` (every position when ``bins`` is None), long double;
    A[r, j]  scale / nseg * sum_s 2 |X_sk| ||v_s||_2 at the same positions;
    B[r]     scale / nseg * sum_s ||v_s||_2^2.

    A direct DFT: the twiddle of term (k, m) is exp(-2 pi i q / L) with q = k m mod L reduced in integers, so the cosine and sine only ever
    see L distinct arguments in [0, 2 pi).  The result for a subset of bins is the same arithmetic as the full result's, bit for bit.  A 1-D
    input gives 1-D p and A and a scalar B."""
    _need_long_double()
    L = int(nperseg)
    one_d = np.asarray(x).ndim == 1
    x, rows, nseg, idx = _segments(x, L)
    cplx = np.iscomplexobj(x)
    pos = np.arange(L) if bins is None else np.asarray(bins, dtype=np.int64)
    k = shifted_bins(L)[pos]
    w = hann_ld(L)
    scale = LD(1) / w.sum() ** 2
    ang = 2 * _pi() * np.arange(L, dtype=LD) / LD(L)
    ctab, stab = np.cos(ang), np.sin(ang)
    q = (np.arange(L, dtype=np.int64)[:, None] * k[None, :].astype(np.int64)) % L          # (L, nbins), exact in int64
    Cq, Sq = ctab[q], stab[q]                                                              # exp(-i a) = cos a - i sin a
    p = np.zeros((rows, pos.size), LD)
    A = np.zeros((rows, pos.size), LD)
    B = np.zeros(rows, LD)

    def one_row(r):
        vr = x[r].real.astype(LD)[idx] * w                                                 # (nseg, L)
        re, im = vr @ Cq, -(vr @ Sq)
        nrm2 = (vr * vr).sum(axis=1)
        if cplx:
            vi = x[r].imag.astype(LD)[idx] * w
            re, im = re + vi @ Sq, im + vi @ Cq
            nrm2 = nrm2 + (vi * vi).sum(axis=1)
        mag2 = re * re + im * im
        p[r] = mag2.sum(axis=0) * (scale / nseg)
        A[r] = (2 * np.sqrt(mag2) * np.sqrt(nrm2)[:, None]).sum(axis=0) * (scale / nseg)
        B[r] = nrm2.sum() * (scale / nseg)

    if rows == 1:
        one_row(0)
    else:                                                  # NumPy's long-double matmul has no BLAS behind it and releases the GIL: a thread per row
        with ThreadPoolExecutor(max_workers=min(rows, 4)) as pool:
            list(pool.map(one_row, range(rows)))
    if one_d:
        return p[0], A[0], B[0]
    return p, A, B


def welch_terms64(x, nperseg: int):
    """(A, B) of welch_ref for EVERY bin from NumPy's float64 FFT: the shape factors of the bound where a long-double DFT of every bin is out of
    reach (L >= 2048).  They enter the bound as factors, so their own float64 error (1e-16 of ||v||) does not matter; where a bin's exact
    |X| is zero (a constant input) use welch_ref."""
    L = int(nperseg)
    one_d = np.asarray(x).ndim == 1
    x, rows, nseg, idx = _segments(x, L)
    w = hann_ld(L).astype(np.float64)
    scale = 1.0 / float(hann_ld(L).sum()) ** 2
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    A = np.zeros((rows, L))
    B = np.zeros(rows)
    blk = max(1, (1 << 22) // (nseg * L))                          # rows per block: about 64 MiB of complex128 segments at a time
    for r0 in range(0, rows, blk):
        v = x[r0:r0 + blk][:, idx] * w                             # (rows, nseg, L)
        X = np.fft.fftshift(np.fft.fft(v, axis=-1), axes=-1)
        nrm = np.sqrt((np.abs(v) ** 2).sum(axis=2))
        A[r0:r0 + blk] = (2 * np.abs(X) * nrm[:, :, None]).sum(axis=1) * (scale / nseg)
        B[r0:r0 + blk] = (nrm ** 2).sum(axis=1) * (scale / nseg)
    if one_d:
        return A[0], B[0]
    return A, B


def depth(nperseg: int) -> float:
    """T of the bound for the route ``nperseg`` takes (opticomlib_amd.utils._welch_layout)."""
    L = int(nperseg)
    if L < 16:
        return math.sqrt(L)
    if L <= 8192 and L & (L - 1) == 0:
        return float(L.bit_length() - 1)
    M = 1 << max(8, (2 * L - 2).bit_length())                       # the chirp-z plan's line
    return 3.0 * (M.bit_length() - 1)


def bound(A, B, T: float, k: float = K):
    """bound_k = K u T A_k + (K u T)^2 B, float64, broadcast over rows."""
    e = k * U * T
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    return e * A + e * e * (B[..., None] if A.ndim > B.ndim else B)


def scipy_r(p_scipy, p_ref, A, T: float, B=None) -> float:
    """max_k |p_scipy - p_ref| / (u T A_k): SciPy's own distance from the reference in the unit of the bound's first-order term, over the bins
    where that term is the larger one (A_k > u T B; with no B: A_k > 0).  Where the exact |X| vanishes (the empty bins of a constant) the
    ratio would divide a second-order error by nothing and says nothing about K."""
    d = np.abs(np.asarray(p_scipy, dtype=LD) - p_ref)
    A = np.asarray(A, dtype=LD)
    floor = 0 if B is None else LD(U) * LD(T) * np.asarray(B, dtype=LD)
    ok = A > (floor[..., None] if np.ndim(floor) and A.ndim > np.ndim(floor) else floor)
    if not ok.any():
        return 0.0
    return float(np.max(d[ok] / (LD(U) * LD(T) * A[ok])))


def f32_neighbours(got, ref):
    """True per element where ``got`` (float32) is np.float32(ref) or one of its two neighbours; elements whose reference is not a normal
    float32 pass (they are not judged)."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    r = np.asarray(ref, dtype=np.float64).astype(np.float32)
    normal = np.isfinite(r) & (np.abs(r) >= np.finfo(np.float32).tiny)
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    return ~normal | (got == r) | (got == lo) | (got == hi)
