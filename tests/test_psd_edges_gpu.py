"""Welch's PSD (csrc/psd.hip, opticomlib_amd/utils.py) held bin by bin to a float64 error bound, at every route, workgroup split and chunk seam.

References: SciPy's float64 Welch on the same (widened) values (its per-segment spectra, averaged in long double: see Ref), every bin, at
2 x bound (both sides carry an error), and the long-double
restatement tests/psd_numpy.py at 1 x bound -- every bin up to L = 1024; from 2048 on, the 16 bins around the tone and 240 seeded ones.
bound_k = K u T A_k + (K u T)^2 B (psd_numpy's docstring; K was fixed from SciPy's own distance, not from the device's).  Inputs: `white`
noise, and `tone`: a unit exponential exactly on bin L // 8 over white noise of amplitude 1e-6, whose floor, twelve orders below the peak, is what
a peak-relative test cannot see.  complex64 inputs are judged twice: the float64 result of the same kernels (utils._welch_device with
out_f32 = False) against the bound, and get_psd's float32 result, which must be np.float32(reference) or a neighbour (the device rounds a float64
result once).  complex128 inputs are the complex64 values widened, so the two share a reference.

Every comparison records SciPy's r = max_k |p_scipy - p_ref| / (u T A_k) and the device's worst measured / bound through tests/margins.py
(digest: profiles/psd_margins.txt)."""
import os
import re
import zlib

import numpy as np
import pytest
import scipy.signal as sg

import margins
import psd_numpy as pn
import opticomlib_amd as oa
from opticomlib_amd import _lib, utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POW2 = tuple(1 << m for m in range(4, 14))
KINDS = ("white", "tone")
DOMAINS = ("real", "complex")
WELCH_MAX_NSEG = 50000      # scipy.signal.welch itself is a yardstick up to here (see Ref)
DTYPES = {"real": (np.float64,), "complex": (np.complex64, np.complex128)}


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


# ----------------------------------------------------------------------------------------------- the device and SciPy
def device_psd(x, L):
    """get_psd's estimate of a host array (float32 for complex64 input, float64 otherwise)."""
    return oa.get_psd(x, 1.0, L)[1]


def device_psd_f64(x, L):
    """The float64 estimate of the same kernels for any input type (what get_psd rounds to float32 for a complex64 input)."""
    from opticomlib_amd.devices import default_device
    x = np.ascontiguousarray(x)
    dev = int(default_device())
    rows = int(np.prod(x.shape[:-1])) if x.ndim > 1 else 1
    d = _lib.DeviceArray.from_host(x, device=dev)
    return utils._welch_device(d, rows, x.shape[-1], x.shape[-1], L, False, dev).reshape(x.shape[:-1] + (L,))


def widen(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def scipy_psd(x, L):
    with np.errstate(all="ignore"):
        p = sg.welch(widen(x), fs=1.0, nperseg=L, scaling="spectrum", return_onesided=False, detrend=False)[1]
    return np.fft.fftshift(p, axes=-1)


def scipy_psd_exact_mean(x, L):
    """SciPy's float64 spectrum of every segment (the same helper Welch averages), averaged in long double.  K is measured on this: it is for
    the transform, window, square and scale; SciPy's float64 mean over tens of thousands of segments adds an error of its own order of
    summation (up to thousands of u on equal terms), which is no yardstick for the device's fixed sliced order."""
    with np.errstate(all="ignore"):
        s = sg.spectrogram(widen(x), fs=1.0, window="hann", nperseg=L, noverlap=L // 2, detrend=False, return_onesided=False,
                           scaling="spectrum", mode="psd")[2]
    return np.fft.fftshift(s.astype(np.longdouble).mean(axis=-1), axes=-1)


# ----------------------------------------------------------------------------------------------- inputs
def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def make_input(kind, domain, rows, n, L, seed):
    """(rows, n) float64 or complex128 values; the complex ones are exactly representable in complex64."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n))
    if domain == "complex":
        x = x + 1j * rng.standard_normal((rows, n))
    if kind == "tone":
        a = 2 * np.pi * ((np.arange(n) * (L // 8)) % L) / L
        x = 1e-6 * x + (np.exp(1j * a) if domain == "complex" else np.cos(a))
    return x.astype(np.complex64).astype(np.complex128) if domain == "complex" else x


def length(nseg, L, extra=0):
    """Samples holding exactly nseg segments of L, plus `extra` (< step) trailing ones that must be ignored."""
    step = L - L // 2
    assert 0 <= extra < max(step, 1)
    return L // 2 + nseg * step + extra


def subset(L):
    """Output positions compared with the long-double reference: every bin up to 1024; above, 16 around the tone and 240 seeded ones."""
    if L <= 1024:
        return np.arange(L)
    tone = (L // 8 + L // 2) % L
    near = (tone + np.arange(-8, 8)) % L
    rest = np.setdiff1d(np.arange(L), near)
    return np.sort(np.concatenate([near, np.random.default_rng(L).choice(rest, size=240, replace=False)]))


class Ref:
    """The references of one input: long double on `bins`, SciPy on every bin, and the bound's factors on every bin."""

    def __init__(self, x, L, bins=None, ref=True, survey_bins=0):
        self.L, self.T = L, pn.depth(L)
        self.bins = np.arange(L) if bins is None else bins
        # the SciPy side: its float64 spectrum of every segment, averaged in long double.  scipy.signal.welch's own float64 mean is the same
        # figure up to its order of summation, which on 70 000 near-equal segments is thousands of u off (r = 2032 at P = 3, against K = 33):
        # an error of the yardstick's, far outside the "both sides within bound" that the factor 2 stands for
        # scipy.signal.welch itself is compared as well wherever its mean is harmless: up to WELCH_MAX_NSEG segments its r stays below 12
        # (recorded as `sg.welch r`), within the premise; only route 2's 70 000-segment inputs are beyond
        self.ps = scipy_psd_exact_mean(x, L).astype(np.float64)
        self.pw = scipy_psd(x, L)
        self.welch_ok = pn.layout(np.asarray(x).shape[-1], L)[1] <= WELCH_MAX_NSEG
        one_d = np.asarray(x).ndim == 1
        if not ref and survey_bins:                                # (tools/psd_bound_survey.py: SciPy's r for the SciPy-only inputs too)
            ref, self.bins = True, np.sort(np.random.default_rng(L).choice(L, size=min(L, survey_bins if L <= 1 << 16 else 4), replace=False))
        if ref:
            self.p, self.A, self.B = pn.welch_ref(x, L, bins=self.bins)
            self.r = pn.scipy_r(self.ps[..., self.bins], self.p, self.A, self.T, self.B)
            self.rw = pn.scipy_r(self.pw[..., self.bins], self.p, self.A, self.T, self.B)
        else:
            self.p = self.A = None
            self.r = self.rw = None
        if ref and self.bins.size == L:
            self.A_all, self.B_all = self.A.astype(np.float64), np.asarray(self.B, dtype=np.float64)
        else:
            self.A_all, self.B_all = pn.welch_terms64(x, L)
        if one_d:
            self.B_all = np.asarray(self.B_all)

    def rows(self, sl):
        """The same references for a slice of the rows."""
        o = object.__new__(Ref)
        o.L, o.T, o.bins, o.r, o.rw, o.welch_ok = self.L, self.T, self.bins, self.r, self.rw, self.welch_ok
        o.ps, o.pw, o.A_all, o.B_all = self.ps[sl], self.pw[sl], self.A_all[sl], self.B_all[sl]
        o.p, o.A, o.B = (None, None, None) if self.p is None else (self.p[sl], self.A[sl], self.B[sl])
        return o


def _ratio(d, b):
    d, b = np.asarray(d, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
    return float(np.max(q))


def judge(what, got, ref):
    """Hold `got` to the references of `ref`: float64 against SciPy at 2 x bound on every bin and the long-double reference at bound on its
    bins; float32 by the neighbour rule against both.  Records the figures before it asserts."""
    got = np.asarray(got)
    assert got.shape == ref.ps.shape, (what, got.shape, ref.ps.shape)
    survey = os.environ.get("SSFM_MARGINS_ONLY") == "1"            # (tests/margins.py: a survey run records every margin and fails nothing)
    if ref.r is not None:
        margins.record(f"{what} scipy r (bound column: K)", None, ref.r, pn.K)
        margins.record(f"{what} sg.welch r{'' if ref.welch_ok else ' beyond WELCH_MAX_NSEG'} (bound column: K)", None, ref.rw, pn.K)
    if got.dtype == np.float32:
        ok = pn.f32_neighbours(got, ref.ps) & pn.f32_neighbours(got, ref.pw)           # (float32: both SciPy figures are exact enough)
        assert survey or ok.all(), (what, "float32 against SciPy", int((~ok).sum()))
        if ref.p is not None:
            ok = pn.f32_neighbours(got[..., ref.bins], ref.p)
            assert survey or ok.all(), (what, "float32 against the long-double reference", int((~ok).sum()))
        return
    assert got.dtype == np.float64
    b_all = pn.bound(ref.A_all, ref.B_all, ref.T)
    rs = _ratio(np.abs(got - ref.ps), 2 * b_all)
    margins.record(f"{what} device / SciPy [|d| / (2 bound_k)]", None, rs, 1.0)
    rw = None
    if ref.welch_ok:
        rw = _ratio(np.abs(got - ref.pw), 2 * b_all)
        margins.record(f"{what} device / sg.welch [|d| / (2 bound_k)]", None, rw, 1.0)
    rr = None
    if ref.p is not None:
        b = pn.bound(ref.A, ref.B, ref.T)
        rr = _ratio(np.abs(got[..., ref.bins].astype(np.longdouble) - ref.p).astype(np.float64), b)
        margins.record(f"{what} device / long double [|d| / bound_k]", None, rr, 1.0)
    assert survey or rs <= 1.0, (what, "against SciPy at 2 x bound", rs)
    assert survey or rw is None or rw <= 1.0, (what, "against scipy.signal.welch at 2 x bound", rw)
    assert survey or rr is None or rr <= 1.0, (what, "against the long-double reference at bound", rr)


def run_dtype(what, x, L, ref, dtype):
    """One input through get_psd in `dtype` (and, for complex64, through the float64 form of the same kernels)."""
    xd = x.astype(dtype)
    name = np.dtype(dtype).name
    got = device_psd(xd, L)
    assert got.dtype == (np.float32 if dtype == np.complex64 else np.float64)
    judge(f"{what} {name}", got, ref)
    if dtype == np.complex64:
        judge(f"{what} {name} (float64 result)", device_psd_f64(xd, L), ref)


# ----------------------------------------------------------------------------------------------- route 1: the workgroup geometry
def welch_lines(L):
    """csrc/psd.hip welch_lines: lines of L / E threads (E = 16 points per thread at 8192, else 8) sharing a 256-thread workgroup."""
    q = L // (16 if L == 8192 else 8)
    return 1 if q >= 256 else 256 // q


def target_groups():
    src = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "psd.hip")).read()
    return int(re.search(r"constexpr int64_t kTargetGroups = (\d+);", src).group(1))


def groups(rows, nseg, least):
    """csrc/psd.hip per_group, restated: (segments per workgroup by the target alone, the spw in use, G)."""
    by_target = -(-rows * nseg // target_groups())
    spw = min(max(by_target, least), nseg)
    G = -(-nseg // spw)
    return by_target, -(-nseg // G), G


def nsegs_of(lines):
    return sorted({s for s in (1, lines - 1, lines, lines + 1, 2 * lines, 2 * lines + 1, 5 * lines + 3) if s > 0})


def run_route1(L, kind, domain):
    lines = welch_lines(L)
    assert utils._welch_layout(length(1, L), L)["route"] == 1
    bins = subset(L)
    for nseg in nsegs_of(lines):
        n0 = length(nseg, L)
        base = make_input(kind, domain, 3, n0, L, seed_of("r1", L, kind, domain, nseg))
        ref3 = Ref(base, L, bins)
        for rows in (1, 3):
            _, spw, G = groups(rows, nseg, 2 * lines)
            assert (G > 1) == (nseg > 2 * lines), (L, nseg, rows, G)          # the split cases really split (and the last group is short
            if nseg == 2 * lines + 1:                                          #  or a round is partly live)
                assert G == 2 and (nseg % spw != 0 or spw % lines != 0)
            ref = ref3 if rows == 3 else ref3.rows(slice(0, 1))
            for extra in (0, L // 2 - 1):
                x = np.empty((rows, n0 + extra), base.dtype)
                x[:, :n0] = base[:rows]
                x[:, n0:] = 1e30 if rows == 3 else -3.0                        # trailing samples: dropped, whatever they hold
                assert utils._welch_layout(n0 + extra, L)["nseg"] == nseg
                for dtype in DTYPES[domain]:
                    run_dtype(f"route 1 L={L} {kind} n={n0 + extra} ", x, L, ref, dtype)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", POW2)
def test_route1_every_line_length_and_split(L, kind, domain):
    """nseg around LINES and 2 LINES (one group, a round with idle lines, G > 1 with a short last group), rows 1 and 3, with and without
    trailing samples (1e30 in the three-row variant)."""
    run_route1(L, kind, domain)


BIG_SPLITS = ((1024, 2, 4099), (64, 3, 40001))


def run_route1_target(L, rows, nseg, survey_bins=0):
    by_target, spw, G = groups(rows, nseg, 2 * welch_lines(L))
    assert by_target > 2 * welch_lines(L) and spw == -(-nseg // G) and G > 1 and nseg % spw != 0      # spw from the group target, short last group
    x = make_input("white", "complex", rows, length(nseg, L), L, seed_of("target", L)).astype(np.complex64)
    ref = Ref(x, L, ref=False, survey_bins=survey_bins)
    judge(f"route 1 L={L} spw by target complex64 n={x.shape[1]} ", device_psd(x, L), ref)
    judge(f"route 1 L={L} spw by target complex64 (float64 result) n={x.shape[1]} ", device_psd_f64(x, L), ref)


@pytest.mark.parametrize("L,rows,nseg", BIG_SPLITS)
def test_route1_segments_per_group_from_the_target(L, rows, nseg):
    """Enough segments that the ~1024-workgroup target, not the two-rounds minimum, sets the segments per workgroup.  SciPy only, at 2 x bound
    (and the float32 result by the neighbour rule)."""
    run_route1_target(L, rows, nseg)


# ----------------------------------------------------------------------------------------------- route 2: the direct DFT
ROUTE2_NSEG = (1, 255, 256, 257, 513, 70000)


def run_route2(P):
    assert utils._welch_layout(length(1, P), P)["route"] == 2
    for nseg in ROUTE2_NSEG:
        # the long case (274 workgroups a row) alternates its kind with P; the short ones take both
        for kind in (KINDS if nseg < 70000 else (KINDS[P % 2],)):
            for domain in DOMAINS:
                n = length(nseg, P)
                base = make_input(kind, domain, 2, n, P, seed_of("r2", P, kind, domain, nseg))
                ref2 = Ref(base, P)
                for rows in (1, 2):
                    ref = ref2 if rows == 2 else ref2.rows(slice(0, 1))
                    for dtype in DTYPES[domain]:
                        run_dtype(f"route 2 P={P} {kind} n={n} ", base[:rows], P, ref, dtype)


@pytest.mark.parametrize("P", range(1, 16))
def test_route2_every_length(P):
    """P = 1 (window [1.0], step 1), odd P (step = P - P // 2), segment counts around the 256 threads of a workgroup and 70 000 (many
    workgroups a row); every bin against the long-double reference."""
    run_route2(P)


# ----------------------------------------------------------------------------------------------- route 3: chunk seams
SEAM_L = (17, 100, 129, 1000)
SEAM_C = (16, 1, 2, 3, 5, 7, 15)          # chunk rows of 3 x 5 segments: one chunk first (the others are compared with it)


def plan_line(L):
    return 1 << max(8, (2 * L - 2).bit_length())


def run_route3_seams(L, set_chunk_bytes):
    assert utils._welch_layout(length(5, L), L)["route"] == 3
    assert plan_line(129) == 512 and plan_line(128 - 1) == 256
    M = plan_line(L)
    for kind in KINDS:
        for domain in DOMAINS:
            x = make_input(kind, domain, 3, length(5, L, extra=L // 4), L, seed_of("r3", L, kind, domain))
            ref = Ref(x, L)
            b2 = 2 * pn.bound(ref.A_all, ref.B_all, ref.T)
            for dtype in DTYPES[domain]:
                whole = None
                for c in SEAM_C:
                    set_chunk_bytes(c * M * 16)
                    what = f"route 3 L={L} {kind} chunk={c} {np.dtype(dtype).name}"
                    got = device_psd_f64(x.astype(dtype), L) if dtype == np.complex64 else device_psd(x.astype(dtype), L)
                    judge(what, got, ref)
                    if dtype == np.complex64:
                        judge(what, device_psd(x.astype(dtype), L), ref)
                    if whole is None:
                        whole = got
                    rc = _ratio(np.abs(got - whole), b2)
                    margins.record(f"{what} device / one chunk [|d| / (2 bound_k)]", None, rc, 1.0)
                    assert rc <= 1.0, (what, rc)


@pytest.mark.parametrize("L", SEAM_L)
def test_route3_chunk_seams(L, monkeypatch):
    """3 rows x 5 segments in chunks of 1, 2, 3, 5, 7, 15 and 16 frames: a seam inside a row, on a row boundary, a chunk over two and three
    rows, a short last chunk (its unused frames zeroed), one chunk.  Every result against the references, and against the one-chunk result
    at 2 x bound (the order of the sums changes with the chunk)."""
    run_route3_seams(L, lambda b: monkeypatch.setattr(utils, "CHUNK_BYTES", b))


@pytest.mark.parametrize("L", (7, 100))
def test_a_row_stride_on_routes_2_and_3(L):
    from opticomlib_amd.devices import default_device
    """The first m samples of every row of a longer device array (what .psd() does with a device field): no copy, the host slice's result."""
    ld, m = 7 * L + 11, 5 * L + L // 3
    for dtype in (np.float64, np.complex64, np.complex128):
        domain = "real" if dtype == np.float64 else "complex"
        x = make_input("white", domain, 2, ld, L, seed_of("ld", L, domain)).astype(dtype)
        x[:, m:] = 1e30
        d = _lib.DeviceArray.from_host(x, device=int(default_device()))
        h2d = _lib.TRANSFERS["h2d"]
        f, got = utils._welch(d, 1.0, L, n=m)
        assert _lib.TRANSFERS["h2d"] == h2d
        np.testing.assert_array_equal(got, device_psd(np.ascontiguousarray(x[:, :m]), L))
        judge(f"stride L={L} {np.dtype(dtype).name}", got, Ref(x[:, :m], L))


# ----------------------------------------------------------------------------------------------- row limits
ROW_LIMITS = ((65537, 16, 16), (65537, 16, 4), (65536, 20, 17))


def rows_input(rows, n, L):
    rng = np.random.default_rng(seed_of("rows", rows, L))
    scale = 1.0 + rng.permutation(rows) / rows                     # a distinct scale per row: a row written to the wrong place shows
    return rng.standard_normal((rows, n)) * scale[:, None]


def run_row_limit(rows, n, L, survey_bins=0):
    x = rows_input(rows, n, L)
    ref = Ref(x, L, ref=False, survey_bins=survey_bins)
    judge(f"rows={rows} L={L} float64", device_psd(x, L), ref)


@pytest.mark.parametrize("rows,n,L", ROW_LIMITS, ids=("route1", "route2", "route3"))
def test_more_rows_than_a_grid_takes(rows, n, L):
    """More than 65535 rows: routes 1 and 2 run in row blocks, route 3 accumulates all rows and finishes in row blocks."""
    assert rows > utils._MAX_GRID_ROWS and utils._welch_layout(n, L)["route"] == (1 if L == 16 else 2 if L == 4 else 3)
    run_row_limit(rows, n, L)


# ----------------------------------------------------------------------------------------------- size limit
def run_size_limit(survey_bins=0):
    L = 1 << 21
    x = make_input("white", "real", 1, L, L, seed_of("limit"))[0]
    judge(f"route 3 L=2^21 float64", device_psd(x, L), Ref(x, L, ref=False, survey_bins=survey_bins))


def test_the_longest_segment_route_3_takes():
    assert plan_line(1 << 21) == 1 << 22
    run_size_limit()


def test_one_sample_beyond_it_is_refused_before_any_upload():
    n = (1 << 21) + 1
    x = np.zeros(n)
    h2d = _lib.TRANSFERS["h2d"]
    with pytest.raises(ValueError, match=r"the device transform takes 2 \.\.\. 2\^21 samples per row, got 2097153"):
        oa.get_psd(x, 1.0, n)
    assert _lib.TRANSFERS["h2d"] == h2d


# ----------------------------------------------------------------------------------------------- value edges
EDGE_L = (5, 256, 100)                     # routes 2, 1, 3


@pytest.mark.parametrize("L", EDGE_L)
@pytest.mark.parametrize("bad", (np.nan, np.inf), ids=("nan", "inf"))
def test_a_nan_or_an_infinity_stays_in_its_row(L, bad):
    for domain in DOMAINS:
        x = make_input("white", domain, 3, length(4, L), L, seed_of("bad", L, domain))
        clean = Ref(x[1:], L)
        x[0, L + L // 3] = bad                                     # inside segments 1 and 2 of row 0, away from the window's zero
        assert np.isnan(scipy_psd(x, L)[0]).all()
        for dtype in DTYPES[domain]:
            got = device_psd(x.astype(dtype), L)
            assert np.isnan(got[0]).all(), (L, bad, dtype, got[0])
            assert np.isfinite(got[1:]).all()
            judge(f"rows beside a {bad} L={L} {np.dtype(dtype).name}", got[1:], clean)


@pytest.mark.parametrize("L", EDGE_L)
def test_zeros_give_exact_zeros(L):
    for dtype in (np.float64, np.complex64, np.complex128):
        got = device_psd(np.zeros((2, length(3, L, extra=1)), dtype), L)
        assert got.shape == (2, L) and not got.any() and not np.signbit(got).any()


@pytest.mark.parametrize("L", EDGE_L)
def test_a_constant_has_three_bins(L):
    """x = c: the window's own spectrum, c^2 (1/4 : 1 : 1/4) at the centre and nothing elsewhere -- the reference's other bins are below
    1e-36, and there the bound is its second-order term, (K u T)^2 B, about 1e-29 of the peak: the sharpest look at the window and twiddles."""
    c = 1.2345
    for dtype in (np.float64, np.complex64, np.complex128):
        x = np.full((2, length(6, L, extra=2)), c, dtype)              # (complex64: the rounded constant, exactly, in the reference too)
        ref = Ref(x, L)
        mid = L // 2
        rest = np.setdiff1d(np.arange(L), (mid - 1, mid, mid + 1))
        cc = float(np.real(x[0, 0])) ** 2
        assert abs(float(ref.p[0, mid]) - cc) < 1e-15 and abs(float(ref.p[0, mid - 1]) - cc / 4) < 1e-15
        assert float(np.max(np.abs(ref.p[:, rest]))) < 1e-36
        assert float(np.max(pn.bound(ref.A, ref.B, ref.T)[:, rest])) < 1e-25 * c * c
        got = device_psd(x, L)
        assert np.all(got[:, (mid - 1, mid, mid + 1)] > 0.2)
        if dtype == np.complex64:                                   # float32: the neighbour rule on the three bins (the rest is rounding dust
            three = [mid - 1, mid, mid + 1]                         # of either side); the float64 result of the same kernels on every bin
            assert got.dtype == np.float32 and pn.f32_neighbours(got[:, three], ref.p[:, three]).all()
            got = device_psd_f64(x, L)
        judge(f"constant L={L} {np.dtype(dtype).name}", got, ref)


@pytest.mark.parametrize("L", EDGE_L)
@pytest.mark.parametrize("e", (100, -100))
def test_scaling_by_a_power_of_two_is_exact(L, e):
    """2^e x gives 2^(2e) p bit for bit: a power of two commutes with every rounding, and nothing here is subnormal or overflows."""
    for domain in DOMAINS:
        x = make_input("white", domain, 2, length(7, L), L, seed_of("scale", L, domain))
        p = device_psd(x, L)
        assert p.min() > 1e-12
        y = np.ldexp(x.real, e) + (1j * np.ldexp(x.imag, e) if domain == "complex" else 0)
        np.testing.assert_array_equal(device_psd(y, L), np.ldexp(p, 2 * e))
        if domain == "complex":                                    # complex64 in: the float64 result (2^200 p is no float32)
            y32 = y.astype(np.complex64)
            assert np.array_equal(y32.astype(np.complex128), y) and min(np.abs(y.real).min(), np.abs(y.imag).min()) >= np.finfo(np.float32).tiny
            np.testing.assert_array_equal(device_psd_f64(y32, L), np.ldexp(device_psd_f64(x.astype(np.complex64), L), 2 * e))
