"""The small device kernels under the device paths, one by one, through the C ABI, against a plain float64 (or exact) restatement, at the
lengths that bracket every grid cap and tile of csrc/ and at the value edges the reference defines.

Grid caps and tiles the lengths bracket:
  * blocks_for / blocks_of (device_mem.hip, transmitter.hip): 8192 x 256 = 2^21 items per grid-stride sweep;
  * grid_for (eye.hip, ppm.hip): 4096 x 256 = 2^20; ssfm_device_count_diff: 1024 x 256 = 2^18;
  * the reductions: 1024 (MEAN, MIN) or 512 (MEAN2, POWER) fixed workgroups, then a sequential fold on the host;
  * the scans: tiles of 4096 items, one workgroup scanning 256 tile totals at a time with a carry (so past 2^20 items), and
    4096 workgroups striding over the tiles (so past 2^24 items).

Which kernels must be bit-exact with the reference's NumPy expression: add, convert, axpb, shift, scale_add, sum3,
sample, the ADC quantiser and the PPM kernels.  None of them may be contracted to a fused multiply-add.  The reductions and the cumsum
regroup additions and are checked against a bound derived from their fixed reduction tree; PM and MZM call sin / cos / exp and are checked
at the fixture tests' 1e-14 relative bound."""
import ctypes as C
import math

import numpy as np
import pytest

import eye_numpy as en
import opticomlib_amd as oa
import ppm_numpy as pn
from opticomlib_amd import _lib
from opticomlib_amd.typing import electrical_signal, gv, optical_signal

pytestmark = pytest.mark.gpu

U = 2.0 ** -53                                     # unit roundoff of float64
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 ** 18 - 1, 2 ** 18 + 1, 2 ** 20 - 1, 2 ** 20 + 1, 2 ** 21 - 1, 2 ** 21 + 1,
           3 * 2 ** 21 + 7]
PAST_2_24 = 2 ** 24 + 5
DEV = 0


# Every device buffer a test makes stays alive until the test ends: a DeviceArray that dies goes back to the library's pool (or to
# hipFree), so one made inside a call's argument list (`ssfm_x(P(up(a)))`) must not be freed before the kernel has read it.
_KEEP = []


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    _KEEP.clear()
    oa.devices.release_plans()


def lib():
    return _lib.load()


def ok(rc, what):
    _lib._check(rc, what)


def keep(d):
    _KEEP.append(d)
    return d


def up(a, dtype=None):
    return keep(_lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype), dtype, DEV))


def P(d):
    return None if d is None else _lib._VP(d.ptr)


def scratch(nbytes, fill=None):
    """A uint8 device buffer of nbytes (int32 arrays live in these), zeroed or filled with the byte `fill`."""
    if fill is None:
        return keep(_lib.zeros_device((max(int(nbytes), 1),), np.uint8, DEV))
    return up(np.full(max(int(nbytes), 1), fill, np.uint8))


def host(d, dtype=None, count=None):
    a = d.to_host()
    if dtype is not None:
        a = a.view(dtype)
    return a if count is None else a[:count]


def values(n, seed):
    """float64 of both signs over many binades, with exact zeros of both signs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    x[rng.random(n) < 0.01] = 0.0
    x[rng.random(n) < 0.01] = -0.0
    return x


def same_bits(got, want):
    """Bit-for-bit equality (-0.0 vs 0.0 counts as different); where want is NaN, got must be NaN too."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    f, ui = (np.float32, np.uint32) if want.dtype in (np.float32, np.complex64) else (np.float64, np.uint64)
    g, w = np.ascontiguousarray(got).view(f), np.ascontiguousarray(want).view(f)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan)
    bad = np.nonzero((g.view(ui) != w.view(ui)) & ~nan)[0]
    assert bad.size == 0, f"{bad.size} of {w.size} differ, first at {bad[0]}: {g[bad[0]]!r} vs {w[bad[0]]!r}"


# ============================================================================================ 1. elementwise primitives
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("prec", [_lib.C64, _lib.C128])
def test_add_is_numpy_add(n, prec):
    dt = np.complex64 if prec == _lib.C64 else np.complex128
    a = (values(2 * n, n).view(np.complex128)).astype(dt)
    b = (values(2 * n, n + 1).view(np.complex128)).astype(dt)
    da, db = up(a), up(b)
    out = _lib.DeviceArray((n,), dt, DEV)
    ok(lib().ssfm_device_add(DEV, P(out), P(da), P(db), prec, n), "ssfm_device_add")
    same_bits(out.to_host(), a + b)                                  # one IEEE addition per part: exact


@pytest.mark.parametrize("n", LENGTHS)
def test_convert_every_pair_is_numpy_astype(n):
    x = values(2 * n, n)
    x[:: 97] *= 2.0 ** 200                                           # beyond float32: inf after narrowing, as in NumPy
    c128 = x.view(np.complex128)
    with np.errstate(over="ignore"):
        c64 = c128.astype(np.complex64)
    r = values(n, n + 7)
    cases = [(c64, _lib.C64, _lib.C128, c64.astype(np.complex128)),      # widening: exact
             (c128, _lib.C128, _lib.C64, c64),                            # narrowing: round to nearest even, as NumPy
             (r, _lib.F64_REAL, _lib.C128, r.astype(np.complex128)),      # real -> complex, imaginary part +0
             (r, _lib.F64_REAL, _lib.C64, r.astype(np.complex64)),
             (c128, _lib.C128, _lib.F64_REAL, c128.real.copy())]
    for src, sp, dp, want in cases:
        d = up(src)
        out = _lib.DeviceArray(want.shape, want.dtype, DEV)
        ok(lib().ssfm_device_convert(DEV, P(d), sp, P(out), dp, n), "ssfm_device_convert")
        with np.errstate(over="ignore"):
            same_bits(out.to_host(), want)
    with pytest.raises(_lib.SsfmError):                              # complex -> real float32 is not a conversion the library offers
        ok(lib().ssfm_device_convert(DEV, P(up(c64)), _lib.C64, P(up(r)), _lib.F64_REAL, n), "ssfm_device_convert")


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True])
def test_axpb_is_the_dac_expression(n, cplx):
    x = values(2 * n if cplx else n, n)
    alpha, beta = 0.7310585786300049, -1.2345678901234567
    d = up(x)
    out = _lib.DeviceArray(x.shape, np.float64, DEV)
    ok(lib().ssfm_device_axpb(DEV, P(out), P(d), alpha, beta, n, int(cplx)), "ssfm_device_axpb")
    want = x * alpha + beta                                          # DAC: x * Vpp, then + offset: two roundings, no FMA
    if cplx:
        want[1::2] = x[1::2] * alpha                                 # beta is real: the imaginary parts are only scaled
    same_bits(out.to_host(), want)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True])
def test_shift_adds_re_and_im_to_the_right_lanes(n, cplx):
    x = values(2 * n if cplx else n, n)
    re, im = -0.3183098861837907, 2.718281828459045
    out = _lib.DeviceArray(x.shape, np.float64, DEV)
    ok(lib().ssfm_device_shift(DEV, P(out), P(up(x)), n, int(cplx), re, im), "ssfm_device_shift")
    want = (x.view(np.complex128) + complex(re, im)).view(np.float64) if cplx else x + re
    same_bits(out.to_host(), want)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("with_b", [False, True])
def test_scale_add_is_exact(n, with_b):
    x, b = values(n, n), values(n, n + 3)
    f = 1.4142135623730951
    out = _lib.DeviceArray((n,), np.float64, DEV)
    ok(lib().ssfm_device_scale_add(DEV, P(out), P(up(x)), f, P(up(b)) if with_b else None, n), "ssfm_device_scale_add")
    same_bits(out.to_host(), x * f + b if with_b else x * f)         # a product, then a sum: two roundings (no FMA)


SUM3_N = [1, 257, 4097, 2 ** 21 - 1, 2 ** 21 + 1, 3 * 2 ** 21 + 7, PAST_2_24]


@pytest.mark.parametrize("n", SUM3_N)
@pytest.mark.parametrize("mask", range(8))
def test_sum3_every_null_pattern(n, mask):
    arrs = [values(n, 10 * n + k) if mask >> k & 1 else None for k in range(3)]
    off, scale = 3.0e-3, 50.0
    out = _lib.DeviceArray((n,), np.float64, DEV)
    dev = [None if a is None else up(a) for a in arrs]
    ok(lib().ssfm_device_sum3(DEV, P(out), *[P(d) for d in dev], off, scale, n), "ssfm_device_sum3")
    terms = [a for a in arrs if a is not None]
    if terms:
        v = terms[0]
        for t in terms[1:]:
            v = v + t                                                # PD: (ase + shot) + thermal, then + dark current, times R_load
        want = (v + off) * scale
    else:
        want = np.full(n, off * scale)
    same_bits(out.to_host(), want)


INPLACE_N = [257, 4097, 2 ** 21 + 1, 3 * 2 ** 21 + 7, PAST_2_24]


@pytest.mark.parametrize("n", INPLACE_N)
def test_elementwise_in_place(n):
    """dst == src: every element must be read and written exactly once.  A grid-stride loop that steps too short writes the right value
    again and again out of place, which no value check sees; in place, an element updated twice is wrong."""
    x, b, c = values(n, n), values(n, n + 1), values(n, n + 2)
    def run(host_in, call):
        d = up(host_in)
        call(d)
        return d.to_host()
    f, off, scale = 1.4142135623730951, 3.0e-3, 50.0
    same_bits(run(x, lambda d: ok(lib().ssfm_device_scale_add(DEV, P(d), P(d), f, None, n), "scale_add")), x * f)
    db = up(b)
    same_bits(run(x, lambda d: ok(lib().ssfm_device_scale_add(DEV, P(d), P(d), f, P(db), n), "scale_add")), x * f + b)
    same_bits(run(x, lambda d: ok(lib().ssfm_device_axpb(DEV, P(d), P(d), 0.75, -1.25, n, 0), "axpb")), x * 0.75 - 1.25)
    same_bits(run(x, lambda d: ok(lib().ssfm_device_shift(DEV, P(d), P(d), n, 0, -0.5, 0.0), "shift")), x - 0.5)
    cx = np.concatenate([x, b]).view(np.complex128)
    same_bits(run(cx, lambda d: ok(lib().ssfm_device_add(DEV, P(d), P(d), P(up(cx[::-1].copy())), _lib.C128, cx.size), "add")), cx + cx[::-1])
    dc = up(c)
    for mask in (1, 3, 5, 7):                                         # out aliases a, with and without b and c
        want = x
        for t, bit in ((b, 2), (c, 4)):
            if mask & bit:
                want = want + t
        got = run(x, lambda d: ok(lib().ssfm_device_sum3(DEV, P(d), P(d), P(db) if mask & 2 else None, P(dc) if mask & 4 else None, off, scale, n),
                                  "sum3"))
        same_bits(got, (want + off) * scale)


# ============================================================================================ 2. reductions and scans
def sum_bound(x, depth):
    """|error| of a sum whose every term passes through at most `depth` roundings: depth * u * sum |x| (first order)."""
    return depth * U * math.fsum(np.abs(x))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("with_b", [False, True])
def test_reduce_mean(n, with_b):
    a, b = values(n, n) + 1.0, values(n, n + 1)
    m = C.c_double()
    ok(lib().ssfm_device_reduce(DEV, _lib.REDUCE_MEAN, P(up(a)), P(up(b)) if with_b else None, 1, n, 0, C.byref(m)), "ssfm_device_reduce")
    terms = np.concatenate([a, b]) if with_b else a
    want = math.fsum(terms) / n
    # 1024 x 256 threads: a serial run of ceil(n / 2^18) per thread, 6 shuffle levels, 3 adds over the waves, 1023 on the host; + a[i] + b[i]
    depth = -(-n // 2 ** 18) + 6 + 3 + 1023 + int(with_b)
    assert abs(m.value - want) <= sum_bound(terms, depth) / n + U * abs(want)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True])
def test_reduce_mean2(n, cplx):
    x = values(2 * n if cplx else n, n) - 0.5
    m = (C.c_double * 2)()
    ok(lib().ssfm_device_reduce(DEV, _lib.REDUCE_MEAN2, P(up(x)), None, 1, n, int(cplx), m), "ssfm_device_reduce")
    depth = -(-n // 2 ** 17) + 6 + 3 + 511                           # 512 x 256 threads, then 511 adds on the host
    for k, part in enumerate([x[0::2], x[1::2]] if cplx else [x]):
        want = math.fsum(part) / n
        assert abs(m[k] - want) <= sum_bound(part, depth) / n + U * abs(want), k


@pytest.mark.parametrize("n", [1, 3, 255, 4097, 2 ** 17 + 1, 2 ** 21 + 1])
@pytest.mark.parametrize("rows", [1, 2, 3])
@pytest.mark.parametrize("cplx", [False, True])
def test_reduce_power(n, rows, cplx):
    x = values(rows * n * (2 if cplx else 1), n + rows)
    out = (C.c_double * rows)()
    ok(lib().ssfm_device_reduce(DEV, _lib.REDUCE_POWER, P(up(x)), None, rows, n, int(cplx), out), "ssfm_device_reduce")
    sq = (x * x).reshape(rows, -1)
    depth = -(-n // 2 ** 17) + 6 + 3 + 511 + 2                       # + the square and the re^2 + im^2 of every element
    for r in range(rows):
        want = math.fsum(sq[r]) / n
        assert abs(out[r] - want) <= sum_bound(sq[r], depth) / n + U * abs(want), r


@pytest.mark.parametrize("n", LENGTHS)
def test_reduce_min_is_exact(n):
    rng = np.random.default_rng(n)
    m = C.c_double()
    run = lambda a: (ok(lib().ssfm_device_reduce(DEV, _lib.REDUCE_MIN, P(up(a)), None, 1, a.size, 0, C.byref(m)), "ssfm_device_reduce"), m.value)[1]
    x = rng.random(n) + 1.0
    x[-1] = 0.5                                                      # the minimum in the last element: every stride must reach it
    assert run(x) == 0.5
    x[-1] = -0.0                                                     # the only zero: its sign survives
    assert math.copysign(1.0, run(x)) == -1.0 and run(x) == 0.0
    x[rng.integers(0, n)] = -np.inf
    assert run(x) == -np.inf
    assert run(np.full(n, np.inf)) == np.inf


CUMSUM_N = [1, 2, 255, 4095, 4096, 4097, 256 * 4096 - 1, 256 * 4096 + 1, 2 ** 21 + 1, 5 * 2 ** 20 + 3, 3 * 2 ** 21 + 7]


@pytest.mark.parametrize("n", CUMSUM_N)
def test_cumsum_of_integers_is_exact(n):
    x = np.random.default_rng(n).integers(-8, 9, n).astype(np.float64)     # every partial sum is an integer below 2^53: no rounding at all
    out = _lib.cumsum_device(up(x)).to_host()
    np.testing.assert_array_equal(out, np.cumsum(x))


@pytest.mark.parametrize("n", [4097, 5 * 2 ** 20 + 3])
def test_cumsum_of_random_values_is_within_its_tree(n):
    x = np.random.default_rng(n).standard_normal(n)
    out = _lib.cumsum_device(up(x)).to_host()
    ref = np.cumsum(x.astype(np.longdouble))
    ntiles = -(-n // 4096)
    # a thread's 16 items, 8 Hillis-Steele levels in the tile, 8 levels + a carry per 256 tiles over the totals, the final add
    depth = 16 + 8 + 8 + ntiles // 256 + 2
    bound = depth * U * np.cumsum(np.abs(x))
    assert np.all(np.abs(out - ref.astype(np.float64)) <= bound + 1e-300)


COUNT_N = [1, 63, 4097, 2 ** 18 - 1, 2 ** 18 + 1, 2 ** 20 + 1, 3 * 2 ** 21 + 7, PAST_2_24]


def count_diff(da, db, n):
    e = _lib._I64(0)
    ok(lib().ssfm_device_count_diff(DEV, P(da), P(db), n, C.byref(e)), "ssfm_device_count_diff")
    return e.value


@pytest.mark.parametrize("n", COUNT_N)
def test_count_diff_compares_bytes(n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 3, n, dtype=np.uint8)                        # 0, 1 and 2: a 2 against a 1 is an error too
    b = rng.integers(0, 3, n, dtype=np.uint8)
    assert count_diff(up(a), up(b), n) == int(np.count_nonzero(a != b))
    assert count_diff(up(a), up(a), n) == 0


def test_count_diff_past_2_31():
    n = 2 ** 31 + 5                                                  # two 2 GiB buffers: a 32-bit index or count would wrap
    da, db = _lib.zeros_device((n,), np.uint8, DEV), _lib.zeros_device((n,), np.uint8, DEV)
    patches = {0: (1, 0), 2 ** 31 - 1: (2, 1), 2 ** 31: (1, 1), 2 ** 31 + 1: (0, 255), n - 1: (7, 3)}
    for pos, (va, vb) in patches.items():
        for d, v in ((da, va), (db, vb)):
            byte = np.array([v], np.uint8)
            ok(lib().ssfm_device_copy(DEV, _lib._VP(d.ptr + pos), _lib._ptr(byte), 1, 0), "ssfm_device_copy")
    assert count_diff(da, db, n) == sum(va != vb for va, vb in patches.values())


SAMPLE_COUNTS = [1, 64, 4097, 2 ** 20 - 1, 2 ** 20 + 1, 3 * 2 ** 21 + 7]


@pytest.mark.parametrize("count", SAMPLE_COUNTS)
@pytest.mark.parametrize("noise", [False, True])
def test_sample_is_the_sampler(count, noise):
    step = 3 if count < 2 ** 21 else 2
    start = 5
    n = start + (count - 1) * step + 1 + 2
    rng = np.random.default_rng(count)
    x = rng.integers(-3, 4, n).astype(np.float64) * 0.25             # small multiples of 1/4: many samples (and sums) equal thr exactly
    nz = rng.integers(-2, 3, n).astype(np.float64) * 0.25 if noise else None
    thr = 0.25
    x[start] = thr
    if noise:
        nz[start] = 0.0
    y = (x + nz if noise else x)[start:: step][:count]
    assert np.any(y == thr)
    dx, dn = up(x), (up(nz) if noise else None)
    vals, bits = _lib.DeviceArray((count,), np.float64, DEV), scratch(count, 0xAA)
    ok(lib().ssfm_device_sample(DEV, P(dx), P(dn), start, step, count, thr, P(vals), P(bits)), "ssfm_device_sample")
    same_bits(vals.to_host(), y)
    np.testing.assert_array_equal(bits.to_host(), (y > thr).astype(np.uint8))        # the reference's `>`: a sample equal to thr is 0
    only_v = _lib.DeviceArray((count,), np.float64, DEV)
    ok(lib().ssfm_device_sample(DEV, P(dx), P(dn), start, step, count, thr, P(only_v), None), "ssfm_device_sample")
    same_bits(only_v.to_host(), y)
    only_b = scratch(count, 0xAA)
    ok(lib().ssfm_device_sample(DEV, P(dx), P(dn), start, step, count, thr, None, P(only_b)), "ssfm_device_sample")
    np.testing.assert_array_equal(only_b.to_host(), (y > thr).astype(np.uint8))


def test_sample_count_zero_writes_nothing():
    x, bits = up(np.ones(8)), scratch(8, 0xAA)
    ok(lib().ssfm_device_sample(DEV, P(x), None, 0, 1, 0, 0.5, None, P(bits)), "ssfm_device_sample")
    np.testing.assert_array_equal(bits.to_host(), np.full(8, 0xAA, np.uint8))


# ============================================================================================ 3. sort, shortest interval, ADC
def check_sorted_like_numpy(got, x):
    """np.sort order: the numbers bit for bit (-0.0 and 0.0 keep their input order: the sort is stable and NumPy compares them equal), then
    every NaN last, whatever its sign, with the input's NaN bit patterns."""
    k = int(np.count_nonzero(~np.isnan(x)))
    assert np.all(np.isnan(got[k:]))
    num = x[~np.isnan(x)]
    stable = num[np.argsort(num, kind="stable")]                     # NumPy's order of the numbers; ties (+-0) in input order
    np.testing.assert_array_equal(got[:k].view(np.uint64), stable.view(np.uint64))
    np.testing.assert_array_equal(got[:k], np.sort(x)[:k])
    np.testing.assert_array_equal(np.sort(got[k:].view(np.uint64)), np.sort(x[np.isnan(x)].view(np.uint64)))    # the NaNs themselves, untouched


@pytest.mark.parametrize("n", [1, 2, 65, 2049, 4097, 2 ** 18 + 1, 2 ** 21])
def test_sort_puts_nan_of_either_sign_last(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    neg_nan = np.array([0xFFF8000000000000, 0xFFF0000000000001, 0xFFFFFFFFFFFFFFFF], np.uint64).view(np.float64)
    pos_nan = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], np.uint64).view(np.float64)
    special = np.concatenate([neg_nan, pos_nan, [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324]])
    pos = rng.integers(0, n, special.size)
    x[pos] = special
    d = up(x)
    ok(lib().ssfm_device_sort_f64(DEV, P(d), n), "ssfm_device_sort_f64")
    check_sorted_like_numpy(d.to_host(), x)


def shortest(x, percent):
    out = np.zeros(2)
    ok(lib().ssfm_shortest_int(DEV, P(up(x)), x.size, float(percent), _lib._ptr(out)), "ssfm_shortest_int")
    return out


SHORTEST_N = [2, 3, 64, 257, 4097, 2 ** 18 + 1, 2 ** 21]


@pytest.mark.parametrize("n", SHORTEST_N)
def test_shortest_int_with_ties(n):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 6, n).astype(np.float64)                     # small integers: many windows share the minimum width
    x2 = np.round(rng.standard_normal(n), 1)
    percents = [50, 99.99, 100.0 * 1.5 / n, 100.0 * (n - 0.5) / n] if n > 2 else [50, 99.0]
    for data in (x, x2):
        for p in percents:
            lag = int(n * p / 100)
            if not 1 <= lag < n:
                continue
            np.testing.assert_array_equal(shortest(data, p), en.shortest_int(data, p), err_msg=f"percent {p} lag {lag}")


def test_shortest_int_rejects_bad_percentages():
    x = np.arange(100.0)
    for p in (0.0, -5.0, 100.5, float("nan"), 0.5, 100.0):           # out of (0, 100], or a lag of 0 or of n
        with pytest.raises(_lib.SsfmError):
            shortest(x, p)
    with pytest.raises(_lib.SsfmError):
        shortest(np.arange(2 ** 21 + 1.0), 50)


def quantize(x, vmin, vmax, levels, volts):
    out = _lib.DeviceArray((x.size,), np.float64 if volts else np.int64, DEV)
    ok(lib().ssfm_adc_quantize(DEV, P(up(x)), x.size, vmin, vmax, levels, int(volts), P(out)), "ssfm_adc_quantize")
    return out.to_host()


@pytest.mark.parametrize("nbits", range(1, 17))
def test_adc_quantize_rounds_half_to_even(nbits):
    L = 2 ** nbits - 1
    vmin, vmax = -0.75, 1.25
    span = vmax - vmin
    k = np.arange(-3, L + 3, max(1, L // 4096), dtype=np.float64)
    x0 = vmin + (k + 0.5) * span / L                                  # the midpoints between codes, and codes below 0 / above L
    x = np.concatenate([np.nextafter(x0, -np.inf), x0, np.nextafter(x0, np.inf), vmin + k * span / L, [vmin - 3.0, vmax + 3.0, vmin, vmax]])
    q = (x - vmin) / span * L
    assert np.any(q == np.floor(q) + 0.5)                            # exact ties are present
    codes = np.round(q).astype(np.int64)                              # the reference's expression, in its order
    np.testing.assert_array_equal(quantize(x, vmin, vmax, L, False), codes)
    same_bits(quantize(x, vmin, vmax, L, True), codes / L * span + vmin)


def test_adc_quantize_ties_at_every_even_and_odd_code():
    vmin, vmax, L = 0.0, 255.0, 255                                   # span = L: q = x / 255 * 255, exact for these halves
    x = np.arange(-4, 260) + 0.5
    q = (x - vmin) / (vmax - vmin) * L
    assert np.array_equal(q, x)
    np.testing.assert_array_equal(quantize(x, vmin, vmax, L, False), np.round(q).astype(np.int64))


def test_adc_rejects_more_than_2_21_samples():
    gv(sps=16, R=10e9)
    with pytest.raises(ValueError, match="up to 2\\^21 samples"):
        oa.ADC(electrical_signal(np.arange(2 ** 21 + 1, dtype=np.float64)), otype="n")


# ============================================================================================ 4. PPM kernels
MS = [2, 4, 8, 16, 32, 64, 128, 256]


def slot_targets(M):
    """Symbol counts whose slot count sits on and beside a tile (4096), the scan's carry (256 tiles = 2^20) and the tile stride (2^24)."""
    out = {1}
    for slots in (4096, 2 ** 20, 2 ** 24):
        s = slots // M
        out |= {s - 1, s, s + 1}
    return sorted(v for v in out if v >= 1)


def encode(bits, nsym, M):
    out = scratch(nsym * M, 0xAA)
    ok(lib().ssfm_ppm_encode(DEV, P(bits), nsym, M, P(out)), "ssfm_ppm_encode")
    return out


def decode(slots, n, M, cap=None):
    """(count-only call, write call into a 0xAA-filled buffer of cap + 3 bytes)."""
    nb = _lib._I64(-1)
    ok(lib().ssfm_ppm_decode(DEV, P(slots), n, M, None, 0, C.byref(nb)), "ssfm_ppm_decode")
    cap = nb.value if cap is None else cap
    out = scratch(cap + 3, 0xAA)
    ok(lib().ssfm_ppm_decode(DEV, P(slots), n, M, P(out), cap, None), "ssfm_ppm_decode")
    return nb.value, out.to_host()


@pytest.mark.parametrize("M", MS)
def test_encode_decode_at_tile_and_carry_boundaries(M):
    k = int(np.log2(M))
    rng = np.random.default_rng(M)
    for nsym in slot_targets(M):
        bits = rng.integers(0, 2, nsym * k, dtype=np.uint8)
        slots = encode(up(bits), nsym, M)
        want = pn.encode(bits, M)
        np.testing.assert_array_equal(slots.to_host(), want, err_msg=f"encode nsym={nsym}")
        nb, got = decode(slots, nsym * M, M)
        assert nb == nsym * k
        np.testing.assert_array_equal(got[:nb], bits, err_msg=f"decode nsym={nsym}")
        assert np.all(got[nb:] == 0xAA)


DECODE_N = [1, 2, 255, 4095, 4096, 4097, 256 * 4096 - 1, 256 * 4096 + 1, 2 ** 21 + 1, 3 * 2 ** 21 + 7, PAST_2_24]


@pytest.mark.parametrize("n", DECODE_N)
@pytest.mark.parametrize("M", [2, 16, 256])
def test_decode_any_bytes(n, M):
    """Zero, one or several nonzero slots per symbol, nonzero values other than 1, a length that is not a multiple of M."""
    k = int(np.log2(M))
    rng = np.random.default_rng(n * M)
    x = rng.integers(1, 256, n).astype(np.uint8)
    x[rng.random(n) < (1 - 1.5 / M)] = 0                              # about 1.5 ON slots per symbol: many empty and many multi-ON symbols
    d = up(x)
    want = pn.decode(x, M)
    nb, got = decode(d, n, M)
    assert nb == want.size
    np.testing.assert_array_equal(got[:nb], want)
    assert np.all(got[nb:] == 0xAA)
    if want.size > k:
        cap = want.size - k - (k > 1)                                 # truncated inside a symbol (k > 1): only whole symbols below cap are written
        _, got = decode(d, n, M, cap)
        whole = cap // k * k
        np.testing.assert_array_equal(got[:whole], want[:whole])
        assert np.all(got[whole:] == 0xAA)


FAULTY_N = [1, 2, 4095, 4097, 256 * 4096 + 1, 3 * 2 ** 21 + 7, PAST_2_24]


@pytest.mark.parametrize("n", FAULTY_N)
def test_faulty_lists_every_symbol_not_holding_one_slot(n):
    rng = np.random.default_rng(n)
    c = rng.choice(np.array([0, 1, 2, 7, 65536], np.int32), n, p=[0.1, 0.7, 0.1, 0.05, 0.05]).astype(np.int32)
    idx, cnt = scratch(4 * n), scratch(4 * n)
    nf = _lib._I64(-1)
    ok(lib().ssfm_ppm_faulty(DEV, P(up(c.view(np.uint8))), n, P(idx), P(cnt), C.byref(nf)), "ssfm_ppm_faulty")
    wi, wc = pn.faulty(c)
    assert nf.value == wi.size
    np.testing.assert_array_equal(host(idx, np.int32, wi.size), wi)
    np.testing.assert_array_equal(host(cnt, np.int32, wi.size), wc)


def test_faulty_with_none_one_and_two():
    for c in (np.ones(5000, np.int32), np.r_[np.ones(4999, np.int32), 0].astype(np.int32), np.r_[2, np.ones(4097, np.int32), 0].astype(np.int32)):
        n = c.size
        idx, cnt = scratch(4 * n), scratch(4 * n)
        nf = _lib._I64(-1)
        ok(lib().ssfm_ppm_faulty(DEV, P(up(c.view(np.uint8))), n, P(idx), P(cnt), C.byref(nf)), "ssfm_ppm_faulty")
        wi, wc = pn.faulty(c)
        assert nf.value == wi.size
        np.testing.assert_array_equal(host(idx, np.int32, wi.size), wi)
        np.testing.assert_array_equal(host(cnt, np.int32, wi.size), wc)


def decide_inputs(nsym, M, u8, noise, start, step, seed):
    """x (and noise) covering start + (nsym M - 1) step, with exact ties and NaNs in several lanes; y = the slot samples, (nsym, M)."""
    rng = np.random.default_rng(seed)
    n = start + (nsym * M - 1) * step + 1 + step
    if u8:
        x = (rng.random(n) < 1.5 / M).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
        y = (x != 0).astype(np.float64)
        return x, None, y[start:: step][: nsym * M].reshape(nsym, M)
    x = rng.integers(0, 4, n).astype(np.float64)                      # a handful of levels: ties inside most symbols
    x[rng.random(n) < 0.02] = np.nan
    q = lambda s, j: start + (s * M + j) * step
    x[[q(0, M - 1), q(0, max(1, M // 2))]] = np.nan                   # symbol 0: two NaNs, the lower one wins
    if nsym > 1:
        x[[q(1, j) for j in range(M)]] = 3.0                          # symbol 1: a tie over every slot, slot 0 wins
    if nsym > 2:
        x[[q(2, j) for j in range(M)]] = 1.0
        x[q(2, M - 1)] = np.nan                                       # symbol 2: a NaN in the last slot beats every number
    nz = rng.integers(-1, 2, n).astype(np.float64) if noise else None
    v = x + nz if noise else x
    return x, nz, v[start:: step][: nsym * M].reshape(nsym, M)


DECIDE_CASES = [(M, nsym) for M in (2, 4, 64, 256) for nsym in (1, 3, 1000)] + [(2, 2 ** 20 + 3), (16, 2 ** 17 + 1), (256, 40001)]


@pytest.mark.parametrize("M,nsym", DECIDE_CASES)
@pytest.mark.parametrize("kind", ["u8", "f64", "f64+noise"])
def test_soft_decision_is_np_argmax(M, nsym, kind):
    u8, noise = kind == "u8", kind.endswith("noise")
    start, step = (7, 3) if nsym < 2 ** 17 else (1, 1)
    x, nz, y = decide_inputs(nsym, M, u8, noise, start, step, nsym * M)
    k = int(np.log2(M))
    bits, slots = scratch(nsym * k, 0xAA), scratch(nsym * M, 0xAA)
    ok(lib().ssfm_ppm_decide(DEV, P(up(x)), P(up(nz) if noise else None), int(u8), start, step, nsym, M, 0, 0.0, P(bits), P(slots), None),
       "ssfm_ppm_decide")
    v = np.argmax(y, axis=1)                                          # a NaN wins, the first index wins a tie
    np.testing.assert_array_equal(bits.to_host(), pn.bits_of(v, k))
    np.testing.assert_array_equal(slots.to_host(), pn.one_hot(v, M))


@pytest.mark.parametrize("M,nsym", DECIDE_CASES)
@pytest.mark.parametrize("kind", ["u8", "f64", "f64+noise"])
def test_hard_decision_and_resolve(M, nsym, kind):
    u8, noise = kind == "u8", kind.endswith("noise")
    start, step = (7, 3) if nsym < 2 ** 17 else (1, 1)
    x, nz, y = decide_inputs(nsym, M, u8, noise, start, step, nsym * M + 1)
    thr = 0.5 if u8 else 2.0                                          # integer levels: samples equal to thr are OFF (`>`)
    k = int(np.log2(M))
    dx, dn = up(x), (up(nz) if noise else None)
    bits, slots, counts = scratch(nsym * k, 0xAA), scratch(nsym * M, 0xAA), scratch(4 * nsym)
    ok(lib().ssfm_ppm_decide(DEV, P(dx), P(dn), int(u8), start, step, nsym, M, 1, thr, P(bits), P(slots), P(counts)), "ssfm_ppm_decide")
    on = y > thr
    cnt = on.sum(axis=1)
    np.testing.assert_array_equal(host(counts, np.int32, nsym), cnt)
    one = cnt == 1
    v = np.argmax(on, axis=1)
    gb, gs = bits.to_host().reshape(nsym, k), slots.to_host().reshape(nsym, M)
    np.testing.assert_array_equal(gb[one].ravel(), pn.bits_of(v[one], k))
    np.testing.assert_array_equal(gs[one].ravel(), pn.one_hot(v[one], M))
    assert np.all(gb[~one] == 0xAA) and np.all(gs[~one] == 0xAA)     # left to the resolution
    # the caller's draws for the faulty symbols, in ascending order
    idx, c = pn.faulty(cnt)
    rng = np.random.default_rng(nsym)
    draws = (rng.random(c.size) * np.where(c == 0, M, c)).astype(np.int32)
    ok(lib().ssfm_ppm_resolve(DEV, P(dx), P(dn), int(u8), start, step, nsym, M, thr, P(counts), P(up(idx.astype(np.int32).view(np.uint8))) if idx.size else
                              P(scratch(4)), P(up(draws.view(np.uint8))) if idx.size else P(scratch(4)), idx.size, 0, 0, P(bits), P(slots)), "ssfm_ppm_resolve")
    v[idx] = pn.resolve(on, idx, draws)
    np.testing.assert_array_equal(bits.to_host(), pn.bits_of(v, k))
    np.testing.assert_array_equal(slots.to_host(), pn.one_hot(v, M))


@pytest.mark.parametrize("M,nsym", [(4, 3000), (256, 5000)])
def test_resolve_with_device_draws_is_the_philox_rule(M, nsym):
    """idx NULL: every symbol whose count is not 1 draws r = floor(u bound / 2^32) from Philox4x32-10 keyed by the seed, counter (symbol,
    stream); bound = M for an empty symbol (slot r turns ON), else its count (its r-th ON slot is kept)."""
    x, nz, y = decide_inputs(nsym, M, False, True, 2, 2, M)
    thr, k = 2.0, int(np.log2(M))
    seed, stream = 0x0123456789ABCDEF, 0x100000007                    # both halves of both 64-bit words matter
    dx, dn = up(x), up(nz)
    bits, slots, counts = scratch(nsym * k, 0xAA), scratch(nsym * M, 0xAA), scratch(4 * nsym)
    ok(lib().ssfm_ppm_decide(DEV, P(dx), P(dn), 0, 2, 2, nsym, M, 1, thr, P(bits), P(slots), P(counts)), "ssfm_ppm_decide")
    ok(lib().ssfm_ppm_resolve(DEV, P(dx), P(dn), 0, 2, 2, nsym, M, thr, P(counts), None, None, 0, seed, stream, P(bits), P(slots)),
       "ssfm_ppm_resolve")
    on = y > thr
    cnt = on.sum(axis=1)
    idx, c = pn.faulty(cnt)
    assert np.any(c > 1) and (M > 16 or np.any(c == 0))               # (M = 256: no symbol is empty)
    draws = pn.device_draws(idx, np.where(c == 0, M, c), seed, stream)
    v = np.argmax(on, axis=1)
    v[idx] = pn.resolve(on, idx, draws)
    np.testing.assert_array_equal(bits.to_host(), pn.bits_of(v, k))
    np.testing.assert_array_equal(slots.to_host(), pn.one_hot(v, M))
    if M == 4:                                                        # (the empty symbols' slots spread over [0, M))
        assert set(v[idx[c == 0]].tolist()) == set(range(M))


# ============================================================================================ 5. PM / MZM elementwise kernels
PM_N = [1, 257, 2 ** 21 - 1, 2 ** 21 + 1, 3 * 2 ** 21 + 7]


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def fields(n_pol, n, seed):
    rng = np.random.default_rng(seed)
    shape = (n,) if n_pol == 1 else (2, n)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)), (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 1e-3


@pytest.mark.parametrize("n", PM_N)
@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("cplx", [False, True])
def test_pm_kernel_is_the_reference_expression(n, n_pol, cplx):
    s, z = fields(n_pol, n, n)
    rng = np.random.default_rng(n + 1)
    v, vn = rng.standard_normal(n) * 3.0, rng.standard_normal(n) * 0.1
    if cplx:
        v, vn = v + 0.2j * rng.standard_normal(n), vn + 0.01j * rng.standard_normal(n)
    Vpi = 3.3
    out_s, out_n = _lib.DeviceArray(s.shape, np.complex128, DEV), _lib.DeviceArray(s.shape, np.complex128, DEV)
    ok(lib().ssfm_pm(DEV, P(out_s), P(out_n), P(up(s)), P(up(z)), n_pol, n, P(up(v)), P(up(vn)), int(cplx), Vpi), "ssfm_pm")
    h = np.exp(1j * (v * np.pi / Vpi + vn * np.pi / Vpi))            # reference devices.py:613-620, in float64
    assert rel(out_s.to_host(), s * h) < 1e-14                        # the fixture tests' bound: sin / cos / exp to a few ulp
    assert rel(out_n.to_host(), z * h) < 1e-14


@pytest.mark.parametrize("n", [2 ** 21 + 1])
@pytest.mark.parametrize("n_pol", [1, 2])
def test_pm_scalar_host_and_device_drive(n, n_pol):
    gv(sps=16, R=10e9)
    s, z = fields(n_pol, n, n_pol)
    v = np.random.default_rng(3).standard_normal(n)
    Vpi = 5.0
    for drive, vv in ((2.5, np.full(n, 2.5)), (v, v), (electrical_signal.from_device(up(v, np.float64)), v)):
        out = oa.PM(optical_signal(s, z), drive, Vpi=Vpi)
        h = np.exp(1j * vv * np.pi / Vpi)
        assert rel(out.signal, s * h) < 1e-14 and rel(out.noise, z * h) < 1e-14


@pytest.mark.parametrize("n", PM_N)
@pytest.mark.parametrize("n_pol,dead", [(1, -1), (2, -1), (2, 0), (2, 1)])
@pytest.mark.parametrize("cplx", [False, True])
def test_mzm_kernel_is_the_reference_expression(n, n_pol, dead, cplx):
    s, z = fields(n_pol, n, n + 5)
    rng = np.random.default_rng(n + 6)
    v, vn = rng.standard_normal(n), rng.standard_normal(n) * 0.05
    if cplx:
        v, vn = v + 0.1j * rng.standard_normal(n), vn + 0.01j * rng.standard_normal(n)
    k, bias, sqrt_loss, half_eta = np.pi / (2 * 5.0), 2.5, 0.9, 0.05
    out_s, out_n = _lib.DeviceArray(s.shape, np.complex128, DEV), _lib.DeviceArray(s.shape, np.complex128, DEV)
    ok(lib().ssfm_mzm(DEV, P(out_s), P(out_n), P(up(s)), P(up(z)), n_pol, n, P(up(v)), P(up(vn)), int(cplx), k, bias, sqrt_loss, half_eta, dead), "ssfm_mzm")
    g = k * (v + bias) + k * vn                                       # reference devices.py:762-767
    h = sqrt_loss * (np.cos(g) + 1j * half_eta * np.sin(g))
    ws, wn = s * h, z * h
    if n_pol == 2 and dead >= 0:
        ws[dead] = 0
        wn[dead] = 0
    gs, gn = out_s.to_host(), out_n.to_host()
    assert rel(gs, ws) < 1e-14 and rel(gn, wn) < 1e-14
    if n_pol == 2 and dead >= 0:
        assert not np.any(gs[dead]) and not np.any(gn[dead])
