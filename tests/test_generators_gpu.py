"""The kernels that make data from nothing, element by element against a restatement: what they write is decided by index arithmetic alone, which
goes wrong past the first grid-stride sweep, past a power of two, or when two callers share a counter.

  * k_randn (device_mem.hip): 8192 x 256 pairs per sweep, so elements from 2^22 on come from the second sweep and from 2^23 on from the third;
    every element against tests/philox_numpy.py in long double, at a bound taken from the documented ulp limits of the device math library;
  * rng="device" in PD / EDFA / LASER: the oracle fed the restated draws of the streams the device call must have used, in the oracle's call order;
  * k_prbs (prbs.hip): jumps with M^(2^k) for k up to 26, against a shift map built from the oracle's single shift and powered in NumPy;
  * k_chirp (chirpz.hip): exp(-i pi m^2 / n) against long double with the phase reduced in integers;
  * the loaders of the DAC and of the benchmark field: 4096 x 256 = 2^20 items per sweep, on plans of 2^21 points, bit for bit.

Bound of a normal deviate.  The kernel evaluates mean + std * sqrt(-2 log u1) * (cos, sin)(2 pi u2) with the device math library's double log, sqrt
and sincospi.  This machine's ROCm documentation carries no table of their ulp limits, so the OpenCL full-profile limits for double stand in:
log 3 ulp, sqrt 0.5 ulp (correctly rounded), sincospi 4 ulp.  A relative error e_log of the logarithm is e_log / 2 of its root, the root adds
e_sqrt, the cosine e_sc of at most 1, and the two products round once each (0.5 + 0.5): K = e_log / 2 + e_sqrt + e_sc + 1 = 7 units of 2^-53 of
|std| r, and the final sum with `mean` rounds once more, 2^-53 |result|.  (With r < 1 the bound is taken at r = 1.)"""
import functools
import math

import numpy as np
import pytest

import margins
import opticomlib_amd as oa
import philox_numpy as ph
from opticomlib_amd import _lib
from opticomlib_amd import devices as od
from opticomlib_amd.typing import gv, optical_signal

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
DEV = 0
E_LOG, E_SQRT, E_SINCOS = 3.0, 0.5, 4.0               # OpenCL full profile, double
K_RANDN = E_LOG / 2 + E_SQRT + E_SINCOS + 1.0
SWEEP = 2 ** 22                                        # elements of one grid-stride sweep of k_randn
BIG = 2 ** 23 + 5                                      # the smallest count at which a third sweep starts and the last pair is cut
COUNTS = [1, 2, 3, 511, 512, 513, SWEEP - 1, SWEEP, SWEEP + 1, BIG]
SEED_HI, STREAM_HI = 2 ** 64 - 1, 2 ** 63 + 7

_KEEP = []


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    _KEEP.clear()
    oa.devices.release_plans()


def keep(d):
    _KEEP.append(d)
    return d


def up(a, dtype=None):
    return keep(_lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype), dtype, DEV))


def download(d, start, count):
    """`count` items of the 1-D device array `d` from item `start` on: only the slice compared crosses the bus."""
    out = np.empty(int(count), d.dtype)
    _lib.api.ssfm_device_copy(d.device, _lib._ptr(out), _lib._VP(d.ptr + int(start) * d.dtype.itemsize), out.nbytes, _lib.COPY_D2H)
    return out


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{bad.size} of {w.size} words differ, first at {bad[0]}: {got.view(np.float64)[bad[0]]!r} vs {want.view(np.float64)[bad[0]]!r}"


# ============================================================================================ 1. Philox / Box-Muller, every element
@functools.lru_cache(maxsize=None)
def unit_draws(seed, stream, count):
    """(N(0, 1) draws in long double, r per element) of one (seed, stream): computed once, shared, never written."""
    x, r = ph.randn(count, 1.0, seed, stream)
    rr = np.repeat(r, 2)[:count]
    x.setflags(write=False)
    rr.setflags(write=False)
    return x, rr


def draws(seed, stream, count):
    """A prefix of the long reference where it exists: the content depends on the flat index only."""
    if (seed, stream) == (SEED_HI, STREAM_HI):
        x, r = unit_draws(seed, stream, BIG + 1)
        return x[:count], r[:count]
    return unit_draws(seed, stream, count)


def hold_randn(got, std, seed, stream, mean=0.0, what=""):
    got = np.ascontiguousarray(got).view(np.float64).ravel()
    unit, r = draws(seed, stream, got.size)
    want = LD(mean) + LD(std) * unit
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    bound = K_RANDN * U * abs(std) * np.maximum(r, 1.0) + U * np.abs(got)
    k = int(np.argmax(err / bound))
    margins.record(f"randn {what} n={got.size} (element {k}, r={r[k]:.2f})", None, err[k], bound[k])
    print(f"randn {what} n={got.size}: worst |d| / bound = {err[k] / bound[k]:.3f} at element {k}, r = {r[k]:.3f}")
    assert err[k] <= bound[k], f"element {k}: {got[k]!r} vs {want[k]!r}, |d| = {err[k]:.3e} > {bound[k]:.3e}"


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_randn_every_element(count, dtype):
    cplx = dtype is np.complex128
    shape = ((count + 1) // 2,) if cplx else (count,)             # complex: the same doubles, an even number of them
    d = _lib.randn_device(shape, 1.5, SEED_HI, STREAM_HI, dtype, DEV)
    got = d.to_host()
    assert got.shape == shape and got.dtype == dtype
    hold_randn(got, 1.5, SEED_HI, STREAM_HI, what="complex128" if cplx else "float64")
    if count == BIG and not cplx:                                   # the extreme draws are compared like all the others: they are there
        unit, r = draws(SEED_HI, STREAM_HI, count)
        assert float(np.max(np.abs(unit))) > 5.0 and float(np.max(r)) > 5.3


@pytest.mark.parametrize("rows", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_randn_content_depends_on_the_flat_index_only(rows, dtype):
    n = 4097                                                       # odd: a real pair straddles the row boundary
    shape = (n,) if rows == 1 else (rows, n)
    got = _lib.randn_device(shape, 0.25, SEED_HI, STREAM_HI, dtype, DEV).to_host()
    assert got.shape == shape
    hold_randn(got, 0.25, SEED_HI, STREAM_HI, what=f"{rows} x {n} {np.dtype(dtype).name}")
    flat = _lib.randn_device((rows * n,), 0.25, SEED_HI, STREAM_HI, dtype, DEV).to_host()
    same_bits(got.ravel(), flat)


@pytest.mark.parametrize("seed,stream", [(SEED_HI, 2 ** 32), (0x0123456789ABCDEF, 0), (0x80000000, 2 ** 32 + 1), (1, 2 ** 64 - 1)])
def test_randn_takes_all_64_bits_of_seed_and_stream(seed, stream):
    n = 1001
    got = _lib.randn_device((n,), 1.0, seed, stream).to_host()
    hold_randn(got, 1.0, seed, stream, what=f"seed {seed:#x} stream {stream:#x}")
    for other in ((seed, stream & 0xFFFFFFFF), (seed & 0xFFFFFFFF, stream), (seed, stream ^ (1 << 32)), (seed ^ (1 << 63), stream)):
        if other != (seed, stream):                                # a dropped high word would make these equal
            assert not np.array_equal(got, _lib.randn_device((n,), 1.0, *other).to_host()), other


def raw_randn(n, seed, stream, mean, std):
    out = keep(_lib.DeviceArray((n,), np.float64, DEV))
    _lib.api.ssfm_device_randn(DEV, out, n, seed, stream, float(mean), float(std))
    return out.to_host()


@pytest.mark.parametrize("n", [1, 4099, SWEEP + 1])
def test_randn_mean_and_sign_of_std_through_the_abi(n):
    same_bits(raw_randn(n, SEED_HI, STREAM_HI, -1.25, 0.0), np.full(n, -1.25))            # std = 0: exactly the mean
    hold_randn(raw_randn(n, SEED_HI, STREAM_HI, 0.0, -0.75), -0.75, SEED_HI, STREAM_HI, what="std < 0")
    hold_randn(raw_randn(n, SEED_HI, STREAM_HI, 3.5, 0.75), 0.75, SEED_HI, STREAM_HI, mean=3.5, what="mean 3.5")
    hold_randn(raw_randn(n, SEED_HI, STREAM_HI, -1e3, -2.0), -2.0, SEED_HI, STREAM_HI, mean=-1e3, what="mean -1e3, std < 0")


@pytest.mark.parametrize("dtype", [np.complex64, np.float32, np.uint8, np.int64, np.float16])
def test_randn_device_refuses_what_the_kernel_would_overrun(dtype, monkeypatch):
    """ssfm_device_randn writes float64: a complex64 or float32 buffer is half as long as what it writes.  The refusal comes before any
    buffer exists, so nothing can reach the kernel."""
    def no_buffer(*a, **k):
        raise AssertionError("randn_device made a buffer before it looked at the dtype")
    monkeypatch.setattr(_lib, "DeviceArray", no_buffer)
    monkeypatch.setattr(_lib.api, "ssfm_device_randn", no_buffer, raising=False)
    with pytest.raises(TypeError, match="float64 or complex128"):
        _lib.randn_device((64,), 1.0, 1, 1, dtype)


# ============================================================================================ 2. realisations of rng="device"
class Restated:
    """np.random.normal / randn for the oracle: call k after `start` returns the restated draws of stream start + k of the device seed."""
    def __init__(self, seed, long_double=False):
        self.seed, self.stream, self.long_double = seed, 0, long_double

    def _unit(self, count):
        self.stream += 1
        return ph.randn(count, 1.0, self.seed, self.stream)[0]

    def normal(self, loc, scale, size):
        x = LD(loc) + LD(scale) * self._unit(int(size))
        return x if self.long_double else x.astype(np.float64)

    def randn(self, rows, n):
        """EDFA: the device draws one complex (2, n) array; the reference's randn(4, n) is [re x, re y, im x, im y]."""
        assert rows == 4
        z = self._unit(4 * n).astype(np.float64).view(np.complex128).reshape(2, n)
        return np.array([z[0].real, z[1].real, z[0].imag, z[1].imag])

    def patch(self, monkeypatch):
        monkeypatch.setattr(np.random, "normal", self.normal)
        monkeypatch.setattr(np.random, "randn", self.randn)


def field(n_pol, n, seed, scale):
    rng = np.random.default_rng(seed)
    shape = (n,) if n_pol == 1 else (2, n)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale


TOL_FRONT = 1e-11                                      # the suite's bound for PD: square law, then the zero-phase filter (test_gpu_parity.py)
TOL_FILT = 1e-11
PD_MODES = ("ase-only", "thermal-only", "shot-only", "ase-thermal", "ase-shot", "thermal-shot", "all")


@pytest.mark.parametrize("n", [5000, 2 ** 14])
@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("has_ase", [False, True])
def test_pd_realisation_is_the_oracle_on_the_restated_streams(n, n_pol, has_ase, monkeypatch):
    from oracle import filters_numpy as fo, frontend_numpy as fe
    gv(sps=16, R=10e9)
    fs = gv.fs
    s = field(n_pol, n, n + n_pol, 0.03)
    z = field(n_pol, n, n + n_pol + 7, 0.003) if has_ase else None
    x = optical_signal(s) if z is None else optical_signal(s, z)
    seed = 0xF0E1D2C3B4A59687
    fake = Restated(seed)
    fake.patch(monkeypatch)
    kw = dict(BW=20e9, r=0.8, T=290.0, R_load=75.0, i_dark=5e-9, Fn=1.5)
    oa.device_rng_seed(seed)
    calls = [(m, False) for m in PD_MODES] + [("all", True)]        # the last one: a second call with no reseeding goes on with the next streams
    for mode, _again in calls:
        expect = int("thermal" in mode or mode == "all") + int("shot" in mode or mode == "all")
        s0 = od._DEVICE_RNG["stream"]
        y = oa.PD(x, include_noise=mode, rng="device", **kw)
        assert od._DEVICE_RNG["stream"] - s0 == expect, mode      # one stream per term: thermal first, then shot
        fake.stream = s0
        if mode == "ase-only" and not has_ase:                      # the dark current alone (the reference adds it to a NULL noise)
            want_s, _ = fe.pd(s, None, fs, include_noise="none", **kw)
            want_n = fo.lpf(np.full(n, (0.0 + kw["i_dark"]) * kw["R_load"]), kw["BW"], fs)[0]
        else:
            want_s, want_n = fe.pd(s, z, fs, include_noise=mode, **kw)
        assert fake.stream - s0 == expect, mode
        what = f"PD {mode} n={n} n_pol={n_pol} ase={has_ase}"
        assert margins.within(y.signal, want_s, TOL_FRONT, what=what + " signal")
        assert margins.within(y.noise, want_n, TOL_FRONT, what=what + " noise")
    assert od._DEVICE_RNG["stream"] == 10                          # 0 + 1 + 1 + 1 + 1 + 2 + 2 + 2 streams in all


@pytest.mark.parametrize("n", [5001, 2 ** 14])
@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("has_noise", [False, True])
def test_edfa_realisation_is_the_oracle_on_the_restated_stream(n, n_pol, has_noise, monkeypatch):
    from oracle import frontend_numpy as fe
    gv(sps=16, R=10e9)
    s = field(n_pol, n, 3 * n + n_pol, 0.01)
    z = field(n_pol, n, 3 * n + n_pol + 1, 0.001) if has_noise else None
    x = optical_signal(s) if z is None else optical_signal(s, z)
    seed = 2 ** 64 - 59
    fake = Restated(seed)
    fake.patch(monkeypatch)
    oa.device_rng_seed(seed)
    for BW, bound in ((None, 1e-14), (60e9, TOL_FILT), (None, 1e-14)):       # (the third call: the third stream)
        s0 = od._DEVICE_RNG["stream"]
        y = oa.EDFA(x, G=17.0, NF=5.5, BW=BW, rng="device")
        assert od._DEVICE_RNG["stream"] - s0 == 1
        fake.stream = s0
        want_s, want_n = fe.edfa(s, z, gv.fs, gv.f0, 17.0, 5.5, BW=BW)
        assert fake.stream - s0 == 1
        what = f"EDFA BW={BW} n={n} n_pol={n_pol} noise={has_noise}"
        assert y.signal.shape == (2, n) and y.noise.shape == (2, n)
        assert margins.within(y.signal, want_s, bound, what=what + " signal")
        assert margins.within(y.noise, want_n, bound, what=what + " noise")


LASER_CASES = [dict(lw=1e6), dict(rin=-150), dict(lw=1e6, rin=-150), dict(lw=2e5, rin=-145, df=1e9)]


@pytest.mark.parametrize("N", [313, 1024])
@pytest.mark.parametrize("kw", LASER_CASES, ids=lambda k: "+".join(k))
def test_laser_realisation_is_the_oracle_on_the_restated_streams(N, kw, monkeypatch):
    from oracle import transmitter_numpy as tx
    gv(sps=16, R=10e9, N=N)
    n = gv.t.size
    seed = 0x8000000000000001
    fake = Restated(seed, long_double=True)                         # the oracle's running sum is then the high-precision one
    fake.patch(monkeypatch)
    oa.device_rng_seed(seed)
    expect = int("lw" in kw) + int("rin" in kw)
    for _ in range(2):                                              # the second call goes on with the next streams
        s0 = od._DEVICE_RNG["stream"]
        y = oa.LASER(P0=3, rng="device", **kw)
        assert od._DEVICE_RNG["stream"] - s0 == expect              # the phase increments first, then the intensity noise
        fake.stream = s0
        want = tx.laser(gv.t, gv.dt, gv.fs, 3, **kw)
        assert fake.stream - s0 == expect
        max_phase = 0.0
        if "lw" in kw:
            fake.stream = s0
            max_phase = float(np.max(np.abs(np.cumsum(fake.normal(0, np.sqrt(2 * np.pi * kw["lw"] * gv.dt), n)))))
        got = y.signal
        assert got.shape == (n,) and got.dtype == (np.float64 if set(kw) == {"rin"} else np.complex128)
        # the tree bound of cumsum_device (test_gpu_parity.py) on the phase, relative to the amplitude, and the elementwise kernels' 1e-14
        bound = 4e-16 * max_phase * math.log2(n + 2) + 1e-14
        err = float(np.max(np.abs(got.astype(np.clongdouble) - want)) / np.max(np.abs(want)))
        margins.record(f"LASER {'+'.join(kw)} n={n}", None, err, bound)
        assert err <= bound


# ============================================================================================ 3. PRBS far from the start
def shift_map(order):
    """The one-shift map over GF(2) as a 0 / 1 matrix, column i = the oracle's state after one shift of the basis state e_i: a route to M
    that shares nothing with shift_matrix / mat_mul of prbs.hip."""
    from oracle import prbs_numpy as po
    M = np.zeros((order, order), np.int64)
    for i in range(order):
        _, state = po.prbs(order, 1, 1 << i)
        M[:, i] = (state >> np.arange(order)) & 1
    return M


def host_jump(order, steps, state):
    """M^steps applied to `state`: square and multiply in NumPy, mod 2."""
    P = shift_map(order)
    v = ((int(state) >> np.arange(order)) & 1).astype(np.int64)
    while steps:
        if steps & 1:
            v = (P @ v) % 2
        P = (P @ P) % 2
        steps >>= 1
    return int(np.sum(v << np.arange(order)))


def test_host_jump_is_the_oracle_walk():
    from oracle import prbs_numpy as po
    for order, steps, seed in ((7, 300, 0x55), (23, 5000, 0x2A5A5), (31, 4097, 0x12345678)):
        assert host_jump(order, steps, seed) == po.prbs(order, steps, seed)[1]


def test_prbs23_beyond_its_period_and_2_24():
    from oracle import prbs_numpy as po
    order, length, seed = 23, 2 ** 24 + 3000, 0x2A5A5
    period = 2 ** 23 - 1
    bits, last = _lib.prbs_device(order, length, seed, DEV)
    keep(bits)
    a, b = download(bits, period, length - period), download(bits, 0, length - period)
    assert a.size == 2 ** 23 + 3001 and a.max() <= 1
    np.testing.assert_array_equal(a, b)                              # the sequence repeats after 2^23 - 1 bits, and not sooner:
    assert not np.array_equal(a[: 2 ** 22], download(bits, period - 2 ** 22, 2 ** 22))
    np.testing.assert_array_equal(b[:4096], po.prbs(order, 4096, seed)[0])
    assert last == host_jump(order, length, seed) == host_jump(order, length - 2 * period, seed)
    at = length - 4096
    want, state = po.prbs(order, 4096, host_jump(order, at, seed))
    np.testing.assert_array_equal(a[-4096:], want)
    assert state == last


def test_prbs31_at_2_27_uses_every_power_up_to_26():
    from oracle import prbs_numpy as po
    order, length, seed = 31, 2 ** 27 + 77, 0x5EEDBEEF & (2 ** 31 - 1)
    bits, last = _lib.prbs_device(order, length, seed, DEV)
    keep(bits)
    assert last == host_jump(order, length, seed)
    at = length - 4096
    want, state = po.prbs(order, 4096, host_jump(order, at, seed))
    np.testing.assert_array_equal(download(bits, at, 4096), want)
    assert state == last
    for k in range(18, 27):                                          # around 2^k chunks of 256 bits: where M^(2^k) is used alone for the first time
        for pos in (2 ** k - 2048, 2 ** 27 - 2 ** k - 2048):         # ... and where every power above k is used together
            want, _ = po.prbs(order, 4096, host_jump(order, pos, seed))
            np.testing.assert_array_equal(download(bits, pos, 4096), want, err_msg=f"bits from {pos}")


def test_prbs7_keeps_its_period_up_to_2_26():
    from oracle import prbs_numpy as po
    order, length = 7, 2 ** 26 + 1
    one, _ = po.prbs(order, 127)
    bits, last = _lib.prbs_device(order, length, 127, DEV)
    keep(bits)
    step = 1021                                                      # prime, coprime to 127: the sample walks through every phase
    count = (length - 1) // step + 1
    idx = np.arange(count) * step
    got = _lib.bits_slice_device(bits, 0, step, count).to_host()
    np.testing.assert_array_equal(got, one[idx % 127])
    tail = download(bits, length - 5000, 5000)
    np.testing.assert_array_equal(tail, one[np.arange(length - 5000, length) % 127])
    assert last == po.prbs(order, length % 127)[1]


# ============================================================================================ 4. the chirp
CHIRP_N = [2, 3, 127, 128, 129, 65537, 2 ** 20 + 1, 2 ** 21 + 1]     # grid: 4096 x 256 = 2^20 per sweep; 2^21 + 1 starts a third one


@pytest.mark.parametrize("n", CHIRP_N)
@pytest.mark.parametrize("conj", [False, True])
def test_chirp_every_element(n, conj):
    got = _lib.chirp_device(n, conj, DEV).to_host()
    assert got.shape == (n,) and got.dtype == np.complex128
    m = np.arange(n, dtype=np.uint64)
    r = (m * m) % np.uint64(2 * n)                                   # m^2 < 2^43: exact in uint64
    ang = ph.PI_LD * r.astype(LD) / LD(n)
    want_re, want_im = np.cos(ang), (np.sin(ang) if conj else -np.sin(ang))
    err = np.maximum(np.abs(got.real.astype(LD) - want_re), np.abs(got.imag.astype(LD) - want_im)).astype(np.float64)
    # sincospi's documented limit, in units of 2^-53 (|values| <= 1).  The kernel's one rounding of r / n (an argument below 2) spends up to
    # pi of these 4 units on its own: 3.3 measured at n = 2^21 + 1, 0.5 at n = 128 where the quotient is exact
    bound = E_SINCOS * U
    k = int(np.argmax(err))
    margins.record(f"chirp n={n} conj={int(conj)} (m={k})", None, err[k], bound)
    print(f"chirp n={n} conj={conj}: worst |d| = {err[k] / U:.3f} x 2^-53 at m = {k}")
    assert err[k] <= bound
    # whole quarter turns are exact: +-1 or +-i, the other part a zero
    sgn = 1.0 if conj else -1.0
    for r4, val in ((0, 1 + 0j), (1, sgn * 1j), (2, -1 + 0j), (3, -sgn * 1j)):
        if (r4 * n) % 2:
            continue
        at = np.nonzero(r == np.uint64(r4 * n // 2))[0]
        assert np.all(got[at] == val), (r4, at[:5])
    assert np.count_nonzero(r == 0) >= 1


# ============================================================================================ 5. the loaders past their grid cap
PLAN_N = 2 ** 21                                                     # the loaders' grid: 4096 x 256 = 2^20 items per sweep


def read_field(plan, count):
    out = keep(_lib.DeviceArray((count,), np.complex128, DEV))
    plan.copy_from_field(0, out.ptr, count * 16)
    return out.to_host()


def values(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    x[rng.random(n) < 0.01] = -0.0
    return x


def device_pulse(plan, spec):
    npts = spec[0][1]
    plan.load_pulse(*spec[0])
    h = read_field(plan, PLAN_N)
    assert not h[npts:].any()                                        # zero-padded
    return (h if spec[1] else h.real)[:npts], h[:npts].imag


PULSE_GRIDS = [(65600, 16), (2 ** 21 // 9 - 1, 9)]                   # span * sps + 1 = 2^20 + 1025 and 2^21 - 16 points


@pytest.mark.parametrize("span,sps", PULSE_GRIDS)
def test_pulses_past_the_first_sweep(span, sps):
    from oracle import transmitter_numpy as tx
    assert 2 ** 20 < span * sps + 1 <= PLAN_N
    plan = od.get_plan(PLAN_N, 1, _lib.C128, DEV)
    for T in (1, 2):
        got, im = device_pulse(plan, od._nrz_spec(span, sps, T))
        np.testing.assert_array_equal(got, tx.nrz_pulse(span, sps, T))
        assert not im.any()
    for T, m, c in ((2, 1, 0.5), (1, 2, 0.0)):
        got, _ = device_pulse(plan, od._gauss_spec(span, sps, T=T, m=m, c=c))
        want = tx.gauss_pulse(span, sps, T=T, m=m, c=c)
        mag = np.abs(want)                                           # the bound of test_device_pulses_match_the_reference_expressions
        assert np.all(np.abs(got - want) <= 4e-16 * (2 + np.abs(np.log(mag + 1e-320))) * mag + 1e-300)
    for beta, shape in ((0.0, "normal"), (0.25, "normal"), (1 / 3, "sqrt")):
        got, im = device_pulse(plan, od._rcos_spec(beta, span, sps, shape))
        np.testing.assert_allclose(got, tx.rcos_pulse(beta, span, sps, shape), rtol=1e-12, atol=1e-13)
        assert not im.any()


def stuffed(sym, up_):
    want = np.zeros(PLAN_N, np.complex128)
    want[up_ // 2 + up_ * np.arange(sym.size)] = sym
    return want


@pytest.mark.parametrize("up_", [1, 2, 7, 16])
def test_load_symbols_and_bits_past_the_first_sweep(up_):
    plan = od.get_plan(PLAN_N, 1, _lib.C128, DEV)
    full = PLAN_N // up_                                             # nsym * up == 2^21 where up divides it, the largest below otherwise
    for nsym in (full, (2 ** 20 + 5) // up_ + 1, full - 3):
        assert 2 ** 20 < nsym * up_ <= PLAN_N
        sym = values(nsym, nsym + up_)
        plan.load_symbols(up(sym), up_)
        same_bits(read_field(plan, PLAN_N), stuffed(sym, up_))       # the amplitudes where they belong, +0.0 everywhere else
        bits = np.random.default_rng(nsym).integers(0, 2, nsym, dtype=np.uint8)
        plan.load_bits(up(bits), up_)
        same_bits(read_field(plan, PLAN_N), stuffed(bits.astype(np.float64), up_))
    with pytest.raises(_lib.SsfmError):
        plan.load_bits(up(np.ones(full + 1, np.uint8)), up_)


@pytest.mark.parametrize("count", [1, 2 ** 20 + 1, PLAN_N])
@pytest.mark.parametrize("cplx", [False, True])
def test_load_padded_past_the_first_sweep(count, cplx):
    plan = od.get_plan(PLAN_N, 1, _lib.C128, DEV)
    plan.load_symbols(up(np.full(PLAN_N, 7.0)), 1)                   # something to overwrite: the padding must be written, not left
    src = values(2 * count, count).view(np.complex128) if cplx else values(count, count)
    want = np.zeros(PLAN_N, np.complex128)
    want[:count] = src
    plan.load_padded(up(src))
    same_bits(read_field(plan, PLAN_N), want)
    if count > 1:                                                    # the first `count - 1` values of a longer array
        plan.load_padded(up(src), count - 1)
        want[count - 1] = 0
        same_bits(read_field(plan, PLAN_N), want)


@pytest.mark.parametrize("nsym,sps", [(2 ** 16, 16), (2 ** 16 - 3, 16), (2 ** 20 // 7, 7)])
def test_load_qpsk_two_rows_past_the_first_sweep(nsym, sps):
    n = 2 ** 20                                                      # 2 rows x 2^20 items = two sweeps
    plan = od.get_plan(n, 2, _lib.C128, DEV)
    bits = np.random.default_rng(nsym).integers(0, 2, 4 * nsym, dtype=np.uint8)
    plan.load_qpsk(up(bits), nsym, sps)
    b = bits.astype(np.float64).reshape(2, nsym, 2)
    want = np.zeros((2, n), np.complex128)
    at = sps // 2 + sps * np.arange(nsym)
    want.real[:, at] = (2.0 * b[..., 0] - 1.0) / 1.4142135623730951
    want.imag[:, at] = (2.0 * b[..., 1] - 1.0) / 1.4142135623730951
    same_bits(read_field(plan, 2 * n), want.ravel())
