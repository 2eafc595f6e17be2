"""The data-aided receiver on the MI355X (csrc/sync.hip): the peak reduction alone, the FFT correlation against a direct longdouble sum,
lab.SYNC and lab.GET_EYE_v2 against the NumPy restatement tests/sync_numpy.py and the reference's fixtures, and the residency of both."""

import numpy as np
import pytest

import opticomlib_amd as oa
import sync_numpy as sn
from opticomlib_amd import _lib, lab
from opticomlib_amd.typing import NULL, binary_sequence, electrical_signal, gv
from test_sync_cpu import EMPTY, EYE_GOLDEN, SYNC_GOLDEN, load_case, name_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


# ------------------------------------------------------------------------------------------------ the peak kernel alone
WAVE, GROUP, GRID = 64, 256, 480 * 256                          # a wavefront, a workgroup, the largest grid of the reduction


def peak(x, stride=1):
    d = _lib.DeviceArray.from_host(x, None)
    out = np.zeros(4)
    _lib.api.ssfm_sync_peak(d, stride, x.size, _lib._ptr(out), out.size)
    return out


@pytest.mark.parametrize("n", [1, 2, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, 5 * GROUP + 1, GRID + 1, 3 * GRID + 77])
def test_peak_statistics_at_every_size(n):
    x = np.random.default_rng(n).standard_normal(n)
    mx, arg, mean, std = peak(x)
    assert mx == x.max() and arg == int(np.argmax(x))
    # two float64 sums of n values in tree-like orders: each within eps (log2 n + 2) mean|x| of the exact mean
    assert abs(mean - x.mean()) <= 2 * np.finfo(float).eps * (np.log2(n) + 2) * np.abs(x).mean()
    assert abs(std - x.std()) <= 1e-12 * max(x.std(), np.finfo(float).tiny)


def test_peak_reads_the_real_parts_of_a_complex_array():
    rng = np.random.default_rng(5)
    z = rng.standard_normal(1000) + 1j * (10 + rng.standard_normal(1000))
    mx, arg, mean, std = peak(z, stride=2)
    assert mx == z.real.max() and arg == int(np.argmax(z.real))
    assert abs(std - z.real.std()) <= 1e-12 * z.real.std()


@pytest.mark.parametrize("n", [GROUP + 1, 5 * GROUP + 1, GRID + 1])
@pytest.mark.parametrize("where", ["first", "last", "pair", "lanes", "groups"])
def test_exact_ties_give_the_first_index(n, where):
    x = np.random.default_rng(1).uniform(-1, 0.5, n)
    at = {"first": [0, n // 2, n - 1], "last": [n - 1], "pair": [n // 3, n // 3 + 1], "lanes": [70, 70 + WAVE], "groups": [GROUP - 1, n - 2]}[where]
    x[at] = 1.0
    mx, arg, _, _ = peak(x)
    assert mx == 1.0 and arg == at[0] == int(np.argmax(x))


@pytest.mark.parametrize("n", [1, 3, GROUP + 1, 5 * GROUP + 1])
@pytest.mark.parametrize("value", [0.1, -3.3e7, 0.0])
def test_equal_values_have_a_std_of_exactly_zero(n, value):
    mx, arg, mean, std = peak(np.full(n, value))
    assert (mx, arg, mean, std) == (value, 0, value, 0.0)


def test_a_nan_is_the_maximum_as_in_numpy():
    x = np.random.default_rng(2).standard_normal(5 * GROUP + 1)
    x[[700, 900]] = np.nan
    x[10] = np.inf
    mx, arg, mean, std = peak(x)
    assert np.isnan(mx) and arg == 700 == int(np.argmax(x)) and np.isnan(mean) and np.isnan(std)
    assert not (mx < 3 * std)                                   # the reference's comparison is false: no ValueError, i = the first NaN


@pytest.mark.parametrize("n", [GROUP + 1, 100_003])
def test_std_on_a_large_mean_is_two_pass(n):
    x = 1e6 + np.random.default_rng(3).standard_normal(n)
    one_pass = np.sqrt(abs(np.mean(x * x) - np.mean(x) ** 2))
    _, _, mean, std = peak(x)
    print(f"n={n}: std {std!r}, np.std {x.std()!r}, one-pass {one_pass!r}")
    assert abs(std - x.std()) <= 1e-12 * x.std()
    assert abs(one_pass - x.std()) > 1e-12 * x.std()            # the form the kernel must not use misses this bound


# ------------------------------------------------------------------------------------------------ the correlation
def device_corr(rx, bits, sps):
    l = bits.size * sps
    W = min(rx.size, 2 * l)
    nc = W - l + 1
    M = 1 << max(8, (W - 1).bit_length())
    x = _lib.DeviceArray.from_host(rx, np.float64)
    b = _lib.DeviceArray.from_host(bits.astype(np.uint8), np.uint8)
    plan = oa.devices.get_plan(M, 1, _lib.C128, 0)
    out = _lib.DeviceArray((nc,), np.complex128, 0)
    with plan.lock:
        lab._correlate(plan, x, b, sps, W)
        plan.copy_from_field(0, out.ptr, nc * 16)
    return out.to_host().real


def prbs_like(nbits, seed):
    return np.random.default_rng(seed).integers(0, 2, nbits).astype(np.uint8)


CORR_CASES = [(127, 8, 2.0), (127, 8, 1.37), (511, 16, 2.0), (511, 16, 1.61), (127, 16, 2.0), (127, 16, 1.05)]


@pytest.mark.parametrize("nbits,sps,window", CORR_CASES)
def test_correlation_error_against_a_direct_sum(nbits, sps, window):
    """The device's error may be at most 4 x SciPy's on the same input (another transform length and radix), both against the direct
    np.longdouble correlation and normalised by max|corr|.  The measured pairs are kept in profiles/sync_margins.txt."""
    rng = np.random.default_rng(nbits * sps)
    bits = prbs_like(nbits, nbits + sps)
    l = nbits * sps
    n = int(round(window * l))
    rx = np.roll(np.tile(sn.template(bits, sps), 3), 3 * sps + 1)[:n] + 0.7 + rng.normal(0, 0.1, n)      # a DC offset plus noise
    direct = sn.correlation_direct(rx, bits, sps)
    scale = float(np.max(np.abs(direct)))
    e_dev = float(np.max(np.abs(device_corr(rx, bits, sps) - direct))) / scale
    e_sci = float(np.max(np.abs(sn.correlation(rx, bits, sps) - direct))) / scale
    print(f"SYNC_MARGIN l={l} W={min(n, 2 * l)} nc={direct.size} device {e_dev:.3e} scipy {e_sci:.3e} ratio {e_dev / e_sci:.2f}")
    assert direct.size == min(n, 2 * l) - l + 1
    assert e_dev <= 4 * e_sci


# ------------------------------------------------------------------------------------------------ SYNC end to end
def check_sync(rx, bits, sps, as_signal=False):
    """lab.SYNC against the restatement: the exact i, the slice bit for bit, no noise -- or the same refusal."""
    r = None
    try:
        r = sn.sync(rx, bits, sps)
    except ValueError as e:
        with pytest.raises(ValueError, match=str(e)):
            lab.SYNC(rx, bits, sps)
        return None
    if r["signal"].size == 0:
        with pytest.raises(ValueError, match=EMPTY.replace("(", r"\(").replace(")", r"\)")):
            lab.SYNC(rx, bits, sps)
        return r
    if as_signal:
        gv(sps=sps, R=1e9)
        out, i = lab.SYNC(electrical_signal(rx), binary_sequence(bits))
    else:
        out, i = lab.SYNC(rx, bits, sps)
    assert i == r["i"] and isinstance(i, int)
    assert isinstance(out, electrical_signal) and out.on_device and out._raw("noise") is NULL
    np.testing.assert_array_equal(out.signal, r["signal"])
    assert out.noise is NULL
    return r


@pytest.mark.parametrize("path", SYNC_GOLDEN, ids=name_of)
def test_sync_on_the_reference_fixtures(path):
    g = load_case(path)
    if g["raises"]:
        with pytest.raises(ValueError, match=g["message"].replace("(", r"\(").replace(")", r"\)")):
            lab.SYNC(g["rx"], g["tx"], g["sps"])
        return
    out, i = lab.SYNC(g["rx"], g["tx"], g["sps"])
    assert i == g["i"] and out.noise is NULL
    np.testing.assert_array_equal(out.signal, g["signal"])
    check_sync(g["rx"], g["tx"], g["sps"], as_signal=True)


def draw_record(rng, forced_delay=None):
    sps = int(rng.choice([2, 8, 16, 64]))
    nbits = int(rng.integers(31, 2048))
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    tx = sn.template(bits, sps)
    l = tx.size
    delay = {None: int(rng.integers(0, l + 1)), "l-1": l - 1, "l": l}.get(forced_delay, forced_delay)
    if rng.random() < 0.5 and 0 < delay < l:                    # a periodic record
        rx = np.roll(np.tile(tx, 3), delay)[: l + int(rng.integers(l, 2 * l + 1))]
    else:                                                       # not periodic: other traffic, the word once, other traffic (lag 0 and lag l are peaks of their own)
        other = lambda m: np.repeat(rng.integers(0, 2, m // sps + 1), sps)[:m].astype(float)      # noqa: E731
        rx = np.concatenate([other(delay), tx, other(int(rng.integers(l - delay, 2 * l)))])
    rx = rx * rng.uniform(0.2, 3) + rng.uniform(0, 0.3) + rng.normal(0, 0.05, rx.size)
    return rx, bits, sps, delay


def test_sync_against_the_restatement_on_random_records():
    rng = np.random.default_rng(2024)
    forced = [1, 5, "l-1", "l", 0] * 2 + [None] * 14
    drawn = discarded = 0
    for k, f in enumerate(forced):
        while True:
            rx, bits, sps, delay = draw_record(rng, f)
            drawn += 1
            if sn.margin(sn.correlation(rx, bits, sps)) >= 1e-3:
                break
            discarded += 1                                      # the largest lag does not stand clear of the runner-up: redraw
        r = check_sync(rx, bits, sps, as_signal=bool(k % 2))
        assert r is not None and r["i"] == delay, (k, sps, bits.size, delay)
    print(f"{drawn} records drawn, {discarded} discarded")
    assert discarded <= 0.1 * drawn


def test_an_inverted_record_has_no_maximum():
    bits = prbs_like(127, 7)
    rx = -np.tile(sn.template(bits, 8), 3)
    c = sn.peak_stats(sn.correlation(rx, bits, 8))
    assert c["max"] < 3 * c["std"]
    with pytest.raises(ValueError, match="No correlation maximum found!!"):
        lab.SYNC(rx, bits, 8)


def test_the_slice_keeps_its_quirks():
    """len(rx) == l and i == l select nothing: the reference's constructor refuses the empty slice (fixtures sync_sps8_exact_length and
    sync_sps16_last_lag), and so does this one."""
    bits = prbs_like(127, 8)
    tx = sn.template(bits, 8)
    rng = np.random.default_rng(9)
    exact = tx + rng.normal(0, 0.05, tx.size)
    last = np.concatenate([np.zeros(tx.size), tx, np.zeros(40)]) + rng.normal(0, 0.05, 2 * tx.size + 40)
    assert sn.sync(exact, bits, 8)["signal"].size == 0
    assert sn.sync(last, bits, 8)["i"] == tx.size and sn.sync(last, bits, 8)["signal"].size == 0
    for rx in (exact, last):
        with pytest.raises(ValueError, match=EMPTY.replace("(", r"\(").replace(")", r"\)")):
            lab.SYNC(rx, bits, 8)
    out, i = lab.SYNC(last[1:], bits, 8)                        # one lag earlier: a record again
    assert i == tx.size - 1
    np.testing.assert_array_equal(out.signal, last[1:][i:-1])


def test_a_window_that_is_no_multiple_of_anything():
    bits = prbs_like(127, 11)
    tx = sn.template(bits, 8)
    rx = np.roll(np.tile(tx, 2), 200)[:1525] + np.random.default_rng(4).normal(0, 0.05, 1525)
    r = check_sync(rx, bits, 8)
    assert r["corr"].size == 510 and r["i"] == 200


def test_the_largest_plan_and_one_sample_beyond():
    _, hi = _lib.supported_log2n(_lib.C128, direct=True)
    sps, nbits = 64, (1 << hi) // 128                           # l = 2^(hi - 1): a window of exactly 2^hi samples
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    tx = sn.template(bits, sps)
    delay = 123_457
    rx = np.concatenate([np.zeros(delay), tx, np.zeros(tx.size - delay)]) + rng.normal(0, 0.05, 2 * tx.size)
    assert rx.size == 1 << hi
    out, i = lab.SYNC(rx, bits, sps)
    assert i == delay
    np.testing.assert_array_equal(out.signal, rx[delay:delay + tx.size])
    with pytest.raises(ValueError, match="exceeds the device path"):
        lab.SYNC(np.zeros(2 * (nbits + 1) * sps), np.append(bits, 1).astype(np.uint8), sps)


# ------------------------------------------------------------------------------------------------ GET_EYE_v2
def known_eye(seed, sps, nbits, bits=None, sigma=0.05):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, nbits).astype(np.uint8) if bits is None else np.asarray(bits, dtype=np.uint8)
    lo, hi = 0.1, 1.3
    x = np.repeat(lo + (hi - lo) * bits, sps).astype(float)
    k = np.arange(-2 * sps, 2 * sps + 1)
    h = np.exp(-0.5 * (k / (0.2 * sps)) ** 2)
    x = np.convolve(x, h / h.sum(), mode="same")
    x = x[: x.size - int(rng.integers(0, sps))]                 # odd lengths
    return x, (rng.normal(0, sigma, x.size) if sigma else None), bits


def check_eye_v2(e, r):
    span = r["mu1"] - r["mu0"]
    for k in ("mu0", "mu1", "s0", "s1"):
        assert abs(getattr(e, k) - r[k]) <= 1e-12 * abs(span), (k, getattr(e, k), r[k])
    assert abs(e.threshold - r["threshold"]) <= abs(span) / 499 * (1 + 1e-9)
    for k in ("i", "sps", "t_left", "t_right", "t_dist", "t_opt", "t_span0", "t_span1", "y_left", "y_right"):
        assert getattr(e, k) == r[k], k
    # eye_h = mu1 - 3 s1 - mu0 - 3 s0 and er = 10 log10(mu1 / mu0) of moments within 1e-12 of the span
    assert abs(e.eye_h - r["eye_h"]) <= 8e-12 * abs(span)
    assert abs(e.er - r["er"]) <= 10 / np.log(10) * 1e-12 * abs(span) * (1 / abs(r["mu1"]) + 1 / abs(r["mu0"])) * (1 + 1e-3)
    for k in ("y", "ones", "zeros", "t", "t0", "t1"):
        np.testing.assert_array_equal(getattr(e, k), r[k], err_msg=k)


@pytest.mark.parametrize("path", EYE_GOLDEN, ids=name_of)
def test_eye_v2_on_the_reference_fixtures(path):
    g = load_case(path)
    gv(sps=g["sps"], R=float(g["R"]))
    sig = electrical_signal(g["x"], g["noise"]) if g["noise"].size else electrical_signal(g["x"])
    e = lab.GET_EYE_v2(sig, binary_sequence(g["tx"]), nslots=g["nslots"])
    span = float(g["mu1"] - g["mu0"])
    for k in ("mu0", "mu1", "s0", "s1"):
        assert abs(getattr(e, k) - float(g[k])) <= 1e-12 * span, k
    assert abs(e.threshold - float(g["threshold"])) <= span / 499 * (1 + 1e-9)
    for k in ("y", "ones", "zeros"):
        np.testing.assert_array_equal(getattr(e, k), g[k], err_msg=k)
    assert e.i == int(g["i"]) and e.t0.size == int(g["t0_size"]) and e.t1.size == int(g["t1_size"])


@pytest.mark.parametrize("sps,per_slot", [(8, 1), (16, 1), (32, 3), (64, 7)])
@pytest.mark.parametrize("nslots", ["below", "equal", "above"])
@pytest.mark.parametrize("noisy", [False, True])
def test_eye_v2_against_the_restatement(sps, per_slot, nslots, noisy):
    x, noise, bits = known_eye(sps * 7 + noisy, sps, 301, sigma=0.05)
    gv(sps=sps, R=1e9)
    avail = (x.size - x.size % (2 * sps)) // sps
    ns = {"below": 130, "equal": avail, "above": 4096}[nslots]
    tg = np.linspace(-0.5, 0.5, sps, endpoint=False)
    assert int(((tg > -0.05) & (tg < 0.05)).sum()) == per_slot
    if noisy:
        sig, total = electrical_signal(x, noise), x + noise
    else:
        sig, total = electrical_signal(x + noise), x + noise        # the same samples as one array
    r = sn.get_eye_v2(total, bits, sps, ns)
    e = lab.GET_EYE_v2(sig, bits, ns)
    check_eye_v2(e, r)
    assert e.ones.size + e.zeros.size == min(ns, avail) * sps
    # the same from device-resident inputs
    dsig = oa.devices._wrap_out(electrical_signal, _lib.DeviceArray.from_host(sig.signal, np.float64),
                                _lib.DeviceArray.from_host(sig.noise, np.float64) if noisy else NULL)
    dbits = binary_sequence.from_device(_lib.DeviceArray.from_host(bits, np.uint8))
    check_eye_v2(lab.GET_EYE_v2(dsig, dbits, ns), r)


@pytest.mark.parametrize("lone", [0, 1])
def test_eye_v2_with_one_slot_of_a_level(lone):
    sps, nbits = 32, 600                                        # three span samples per slot: the lone slot gives its level three
    bits = np.full(nbits, 1 - lone, dtype=np.uint8)
    bits[417] = lone
    x, noise, bits = known_eye(31 + lone, sps, nbits, bits=bits)
    gv(sps=sps, R=1e9)
    r = sn.get_eye_v2(x + noise, bits, sps)
    e = lab.GET_EYE_v2(electrical_signal(x, noise), bits)
    check_eye_v2(e, r)
    assert (e.ones if lone else e.zeros).size == sps


def test_eye_v2_without_noise_in_the_signal():
    x, _, bits = known_eye(77, 16, 200, sigma=0)
    gv(sps=16, R=1e9)
    check_eye_v2(lab.GET_EYE_v2(x, bits, 4096), sn.get_eye_v2(x, bits, 16))


def test_eye_v2_refuses_what_the_reference_refuses():
    gv(sps=8, R=1e9)
    x, noise, bits = known_eye(1, 8, 64)
    with pytest.raises(IndexError, match="boolean index did not match"):
        lab.GET_EYE_v2(x, bits[:40])
    with pytest.raises(IndexError):
        sn.get_eye_v2(x, bits[:40], 8)
    flat = np.full(64 * 8, 0.5)
    with pytest.raises(np.linalg.LinAlgError):
        lab.GET_EYE_v2(flat, bits)
    with pytest.raises(np.linalg.LinAlgError):
        sn.get_eye_v2(flat, bits, 8)


# ------------------------------------------------------------------------------------------------ residency
def test_device_resident_inputs_are_used_where_they_lie():
    gv(sps=16, R=1e9, N=381)
    word, tx = oa.PRBS(order=7), oa.PRBS(order=7, len=381)      # the word, and three periods of it
    drive = oa.DAC(tx, Vpp=5.0, offset=-2.5, pulse_shape="gaussian")
    field = oa.MZM(oa.LASER(P0=1e-3), drive, bias=-2.5, Vpi=5.0, loss_dB=3, ER_dB=20)
    pd = oa.PD(field, BW=0.75 * gv.R, r=1.0, include_noise="all")
    record = pd[37:]                                            # a device-side slice: the word now starts 37 samples before a period
    assert record.on_device and word._raw().__class__ is _lib.DeviceArray
    before = dict(_lib.TRANSFERS)
    synced, i = lab.SYNC(record, word)
    assert dict(_lib.TRANSFERS) == before and synced.on_device
    e = lab.GET_EYE_v2(synced, tx)
    assert dict(_lib.TRANSFERS) == before
    off = (i + 37) % (127 * 16)                                 # the start of a period: the pulses are centred in their slots and the
    assert min(off, 127 * 16 - off) <= 2                        # detector's filter has no delay, so at most the half-sample of an even sps
    assert e.mu1 > e.mu0 and e.s0 >= 0 and e.s1 >= 0
    n = e.ones.size + e.zeros.size                              # the first reads download
    assert n == e.y.size and _lib.TRANSFERS["d2h"] == before["d2h"] + 3 and _lib.TRANSFERS["h2d"] == before["h2d"]
