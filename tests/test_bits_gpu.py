"""The binary_sequence algebra on the MI355X: every fixture again with the operands uploaded first (results exact and device-resident, nothing
read back before the result is), a sweep against live NumPy at the sizes where a 16-byte-per-lane kernel of 256-thread workgroups can go wrong
(none, one byte, around one vector, one wavefront, one workgroup, many workgroups), once above the grid cap (2048 workgroups x 256 lanes x 16
bytes = 8 MiB, from where a lane takes a second turn of its grid-stride loop), every destination and source offset modulo 16, tiles of odd
periods, empty sequences, bytes that are not 0 / 1, determinism of the integer reductions, residency, and a chain without host transfers.
Everything here is integers and compared exactly, except ``dac``: 1e-12 of the peak, ``filter``'s bound (the same convolution on the same plan)."""
import numpy as np
import pytest
import scipy.signal as sg

import bits_cases as bc
from opticomlib_amd import PRBS, _lib, binary_sequence, electrical_signal, gv
from test_bits_cpu import CASES, expected, load_group, load_namespace, mismatch

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 65535 * 16 + 1, (1 << 20) + 1)


def up(bits, device=0):
    return binary_sequence.from_device(_lib.DeviceArray.from_host(np.ascontiguousarray(bits, dtype=np.uint8), np.uint8, device))


def dev(x):
    return up(x.data)


def rand_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def read(x):
    """The bits of a device-resident result, which must be one."""
    assert isinstance(x, binary_sequence) and isinstance(x._raw(), _lib.DeviceArray), x
    got = x._raw().to_host()
    assert got.dtype == np.uint8 and got.ndim == 1
    return got


@pytest.mark.parametrize("group", bc.GROUPS)
def test_device_path_matches_the_reference(group):
    fix, v = load_group(group), load_namespace(dev)
    bad = []
    for cid, fn in CASES:
        g, name = cid.split("/", 1)
        if g != group:
            continue
        before = _lib.TRANSFERS["d2h"]
        try:
            r = fn(v)
        except Exception as e:                   # noqa: BLE001  (the exception is the outcome that is compared)
            r = e
        if group not in bc.HOST_RESULT:
            assert _lib.TRANSFERS["d2h"] == before, cid                     # nothing is read back until the result is
            if isinstance(r, binary_sequence):
                assert isinstance(r._raw(), _lib.DeviceArray), cid
            if isinstance(r, electrical_signal):
                assert r.on_device, cid
            if isinstance(r, (int, np.integer)):
                assert type(r) is int, (cid, type(r))
            assert all(x.on_device for k, x in v.items() if k in bc.SEQUENCES), cid         # the operands stay where they are
        why = mismatch(expected(fix, name), bc.describe(r))
        if why:
            bad.append((cid, why))
    gv.default()
    assert not bad, bad[:10]


@pytest.mark.parametrize("n", SIZES)
def test_sweep_against_numpy(n):
    a, b = rand_bits(n, 1000 + n), rand_bits(n, 2000 + n)
    da, db = up(a), up(b)
    before = _lib.TRANSFERS["d2h"]
    results = {"~": ~da, "&": da & db, "|": da | db, "^": da ^ db, "!=": da != db, "flip": da.flip(), "*": da * db}
    counts = {"ones": da.ones, "zeros": da.zeros, "hamming": da.hamming_distance(db), "hamming_self": da.hamming_distance(da)}
    assert _lib.TRANSFERS["d2h"] == before
    want = {"~": 1 - a, "&": a & b, "|": a | b, "^": a ^ b, "!=": a ^ b, "flip": 1 - a, "*": a & b}
    for k, r in results.items():
        assert np.array_equal(read(r), want[k]), (k, n)
    assert counts == {"ones": int(a.sum()), "zeros": n - int(a.sum()), "hamming": int((a ^ b).sum()), "hamming_self": 0}
    assert all(type(c) is int for c in counts.values())
    if n:                                        # one bit against n, either order, a device or a host bit
        for bit in (0, 1):
            one = up([bit])
            assert np.array_equal(read(da & one), a & bit) and np.array_equal(read(one | da), a | bit) and np.array_equal(read(da ^ bit), a ^ bit)
            assert da.hamming_distance(one) == one.hamming_distance(da) == int((a ^ bit).sum())
        assert da[n - 1] == int(a[-1]) and da[-n] == int(a[0]) and type(da[0]) is int
        with pytest.raises(IndexError):
            da[n]
    assert da.on_device and db.on_device


def test_above_the_grid_cap():
    """Results of more than 8 MiB: every kernel's lanes go round their grid-stride loop a second time (the tile's lanes advance their position
    in the period there; the strided gather's cap is 2048 x 256 bytes)."""
    n = (1 << 23) + 4097 + 3
    a, b = rand_bits(n, 23), rand_bits(n, 24)
    da, db = up(a), up(b)
    assert np.array_equal(read(~da), 1 - a) and np.array_equal(read(da ^ db), a ^ b)
    assert da.ones == int(a.sum()) and da.zeros == n - int(a.sum()) and da.hamming_distance(db) == int((a ^ b).sum())
    assert np.array_equal(read(da[3:]), a[3:]) and np.array_equal(read(da[::-1]), a[::-1]) and np.array_equal(read(da[5::3]), a[5::3])
    assert np.array_equal(read(da[7:] + db[:11]), np.concatenate((a[7:], b[:11])))
    for period, reps in ((4097, 2100), (7, 1300000), (65537, 130)):
        w = a[:period]
        assert np.array_equal(read(up(w) * reps), np.tile(w, reps)), (period, reps)
    shifted = da[1:] * 2                          # a tile whose source and destination are both off the 16-byte grid is the same kernel: its source is a fresh array
    assert np.array_equal(read(shifted), np.tile(a[1:], 2))


def test_empty_sequences():
    e, a = up([]), up([1, 0, 1])
    assert e.size == 0 and e.on_device and e.ones == 0 and e.zeros == 0 and e.hamming_distance(e) == 0 and e.hamming_distance(1) == 0
    for r, want in ((e + e, []), (e + a, [1, 0, 1]), (a + e, [1, 0, 1]), (~e, []), (e & e, []), (e ^ 1, []), (up([1]) | e, []), (e * 3, []), (e[::2], []),
                    (a[5:], []), (a[5:] + a, [1, 0, 1])):
        assert list(read(r)) == want
    c = e._raw().copy()
    assert c.size == 0 and c.to_host().shape == (0,) and e._raw().astype(np.uint8).size == 0
    with pytest.raises(ValueError, match="invalid shape"):
        e.dac(np.ones(3))
    with pytest.raises(ValueError, match="broadcast"):
        e & a


@pytest.mark.parametrize("len_b", (1, 16, 4099))
@pytest.mark.parametrize("len_a", (1, 3, 15, 16, 17, 4097))
def test_concatenation_at_every_destination_offset(len_a, len_b):
    a, b = rand_bits(len_a, 31 + len_a), rand_bits(len_b, 77 + len_b)
    da, db = up(a), up(b)
    assert np.array_equal(read(da + db), np.concatenate((a, b))) and np.array_equal(read(db + da), np.concatenate((b, a)))
    assert np.array_equal(read(da + list(b)), np.concatenate((a, b))) and np.array_equal(read(b + da), np.concatenate((b, a)))    # ndarray + a
    assert np.array_equal(read(da + db + da), np.concatenate((a, b, a)))


@pytest.mark.parametrize("reps", (2, 3, 1000))
@pytest.mark.parametrize("period", (1, 3, 7, 64, 127, 4097))
def test_tiles(period, reps):
    a = rand_bits(period, 500 + period)
    a[0] = 1
    assert np.array_equal(read(up(a) * reps), np.tile(a, reps)) and np.array_equal(read(reps * up(a)), np.tile(a, reps))


def test_slices():
    n = 4099
    a = rand_bits(n, 4099)
    da = up(a)
    before = _lib.TRANSFERS["d2h"]
    keys = [slice(k, None) for k in range(18)] + [slice(None, None, -1), slice(None, None, 3), slice(-5, 2, -2), slice(5, 5), slice(7, 4000), slice(-9000, 9000),
                                                   slice(5000, None), slice(None, None, -4098), slice(4098, None, 5)]
    got = [da[k] for k in keys]
    assert _lib.TRANSFERS["d2h"] == before and da.on_device
    for k, r in zip(keys, got):
        assert np.array_equal(read(r), a[k]), k
    # a slice of a slice reads at a misaligned source into an aligned destination, and logic on it reads two differently aligned sources
    assert np.array_equal(read(da[5:][3:1000] ^ da[1:998]), a[8:1005] ^ a[1:998])


def test_an_index_array_materialises_on_the_host():
    a = rand_bits(100, 5)
    da = up(a)
    r = da[np.arange(0, 100, 7)]
    assert isinstance(r, binary_sequence) and not r.on_device and np.array_equal(r.data, a[::7]) and not da.on_device      # as __getitem__ did before


def test_bytes_that_are_not_0_or_1_count_as_ones():
    raw = np.tile(np.array([0, 1, 2, 255], np.uint8), 10)[:37]
    a, b = (raw != 0).astype(np.uint8), rand_bits(37, 37)
    x = binary_sequence.from_device(_lib.DeviceArray.from_host(raw))
    db = up(b)
    assert x.ones == int(a.sum()) and x.zeros == 37 - int(a.sum()) and [x[i] for i in range(4)] == [0, 1, 1, 1]
    for r, want in ((~x, 1 - a), (x & db, a & b), (db | x, a | b), (x ^ db, a ^ b), (x != db, a ^ b), (x & 1, a), (x | 0, a), (x + db, np.concatenate((a, b))),
                    (db + x, np.concatenate((b, a))), (x * 3, np.tile(a, 3)), (x[1:], a[1:]), (x[::2], a[::2]), (x[::-1], a[::-1]), (x * db, a & b)):
        got = read(r)
        assert np.array_equal(got, want) and set(np.unique(got)) <= {0, 1}
    # hamming_distance of equal lengths is ssfm_device_count_diff, which compares bytes: a 2 or a 255 against a 1 is a difference there (the
    # documented exception); the mask's sum is the normalised count
    assert x.hamming_distance(up(a)) == int(np.count_nonzero(raw > 1)) == 18 and (x != up(a)).ones == 0


def test_reductions_give_the_same_integer_twice():
    a, b = up(rand_bits((1 << 20) + 1, 8)), up(rand_bits((1 << 20) + 1, 9))
    assert a.ones == a.ones and a.zeros == a.zeros and a.hamming_distance(b) == a.hamming_distance(b) == (a != b).ones


def test_the_operand_stays_on_the_device():
    a = up(rand_bits(100, 3))
    before = _lib.TRANSFERS["d2h"]
    a.ones, a.zeros, a[2:9], a[5], a.hamming_distance(a), ~a, a + a, a * 2, len(a), a.size, a.sizeof, repr(a), str(a)       # noqa: B018
    assert a.on_device and _lib.TRANSFERS["d2h"] == before
    assert "on GPU" in str(a) and a.print("title") is a and a.on_device


def test_operands_on_different_devices():
    if _lib.device_count() < 2:
        pytest.skip("one GPU is visible")
    a, b = up([1, 0, 1], 0), up([1, 1, 0], 1)
    for op in (lambda: a & b, lambda: a + b, lambda: a != b, lambda: a.hamming_distance(b), lambda: a * b):
        with pytest.raises(ValueError, match="different GPUs"):
            op()


def test_prbs_is_devices_prbs():
    s, last = binary_sequence.prbs(7, 300, 5, True)
    t, last2 = PRBS(7, 300, 5, True)
    assert s.on_device and last == last2 and s.hamming_distance(t) == 0 and np.array_equal(read(s), read(t))


def test_a_chain_without_host_transfers():
    gv(sps=8)
    h = np.random.default_rng(33).standard_normal(33)
    p, q = PRBS(15), PRBS(15, seed=0x1234)
    hp, hq = p._raw().to_host(), q._raw().to_host()
    before = _lib.TRANSFERS["d2h"]
    y = (~p + q * 3)[7:].dac(h)
    assert y.on_device and p.on_device and q.on_device and _lib.TRANSFERS["d2h"] == before
    bits = np.concatenate((1 - hp, np.tile(hq, 3)))[7:]
    xu = np.zeros(bits.size * 8)
    xu[4::8] = bits
    want = sg.fftconvolve(xu, h, mode="same")
    got = y.signal
    gv.default()
    assert got.shape == want.shape and got.dtype == want.dtype
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"chain: {bits.size} bits, max|d|/peak = {err:.3e}")
    assert err <= 1e-12
