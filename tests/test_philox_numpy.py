"""The NumPy restatement of the device generator (tests/philox_numpy.py) against what is published and against the suite's scalar restatement:
the yardstick of tests/test_generators_gpu.py has to be right before a kernel is held to it."""
import numpy as np

import philox_numpy as ph


def words(c):
    return [int(w[0]) for w in c]


def test_random123_known_answers():
    # Random123's published known-answer vectors for philox4x32_10 (kat_vectors)
    assert words(ph.philox4x32_10((0, 0, 0, 0), (0, 0))) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert words(ph.philox4x32_10((f, f, f, f), (f, f))) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert words(ph.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_agrees_with_the_scalar_restatement():
    from test_gpu_parity import _philox4x32_10
    rng = np.random.default_rng(1)
    n = 300
    ctr = rng.integers(0, 2 ** 32, (4, n), dtype=np.uint64)
    ctr[:, :40] |= np.uint64(0x80000000)                             # high bits set: the products need all 64 bits
    ctr[:, 40:44] = np.uint64(0xFFFFFFFF)
    for key in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x89ABCDEF, 0x01234567), (0xFFFFFFFE, 0x80000000)):
        got = ph.philox4x32_10(tuple(ctr), key)
        for j in range(n):
            assert [int(w[j]) for w in got] == _philox4x32_10(tuple(int(v) for v in ctr[:, j]), key), (key, j)
    # the counter / key layout of `uniforms`: (pair lo, pair hi, stream lo, stream hi), (seed lo, seed hi)
    seed, stream = 0xFEDCBA9876543210, 2 ** 63 + 7
    pairs = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], np.uint64)
    u1, u2 = ph.uniforms(pairs, seed, stream)
    for j, p in enumerate(int(v) for v in pairs):
        c = _philox4x32_10((p & 0xFFFFFFFF, p >> 32, stream & 0xFFFFFFFF, stream >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert u1[j] == (((c[0] >> 5) << 26 | (c[1] >> 6)) + 0.5) * 2.0 ** -53
        assert u2[j] == (((c[2] >> 5) << 26 | (c[3] >> 6)) + 0.5) * 2.0 ** -53


def test_the_uniforms_lie_in_0_1_with_1_included():
    f = 0xFFFFFFFF
    assert ph.uniform53(f, f) == 1.0                                 # 2^53 - 1 + 0.5 is a tie and rounds to the even 2^53
    assert ph.uniform53(f, f - 64) == 1.0 - 2.0 ** -52               # 2^53 - 2 + 0.5 rounds to the even 2^53 - 2
    assert ph.uniform53(0, 0) == 2.0 ** -54                          # the smallest: never 0, so ln u1 is finite
    assert ph.uniform53(0, 64) == 1.5 * 2.0 ** -53
    x, r = ph.randn(5, 2.0, 3, 4, mean=1.0)
    assert x.dtype == np.longdouble and x.shape == (5,) and r.dtype == np.float64 and r.shape == (3,)
    a, _ = ph.randn(4, 2.0, 3, 4, mean=1.0)
    np.testing.assert_array_equal(x[:4], a)                          # an odd count cuts the last pair, nothing else
    u1, u2 = ph.uniforms(np.arange(3), 3, 4)
    want = 1.0 + 2.0 * np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    assert np.max(np.abs(x[0::2].astype(np.float64) - want)) < 1e-14
