"""A vectorised NumPy restatement of the device generator of csrc/device_mem.hip (`k_randn`): Philox4x32-10 (Salmon et al., SC'11) in uint64
arithmetic, the two 53-bit uniforms of a pair built in float64 exactly as the kernel builds them (that construction is part of the generator's
definition), and the Box-Muller pair evaluated in np.longdouble.  Test infrastructure; only tests/ imports it.

    counter = (pair lo, pair hi, stream lo, stream hi),  key = (seed lo, seed hi)
    u1 = ((c0 >> 5) * 2^26 + (c1 >> 6) + 0.5) * 2^-53,  u2 likewise from (c2, c3)              -- in (0, 1]: see `uniforms`
    element 2p = mean + std * sqrt(-2 ln u1) * cos(2 pi u2),  element 2p + 1 = ... * sin(2 pi u2)
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))


def philox4x32_10(counters, key):
    """counters: four uint64 arrays (or integers) holding 32-bit words; key: two integers.  Returns the four output words (uint64 arrays)."""
    c = [np.atleast_1d(np.asarray(w, np.uint64)) & M32 for w in counters]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]                              # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def uniform53(hi, lo):
    """The kernel's uniform from two output words: 27 bits of `hi` above 26 bits of `lo`, + 0.5, * 2^-53, every operation in float64.  The
    integer is below 2^53 and converts exactly; + 0.5 is exact below 2^52 and rounds to even above, so the largest integer 2^53 - 1 gives
    2^53 and u = 1.0: the interval is (0, 1], and u = 1 only makes r = 0."""
    k = ((np.asarray(hi, np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(lo, np.uint64) >> np.uint64(6))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def uniforms(pairs, seed, stream):
    """(u1, u2) in float64 for the pair indices `pairs` (any integers below 2^64) of (seed, stream)."""
    p = np.atleast_1d(np.asarray(pairs, np.uint64))
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    full = lambda v: np.full(p.shape, v, np.uint64)
    c = philox4x32_10((p & M32, p >> _S32, full(stream & 0xFFFFFFFF), full(stream >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return uniform53(c[0], c[1]), uniform53(c[2], c[3])


def randn(count, std, seed, stream, mean=0.0):
    """The `count` values ssfm_device_randn writes for (seed, stream), in np.longdouble, and r = sqrt(-2 ln u1) per pair (float64): elements
    2p and 2p + 1 come from pair p, an odd count cuts the last pair."""
    count = int(count)
    npairs = (count + 1) // 2
    u1, u2 = uniforms(np.arange(npairs, dtype=np.uint64), seed, stream)
    r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    ang = (LD(2) * PI_LD) * u2.astype(LD)
    out = np.empty(2 * npairs, LD)
    out[0::2] = LD(mean) + LD(std) * r * np.cos(ang)
    out[1::2] = LD(mean) + LD(std) * r * np.sin(ang)
    return out[:count], r.astype(np.float64)
