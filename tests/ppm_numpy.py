"""A NumPy restatement of the PPM receiver of opticomlib_amd.ppm (reference opticomlib/ppm.py), without the reference: the encoder, the
decoder, the slot decisions and HDD's draw scheme -- the ON count of every symbol, then np.random.randint(M) for each empty symbol in
ascending order, then np.random.randint(count) (the index among the ON slots, as np.random.choice takes it) for each multi-ON symbol in
ascending order, from NumPy's global generator."""
import numpy as np


def encode(bits, M):
    k = int(np.log2(M))
    b = np.asarray(bits, dtype=bool)
    b = b[: b.size // k * k].reshape(-1, k).astype(np.int64)
    v = b @ (1 << np.arange(k)[::-1])
    out = np.zeros(v.size * M, np.uint8)
    out[np.arange(v.size) * M + v] = 1
    return out


def decode(slots, M):
    k = int(np.log2(M))
    p = np.nonzero(np.asarray(slots) != 0)[0] % M
    return ((p[:, None] >> np.arange(k)[::-1]) & 1).astype(np.uint8).ravel()


def hdd(slots, M):
    """HDD on a 0 / 1 slot sequence: the one-hot symbols (a new array; the input is not written)."""
    s = (np.asarray(slots) != 0).reshape(-1, M).astype(np.uint8)
    cnt = s.sum(axis=1)
    out = s.copy()
    empty, multi = np.nonzero(cnt == 0)[0], np.nonzero(cnt > 1)[0]
    out[empty, np.random.randint(M, size=empty.size)] = 1
    if multi.size:
        r = np.random.randint(0, cnt[multi])
        ons = [np.nonzero(s[i])[0] for i in multi]
        out[multi] = 0
        out[multi, [o[j] for o, j in zip(ons, r)]] = 1
    return out.ravel()


def slot_samples(x, sps):
    return np.asarray(x, dtype=np.float64)[sps // 2:: sps]


def sdd(x, M, sps):
    y = slot_samples(x, sps).reshape(-1, M)
    out = np.zeros(y.shape, np.uint8)
    out[np.arange(y.shape[0]), np.argmax(y, axis=1)] = 1
    return out.ravel()


def dsp_hard(x, M, sps, rth):
    """The hard decision on the summed signal x with threshold rth: x[sps//2 :: sps] > rth, HDD, decoder."""
    return decode(hdd(slot_samples(x, sps) > rth, M), M)
