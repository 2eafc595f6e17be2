"""NumPy / SciPy float64 restatement of the data-aided receiver (reference lab.py:92-273): the checker of tests/test_sync_gpu.py (the GPU box
has no reference).  Written from the algebra:

  SYNC        l = len(slots) sps, W = min(len(rx), 2 l), nc = W - l + 1 lags; corr[k] = sum_m rx[k + m] tx[m], tx = kron(slots, ones(sps));
              BufferError when len(rx) < l; ValueError when max(corr) < 3 std(corr) (population std); i = the first index of the maximum; the
              cut is rx[i : len(rx) - (l - i)] read as Python reads rx[i:-(l - i)] (-(0) is 0: nothing).
  GET_EYE_v2  truncation to a multiple of 2 sps and to nslots slots; x = Re(signal + noise), y = roll(x, -sps // 2 + 1); ones / zeros = the
              samples of x whose slot was sent as 1 / as 0; the moments of those whose slot-grid time lies strictly inside (-0.05, 0.05); the
              threshold = argmin over linspace(mu0, mu1, 500) of gaussian_kde(zeros first, then ones).
"""
from __future__ import annotations

import numpy as np
import scipy.signal as sg
from scipy.stats import gaussian_kde


def template(slots, sps: int) -> np.ndarray:
    return np.kron(np.asarray(slots, dtype=np.float64), np.ones(sps))


def correlation(rx, slots, sps: int) -> np.ndarray:
    """corr[k], k < nc, by SciPy's FFT convolution (what the reference calls)."""
    rx = np.asarray(rx, dtype=np.float64)
    tx = template(slots, sps)
    l = tx.size
    if rx.size < l:
        raise BufferError('The length of the received vector must be greater than the transmitted vector!!')
    return sg.fftconvolve(rx[:2 * l], tx[::-1], mode="valid")


def correlation_direct(rx, slots, sps: int) -> np.ndarray:
    """The same sums term by term in np.longdouble: the yardstick of the two FFT correlations.  tx is 0 / 1, so a lag's sum is a difference of
    running sums over the slots' runs -- formed here as plain windowed sums, one slot at a time."""
    rx = np.asarray(rx, dtype=np.longdouble)
    slots = np.asarray(slots)
    l = slots.size * sps
    W = min(rx.size, 2 * l)
    nc = W - l + 1
    out = np.zeros(nc, dtype=np.longdouble)
    win = np.lib.stride_tricks.sliding_window_view(rx[:W], sps).sum(axis=1, dtype=np.longdouble)     # win[j] = sum rx[j : j + sps]
    for s in np.nonzero(slots)[0]:
        out += win[s * sps: s * sps + nc]
    return out


def peak_stats(corr) -> dict:
    corr = np.asarray(corr)
    return {"max": float(np.max(corr)), "argmax": int(np.argmax(corr)), "mean": float(np.mean(corr)), "std": float(np.std(corr))}


def margin(corr) -> float:
    """How far the largest lag stands above the runner-up, relative to it (0 for a tie)."""
    c = np.sort(np.asarray(corr, dtype=np.float64))
    return float((c[-1] - c[-2]) / abs(c[-1])) if c.size > 1 and c[-1] != 0 else np.inf


def sync(rx, slots, sps: int) -> dict:
    """corr, its peak statistics, i and the cut record (an empty array where the reference's constructor would refuse the empty slice)."""
    rx = np.asarray(rx, dtype=np.float64)
    corr = correlation(rx, slots, sps)
    d = {"corr": corr, **peak_stats(corr)}
    if d["max"] < 3 * d["std"]:
        raise ValueError('No correlation maximum found!!')
    l = np.asarray(slots).size * sps
    i = d["argmax"]
    d["i"] = i
    d["signal"] = rx[i:-(l - i)]
    return d


def get_eye_v2(x, slots, sps: int, nslots: int = 4096) -> dict:
    """Every key of the reference's eye for the real signal ``x`` (signal + noise)."""
    x = np.asarray(x).real.astype(np.float64)
    slots = np.asarray(slots)
    d = {"sps": sps}
    r = x.size % (2 * sps)
    if r:
        x = x[:-r]
    nslots = min(int(x.size // sps), nslots)
    x = x[: nslots * sps]
    d["nslots"] = nslots
    d["y"] = np.roll(x, -sps // 2 + 1)
    d["t"] = np.kron(np.ones(nslots // 2), np.linspace(-1, 1 - 1 / sps, 2 * sps))
    ref = np.kron(slots[:nslots], np.ones(sps))
    d["ones"] = ones = x[ref == 1]                              # IndexError when the slots are too few
    d["zeros"] = zeros = x[ref == 0]
    grid = np.linspace(-0.5, 0.5, sps, endpoint=False)
    d["t0"] = t0 = np.kron(np.ones(zeros.size // sps), grid)
    d["t1"] = t1 = np.kron(np.ones(ones.size // sps), grid)
    d.update(i=sps // 2, t_left=-0.5, t_right=0.5, y_left=None, y_right=None, t_dist=1, t_opt=0)
    d["t_span0"] = s0_ = 0 - 0.05 * 1
    d["t_span1"] = s1_ = 0 + 0.05 * 1
    ones_ = ones[(t1 > s0_) & (t1 < s1_)]
    zeros_ = zeros[(t0 > s0_) & (t0 < s1_)]
    with np.errstate(invalid="ignore", divide="ignore"):
        d["mu0"] = mu0 = float(np.mean(zeros_))
        d["mu1"] = mu1 = float(np.mean(ones_))
        d["s0"] = float(np.std(zeros_))
        d["s1"] = float(np.std(ones_))
        grid500 = np.linspace(mu0, mu1, 500)
        pdf = gaussian_kde(zeros_.tolist() + ones_.tolist()).evaluate(grid500)      # LinAlgError when the samples are all equal
        d["threshold"] = float(grid500[np.argmin(pdf)])
        d["er"] = 10 * np.log10(mu1 / mu0) if mu0 > 0 else np.inf if mu0 == 0 else np.nan
    d["eye_h"] = mu1 - 3 * d["s1"] - mu0 - 3 * d["s0"]
    return d
