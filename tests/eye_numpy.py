"""NumPy / SciPy restatement of the OOK receiver (reference devices.py:1635-1891, ook.py:22-220) with the deterministic two-means of
csrc/eye.hip in place of sklearn's KMeans: the checker of tests/test_eye_gpu.py (the GPU box has no reference and may have no sklearn).

The two-means, as on the device:
  * 1-D: centres (min, max); a sample belongs to centre 1 when |x - c1| < |x - c0|;
  * 2-D: the points of the 25-75 % band split at their mean t (t >= mean: cluster 1), then Lloyd on (t - ct)^2 + (y - cy)^2;
  * an iteration recomputes the centres from the assignment (an empty cluster keeps its centre) and stops when they no longer change,
    or after 300 updates (sklearn's max_iter).
With ``updates=True`` each two-means also returns how many times its centres changed; ``get_eye`` reports both counts as ``_updates1`` /
``_updates2`` (what the device's host loop of 24-step chunks depends on).  A signal that holds NaN or infinity raises ValueError, as
sklearn's input validation does in the reference's ``KMeans.fit``.
"""
from __future__ import annotations

import numpy as np
from scipy.signal import resample
from scipy.special import erfc

LLOYD_MAX = 300


def Q(x):
    return 0.5 * erfc(x / np.sqrt(2))


def t_grid(s: int) -> np.ndarray:
    return np.linspace(-1, 1 - 1 / s, 2 * s)


def find_nearest(levels: np.ndarray, v: float) -> float:
    """The value of the SORTED set ``levels`` closest to v, the lower one on ties (reference find_nearest)."""
    return float(levels[np.argmin(np.abs(levels - v))])


def shortest_int(x: np.ndarray, percent: float = 50) -> np.ndarray:
    x = np.sort(x)
    lag = int(len(x) * percent / 100)
    if lag < 1:
        raise ValueError(f"Computed lag ({lag}) must be at least 1.")
    diff = x[lag:] - x[:-lag]
    i = np.where(np.abs(diff - np.min(diff)) < 1e-10)[0]
    i = int(np.mean(i)) if len(i) > 1 else int(i[0])
    return np.array((x[i], x[i + lag]))


def two_means_1d(x: np.ndarray, updates: bool = False):
    c = np.array([x.min(), x.max()])
    u = 0
    for _ in range(LLOYD_MAX):
        one = np.abs(x - c[1]) < np.abs(x - c[0])
        new = c.copy()
        if (~one).any():
            new[0] = x[~one].mean()
        if one.any():
            new[1] = x[one].mean()
        if np.array_equal(new, c):
            break
        c = new
        u += 1
    return (c, u) if updates else c


def two_means_2d(t: np.ndarray, y: np.ndarray, updates: bool = False):
    """Centres (2, 2) as rows (t, y)."""
    def means(one, c):
        new = c.copy()
        if (~one).any():
            new[0] = t[~one].mean(), y[~one].mean()
        if one.any():
            new[1] = t[one].mean(), y[one].mean()
        return new
    one = ~(t < t.mean())
    c = means(one, np.full((2, 2), np.nan))
    if not (~one).any():
        c[0] = c[1]
    if not one.any():
        c[1] = c[0]
    u = 0
    for _ in range(LLOYD_MAX):
        one = (t - c[1, 0]) ** 2 + (y - c[1, 1]) ** 2 < (t - c[0, 0]) ** 2 + (y - c[0, 1]) ** 2
        new = means(one, c)
        if np.array_equal(new, c):
            break
        c = new
        u += 1
    return (c, u) if updates else c


def kde_argmin(y: np.ndarray, mu0: float, mu1: float, npts: int = 500):
    """x[argmin(gaussian_kde(y).evaluate(x))] over x = linspace(mu0, mu1, npts); None when the KDE is singular."""
    from scipy.stats import gaussian_kde
    x = np.linspace(mu0, mu1, npts)
    try:
        return float(x[np.argmin(gaussian_kde(y).evaluate(x))])
    except Exception:
        return None


def get_eye(x: np.ndarray, sps: int, nslots: int = 4096, sps_resamp=None) -> dict:
    """GET_EYE on the real signal ``x`` (signal + noise) with ``sps`` samples per slot: the reference's attributes as a dict."""
    x = np.asarray(x).real.astype(np.float64)
    d = {"sps": sps}
    r = x.size % (2 * sps)
    if r:
        x = x[:-r]
    nslots = min(int(x.size // sps), nslots)
    x = np.roll(x[: nslots * sps], -sps // 2 + 1)
    y_set = np.unique(x)
    s = sps_resamp if sps_resamp else sps
    if sps_resamp:
        x = resample(x, nslots * sps_resamp)
    tg = t_grid(s)
    t = np.kron(np.ones(nslots // 2), tg)
    d["y"], d["t"] = x, t
    if not np.isfinite(x).all():
        raise ValueError("Input X contains NaN or infinity.")
    c, d["_updates1"] = two_means_1d(x, updates=True)
    d["_updates2"] = 0
    vm = np.mean(c)
    d["top_int"] = top = shortest_int(x[x > vm])
    d["bot_int"] = bot = shortest_int(x[x < vm])
    s1, s0 = np.mean(top), np.mean(bot)
    d01 = s1 - s0
    v75, v25 = s1 - 0.25 * d01, s0 + 0.25 * d01
    band = (x > v25) & (x < v75)
    if band.sum() >= 2:
        cc, d["_updates2"] = two_means_2d(t[band], x[band], updates=True)
        left, right = np.argmin(cc[:, 0]), np.argmax(cc[:, 0])
        d["t_left"] = t_left = find_nearest(tg, cc[left, 0])
        d["t_right"] = t_right = find_nearest(tg, cc[right, 0])
        d["t_opt"] = t_c = find_nearest(tg, cc[:, 0].mean())
        d["y_left"] = find_nearest(y_set, cc[left, 1])
        d["y_right"] = find_nearest(y_set, cc[right, 1])
    else:
        d["t_left"], d["t_right"], d["t_opt"] = t_left, t_right, t_c = -0.5, 0.5, 0.0
        d["y_left"] = d["y_right"] = None
    d["t_dist"] = t_dist = t_right - t_left
    d["t_span0"] = t0 = t_c - 0.05 * t_dist
    d["t_span1"] = t1 = t_c + 0.05 * t_dist
    d["y_center"] = yc = find_nearest(y_set, (s0 + s1) / 2)
    if sps_resamp:
        i = np.abs(t - t_c).argmin() - sps_resamp // 2 + 1
        d["i"] = int(i / sps_resamp * sps)
    else:
        d["i"] = int(np.abs(t - t_c).argmin() - sps // 2 + 1)
    mid = (t0 < t) & (t < t1)
    top_m, bot_m = (x > yc) & mid, (x < yc) & mid
    with np.errstate(invalid="ignore", divide="ignore"):
        d["mu1"] = mu1 = float(np.mean(x, where=top_m))
        d["s1"] = float(np.std(x, where=top_m))
        d["mu0"] = mu0 = float(np.mean(x, where=bot_m))
        d["s0"] = float(np.std(x, where=bot_m))
        d["threshold"] = kde_argmin(x[mid], mu0, mu1)
        d["er"] = 10 * np.log10(mu1 / mu0) if mu0 > 0 else np.inf if mu0 == 0 else np.nan
    d["eye_h"] = mu1 - 3 * d["s1"] - mu0 - 3 * d["s0"]
    return d


def threshold_est(mu0, mu1, s0, s1) -> float:
    r = np.linspace(mu0, mu1, 1000)
    return float(r[np.argmin(0.5 * (Q((mu1 - r) / s1) + Q((r - mu0) / s0)))])


def dsp(x: np.ndarray, sps: int):
    """ook.DSP without a filter on the real signal x: (bits, eye dict, rth)."""
    e = get_eye(x, sps, nslots=8192, sps_resamp=128)
    rth = threshold_est(e["mu0"], e["mu1"], e["s0"], e["s1"])
    bits = (np.asarray(x).real[sps // 2::sps] > rth).astype(np.uint8)
    return bits, e, rth


def ber_estimator(e: dict) -> float:
    um = threshold_est(e["mu0"], e["mu1"], e["s0"], e["s1"])
    return float(0.5 * (Q((e["mu1"] - um) / e["s1"]) + Q((um - e["mu0"]) / e["s0"])))
