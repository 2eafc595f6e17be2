"""``eye.plot`` on the MI355X (the fold entry points of csrc/eye_density.hip, opticomlib_amd.utils.eye_fold_density, eye.plot) against the NumPy /
SciPy restatement of the reference's lines (tests/eye_plot_numpy.py): counts, edges, grid indices and the masked histogram equal, the blurred grid
within (4 r + 4) 2^-53 max(grid), r = 12, of scipy.ndimage.gaussian_filter, the colours within three such bounds over the colour range, the smooth
side panel within ten.  Every measured deviation goes through tests/margins.py (profiles/eye_plot_margins.txt is such a file)."""
import hashlib
import os

import numpy as np
import pytest

import eye_plot_cases as pc
import eye_plot_numpy as pn
import eyediagram_cases as ec
import margins
from opticomlib_amd import _lib, utils
from opticomlib_amd.typing import EyeShowOptions, eye, gv

pytestmark = pytest.mark.gpu

# (sps, sps_resamp, samples): 2 sps < 8 leaves whole column groups empty; 2 sps >= 350 lets phases share columns; 1000 and 77 are no whole number
# of periods; 35200 samples at sps 16 are 1100 traces, more than one workgroup's 1024; (8, 32) is the resampled eye, L = 16 and P = 64
SHAPES = ((2, None, 4), (2, None, 200), (3, None, 18), (3, None, 606), (16, None, 1024), (16, None, 1000), (16, None, 35200), (256, None, 2048),
          (256, None, 4096 + 77), (8, 32, 512), (8, 32, 64 * 40 + 13))
WINDOW = (-0.05, 0.05)


def up(a):
    return _lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.float64))


def signal(sps, s, n, seed=0):
    s = s or sps
    rng = np.random.default_rng(seed + 7 * sps + n)
    return np.repeat(rng.integers(0, 2, -(-n // s)).astype(np.float64), s)[:n] + 0.1 * rng.standard_normal(n)


def make_eye(y, sps, s=None, **scalars):
    kw = dict(pc.SCALARS, sps=sps, dt=1e-9 / sps, y=y, i=sps // 2, execution_time=0.0, _nslots=int(y.size) // (s or sps))
    if s:
        kw["sps_resamp"] = s
    kw.update(scalars)
    return eye(**kw)


def check(d, r, what, colors=True, window=None):
    """Hold a device result to the restatement's; returns the blur bound."""
    assert d.n_traces == r["n_traces"] and d.extent == r["extent"], what
    assert d.counts.dtype == np.uint32 and d.counts.shape == (350, 350) and np.array_equal(d.counts, r["counts"]), what
    assert int(d.counts.sum(dtype=np.int64)) == len(r["y"]), what
    assert d.xedges.tobytes() == r["xedges"].tobytes() and d.yedges.tobytes() == r["yedges"].tobytes(), what
    bound = pn.blur_bound(r["grid"])
    dev = float(np.abs(d.grid - r["grid"]).max())
    margins.record(f"{what} grid", None, dev, bound)
    assert d.grid.dtype == np.float64 and dev <= bound, (what, dev, bound)
    pdev = float(np.abs(d.grid[170:180].sum(axis=0) - r["profile"]).max())
    margins.record(f"{what} side panel", None, pdev, 10 * bound)
    assert pdev <= 10 * bound, (what, pdev)
    if colors:
        k = r["k"]
        assert np.array_equal(d.x, r["t"][:k]) and np.array_equal(d.y, r["y"][:k]), what
        assert np.array_equal(d.ix, r["it"][:k]) and np.array_equal(d.iy, r["iy"][:k]), what
        assert d.colors.shape == (k,) and np.array_equal(np.isnan(d.colors), np.isnan(r["colors"][:k])), what
        if k and r["span"] > 0:
            cb = 3 * bound / r["span"]
            cdev = float(np.abs(d.colors - r["colors"][:k]).max())
            margins.record(f"{what} colours", None, cdev, cb)
            assert cdev <= cb, (what, cdev, cb)
    if window is not None:
        assert d.hist_counts.dtype == np.uint32 and np.array_equal(d.hist_counts, r["hist_counts"]), what
        assert d.hist_edges.tobytes() == r["hist_edges"].tobytes() and d.n_masked == r["n_masked"], what
    return bound


# ------------------------------------------------------------------------------------------------ counts, edges, grid, colours, histogram
@pytest.mark.parametrize("sps,s,n", SHAPES)
def test_counts_edges_indices_and_histogram_are_numpys(sps, s, n):
    y = signal(sps, s, n)
    d = utils.eye_fold_density(make_eye(up(y), sps, s), colors=True, hist=WINDOW)
    r = pn.reference(y, sps, s, WINDOW)
    check(d, r, f"sps={sps} s={s} n={n}", window=WINDOW)
    if (sps, n) == (16, 1000):
        assert len(r["y"]) % 32 == 24 and r["n_traces"] == 30                  # the count ends mid-trace
    if (sps, n) == (2, 4):
        assert r["n_traces"] == 0 and d.colors.size == 0 and r["n_masked"] == 0 and not d.hist_counts.any()
    if sps == 256:
        assert np.bincount((np.arange(512) * 350) // 512).max() >= 2             # phases share columns


@pytest.mark.parametrize("sps,s", ((16, None), (8, 32)))
def test_windows_that_take_one_phase_many_or_none(sps, s):
    y = signal(sps, s, 64 * (s or sps), seed=3)
    dy = up(y)
    for window in ((-0.05, 0.05), (-0.5, 0.5), (-2.0, 2.0), (1 / 64 + 1e-9, 1 / 64 + 2e-9), (0.0, 0.0)):
        d = utils.eye_fold_density(make_eye(dy, sps, s), hist=window)
        r = pn.reference(y, sps, s, window)
        check(d, r, f"sps={sps} s={s} window={window}", colors=False, window=window)
        if window[1] - window[0] < 1e-6:
            assert d.n_masked == 0 and d.hist_edges.tobytes() == np.linspace(0, 1, 201).tobytes()


def test_a_record_made_of_the_edge_values():
    sps, n = 3, 3 * 400
    a, b = -0.3, 1.7
    edges = np.linspace(a, b, 351)
    rng = np.random.default_rng(5)
    pool = np.concatenate([edges, np.nextafter(edges[1:], -np.inf), np.nextafter(edges[:-1], np.inf)])
    y = pool[rng.integers(0, pool.size, n)]
    y[sps], y[sps + 1] = a, b                                   # both ends are among the plotted points
    r = pn.reference(y, sps, None, (-0.4, 0.1))
    assert r["yedges"].tobytes() == edges.tobytes()
    d = utils.eye_fold_density(make_eye(up(y), sps), colors=True, hist=(-0.4, 0.1))
    check(d, r, "edge values", window=(-0.4, 0.1))
    # the histogram's own edges: a record whose masked values are its 201 edges and their neighbours
    hedges = np.linspace(a, b, 201)
    pool = np.concatenate([hedges, np.nextafter(hedges[1:], -np.inf), np.nextafter(hedges[:-1], np.inf)])
    y = pool[rng.integers(0, pool.size, n)]
    y[sps + 2], y[sps + 8] = a, b                               # phase 2 (t = -1/3) passes the window
    r = pn.reference(y, sps, None, (-0.4, 0.1))
    assert r["hist_edges"].tobytes() == hedges.tobytes()
    check(utils.eye_fold_density(make_eye(up(y), sps), hist=(-0.4, 0.1)), r, "histogram edge values", colors=False, window=(-0.4, 0.1))


def test_a_constant_record():
    y = np.full(16 * 8, 0.75)
    d = utils.eye_fold_density(make_eye(up(y), 16), colors=True, hist=WINDOW)
    r = pn.reference(y, 16, None, WINDOW)
    check(d, r, "constant", window=WINDOW)
    assert d.yedges[0] == 0.25 and d.yedges[-1] == 1.25 and not d.iy.any() and np.isnan(d.colors).all() and d.hist_edges[0] == 0.25


# ------------------------------------------------------------------------------------------------ non-finite values
def test_non_finite_values_among_the_plotted_points_and_outside_them(monkeypatch):
    sps, n = 16, 1024
    y = signal(sps, None, n, seed=9)
    clean = utils.eye_fold_density(make_eye(up(y), sps), hist=WINDOW)

    def never(*a):
        raise AssertionError("the density was launched after the range had failed")
    for pos, bad in ((sps, np.nan), (n // 2, np.nan), (n - 1, np.nan), (sps + 123, np.inf), (n - 4, -np.inf)):
        v = y.copy()
        v[pos] = bad
        t_, y_ = pn.fold(v, sps)
        with pytest.raises(ValueError) as numpys:
            np.histogram2d(t_, y_, bins=350)
        assert "is not finite" in str(numpys.value)
        with monkeypatch.context() as m:
            m.setattr(_lib.api, "ssfm_eye_fold_density", never, raising=False)
            with pytest.raises(ValueError) as ours:
                utils.eye_fold_density(make_eye(up(v), sps), colors=True, hist=WINDOW)
        assert str(ours.value) == str(numpys.value)
    for pos in (0, sps // 2, sps - 1):                           # y[:sps] is outside the fold
        v = y.copy()
        v[pos] = np.nan
        d = utils.eye_fold_density(make_eye(up(v), sps), hist=WINDOW)
        assert d.counts.tobytes() == clean.counts.tobytes() and d.grid.tobytes() == clean.grid.tobytes() and d.hist_counts.tobytes() == clean.hist_counts.tobytes()


def test_two_calls_give_the_same_bits():
    y = signal(16, None, 35200, seed=2)
    e = make_eye(up(y), 16)
    a = utils.eye_fold_density(e, colors=True, hist=WINDOW)
    b = utils.eye_fold_density(e, colors=True, hist=WINDOW)
    for k in ("counts", "grid", "colors", "y", "iy", "hist_counts", "hist_edges"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ------------------------------------------------------------------------------------------------ the old entry points
# sha256 of the float64 grid and of the colours that utils.eye_density returned for these cases of tests/eyediagram_cases.py on an MI355X with
# the library of the commit before the kernels took the general fold.  The records come from NumPy's default_rng and the edges from np.linspace, so a
# NumPy whose generator or linspace gives other bits changes these hashes with no change in the kernels: regenerate them then by building that commit's
# library (the parent of the one that added this file), pointing SSFM_LIB at it and hashing what this test hashes.
OLD_GRID_SHA256 = {"sps16_t300_density": ("2f9240a0183329a867968bde8851bae9b44b2231cc1596768cd3fb139d6ad399",
                                          "2fd7cc3e003ad87fc2eac81e7e3476f10fceb2aff3dfff848860f387ef767f25"),
                   "sps16_noise_line_cap": ("6c4d5562e8957496271057bfb3ccc5c416d72ad10cb81f94ed35669293f4b02d",
                                            "84b9a6ff53aad52a36703eaacd85c4ae3abba1199c67e731640a25d1b6397ebf"),
                   "sps3_t300_dot": ("6fa90a56735567ca790c1823aa29765f66d4f980595a8845fb8b866193217939",
                                     "dba23a5df083030fc890496954ea6b4eca8853485265083ef02c30f53df9c538")}


@pytest.mark.parametrize("name", sorted(OLD_GRID_SHA256))
def test_the_old_entry_points_give_the_bits_they_gave(golden_dir, name):
    c = ec.CASES[name]
    y, z = ec.record(name)
    kw = c["kw"]
    B, sigma, nt = kw.get("N_grid_bins", 200), kw.get("grid_sigma", 5), min(kw.get("n_traces", 4096), 4096)
    d = utils.eye_density(up(y if z is None else y + z), c["sps"], nt, B, sigma, colors=True)
    assert (hashlib.sha256(d.grid.tobytes()).hexdigest(), hashlib.sha256(d.colors.tobytes()).hexdigest()) == OLD_GRID_SHA256[name]
    want = np.load(os.path.join(golden_dir, f"eyediagram_{name}.npz"))
    if "image" in want.files:                                   # the reference's picture: SciPy's bits, within the blur bound
        image = want["image"]
        assert np.abs(d.grid.T - image).max() <= (4 * int(4.0 * sigma + 0.5) + 4) * 2.0 ** -53 * image.max()
    elif "offsets" in want.files:                               # the scatter's points
        assert np.array_equal(want["offsets"], np.column_stack([d.x, d.y]))
    else:                                                       # the last trace's segments
        assert np.array_equal(want["last_segments"][:, 0, 1], d.y[-2 * c["sps"]:-1])


# ------------------------------------------------------------------------------------------------ residency
@pytest.fixture
def agg():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.close("all")
    yield plt
    plt.close("all")
    gv.default()


# device-to-host array copies of one plot: counts and grid; with smooth=False the drawn points' values, indices and colours; the step histogram's counts
D2H = {(True, False): 2, (True, True): 2, (False, False): 5, (False, True): 6}


@pytest.mark.parametrize("smooth,histogram", sorted(D2H))
def test_plot_leaves_the_record_on_the_device(agg, smooth, histogram):
    y = pc.record("sps16_lines_hist")
    e = make_eye(up(y), 16)
    t0 = dict(_lib.TRANSFERS)
    assert e.plot(EyeShowOptions(histogram=histogram), smooth=smooth) is e
    t1 = dict(_lib.TRANSFERS)
    assert t1["h2d"] == t0["h2d"] and t1["d2h"] - t0["d2h"] == D2H[smooth, histogram]
    assert isinstance(e.__dict__["_y"], _lib.DeviceArray)
    assert np.array_equal(e.y, y) and isinstance(e.__dict__["_y"], np.ndarray)      # read once: a host record from here on
    t2 = dict(_lib.TRANSFERS)
    e.plot(EyeShowOptions(histogram=histogram), smooth=smooth)
    assert _lib.TRANSFERS == t2


# ------------------------------------------------------------------------------------------------ artists
@pytest.mark.parametrize("name", [k for k, c in sorted(pc.CASES.items()) if not c.get("empty")])
def test_a_device_eye_draws_what_the_host_path_draws(agg, name):
    c = pc.CASES[name]
    host = pc.run(name, eye, EyeShowOptions)
    h2d = _lib.TRANSFERS["h2d"]
    dy = up(pc.record(name))
    dev = pc.run(name, eye, EyeShowOptions, y=dy)
    assert _lib.TRANSFERS["h2d"] == h2d + 1                     # the upload above and nothing else
    assert str(dev["kind"]) == str(host["kind"])
    if str(host["kind"]) == "error":
        assert str(dev["error_type"]) == str(host["error_type"]) and str(dev["error_text"]) == str(host["error_text"])
        return
    r = pn.reference(pc.record(name), c["sps"], c.get("resamp"))
    pn.compare(dev, host, pn.blur_bound(r["grid"]), float(r["counts"].max() - r["counts"].min()),
               smooth_hist=c["kw"].get("smooth", True) and bool(c["opts"].get("histogram") or c["opts"].get("all_none")), cmap=c["kw"].get("cmap", "winter"))


def test_eyes_of_get_eye_and_get_eye_v2_plot_from_the_device(agg):
    from opticomlib_amd import DAC, GET_EYE, LPF, PRBS, lab
    gv(sps=16, R=10e9)
    bits = PRBS(order=9, len=512)
    x = LPF(DAC(bits, Vpp=1.0, pulse_shape="gaussian"), BW=7e9)
    assert x.on_device
    for origin, e, s in (("GET_EYE", GET_EYE(x, nslots=256), None), ("GET_EYE sps_resamp=64", GET_EYE(x, nslots=256, sps_resamp=64), 64),
                         ("lab.GET_EYE_v2", lab.GET_EYE_v2(x, bits, nslots=256), None)):
        assert isinstance(e.__dict__["_y"], _lib.DeviceArray)
        t0 = dict(_lib.TRANSFERS)
        window = (e.t_opt - 0.05 * e.t_dist, e.t_opt + 0.05 * e.t_dist)
        d = utils.eye_fold_density(e, colors=True, hist=window)
        for smooth in (True, False):
            agg.close("all")
            assert e.plot(EyeShowOptions(all_none=True), smooth=smooth) is e
            assert len(agg.gcf().axes) == 2
        t1 = dict(_lib.TRANSFERS)
        assert t1["h2d"] == t0["h2d"] and t1["d2h"] - t0["d2h"] == 6 + 2 + 6 and isinstance(e.__dict__["_y"], _lib.DeviceArray)
        lc = agg.gcf().axes[0].collections
        assert len(lc) == d.n_traces == (256 * (s or 16) - 16) // 32
        y = e.y                                                 # the download, after everything was drawn
        check(d, pn.reference(y, 16, s, window), origin, window=window)
