"""The eye diagram's density on the MI355X (csrc/eye_density.hip, opticomlib_amd.utils.eye_density / eyediagram, electrical_signal.plot_eye) against
NumPy and SciPy on this machine (tests/eye_density_numpy.py): counts equal to np.histogram2d's integers and edges to its bits, the blur within
(4 r + 4) 2^-53 max(grid) of scipy.ndimage.gaussian_filter, the plotted points' grid indices exact and their colours within three blur bounds over
the colour range.  With EYE_DENSITY_MARGINS=<path> the measured margins are written there (profiles/eye_density_margins.txt is such a file)."""
import os
import warnings

import numpy as np
import pytest

import eye_density_numpy as en
from opticomlib_amd import _lib, utils
from opticomlib_amd.typing import electrical_signal, gv

pytestmark = pytest.mark.gpu

SPS = (2, 3, 16, 64)
BINS = (1, 2, 7, 8, 200, 350)
MARGINS = {"blur": (0.0, None), "colour": (0.0, None), "scipy_vs_restatement": (0.0, None)}


def chunk_traces(sps):
    return max(1, utils.EYE_CHUNK_POINTS // (2 * sps))


def trace_counts(sps):
    """1, 2, 257, the first count that needs a second workgroup of the counting kernel, and one more."""
    c = chunk_traces(sps)
    return sorted({1, 2, 257, c + 1, c + 2})


def record(sps, T, tail, seed=0, noise=False):
    """An OOK-like record of exactly T whole traces after the cut, plus `tail` (< 2 sps) samples."""
    rng = np.random.default_rng(seed + 1000 * sps + T)
    n = 2 * (sps // 2) + T * 2 * sps + tail
    y = rng.integers(0, 2, n).astype(np.float64) + 0.1 * rng.standard_normal(n)
    z = 0.05 * rng.standard_normal(n) if noise else None
    return y, z


def up(a):
    return None if a is None else _lib.DeviceArray.from_host(a)


def device_density(y, z, sps, n_traces, B, sigma, colors=False):
    s = up(y)
    arg = s if z is None else electrical_signal.from_device(s, up(z))
    return utils.eye_density(arg, sps, n_traces, B, sigma, colors=colors)


def margin(name, dev, bound):
    m = dev / bound if bound > 0 else (0.0 if dev == 0 else np.inf)
    if m >= MARGINS[name][0]:
        MARGINS[name] = (m, bound)
    return m


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("noise", (False, True))
@pytest.mark.parametrize("sps", SPS)
def test_counts_are_numpys_integers_and_edges_its_bits(sps, noise):
    P = 2 * sps
    for T in trace_counts(sps):
        y, z = record(sps, T, tail=P - 1, noise=noise)         # a tail of P - 1 samples after the last whole trace
        s, nz = up(y), up(z)
        arg = s if nz is None else electrical_signal.from_device(s, nz)
        X, Y, Tr = en.points(y if z is None else y + z, sps)
        assert Tr == T
        for B in BINS:
            want, xe, ye = en.histogram(X, Y, B)
            d = utils.eye_density(arg, sps, None, B, 0)
            assert d.n_traces == T and d.counts.dtype == np.uint32 and d.counts.shape == (B, B)
            assert np.array_equal(d.counts, want), (sps, T, B, noise, int(np.abs(d.counts - want).max()))
            assert int(d.counts.sum(dtype=np.int64)) == T * P
            assert d.xedges.tobytes() == xe.tobytes() and d.yedges.tobytes() == ye.tobytes(), (sps, T, B)
            assert np.array_equal(d.grid, want)                # sigma = 0 is the identity
            assert d.extent == (X.min(), X.max(), Y.min(), Y.max())


def test_the_shape_that_fits_no_lds_tile():
    """sps = 64 with B = 350: 350 x 350 counters are 490 kB, the columns are taken in groups; with noise, and across a workgroup boundary."""
    sps, B = 64, 350
    for T in (chunk_traces(sps) + 1, 3):
        y, z = record(sps, T, tail=5, noise=True, seed=7)
        d = device_density(y, z, sps, None, B, 3)
        r = en.reference(y + z, sps, None, B, 3)
        assert np.array_equal(d.counts, r["counts"])
        bound = en.blur_bound(3, r["grid"])
        assert margin("blur", float(np.abs(d.grid - r["grid"]).max()), bound) <= 1.0


@pytest.mark.parametrize("sps", (3, 16))
def test_n_traces_below_at_and_above_the_available_number(sps):
    y, _ = record(sps, 9, tail=0, seed=3)                      # no tail at all
    s = up(y)
    for nt in (1, 8, 9, 10, 5000, None):
        X, Y, T = en.points(y, sps, nt)
        assert T == (9 if nt is None else min(9, nt))
        for B in (7, 200):
            want, xe, ye = en.histogram(X, Y, B)
            d = utils.eye_density(s, sps, nt, B, 0)
            assert d.n_traces == T and np.array_equal(d.counts, want) and d.yedges.tobytes() == ye.tobytes()


# ------------------------------------------------------------------------------------------------ hard values
@pytest.mark.parametrize("B", (2, 7, 8, 200, 350))
def test_a_record_made_of_the_edge_values(B):
    sps, T = 3, 120
    a, b = -0.3, 1.7
    edges = np.linspace(a, b, B + 1)
    rng = np.random.default_rng(B)
    n = 2 * (sps // 2) + T * 2 * sps
    y = edges[rng.integers(0, B + 1, n)]
    y[1], y[2] = a, b                                          # both ends are present among the plotted points
    X, Y, _ = en.points(y, sps)
    want, _, ye = en.histogram(X, Y, B)
    assert ye.tobytes() == edges.tobytes()
    d = utils.eye_density(up(y), sps, None, B, 0)
    assert np.array_equal(d.counts, want) and d.yedges.tobytes() == edges.tobytes()
    # every interior edge value lands in the bin to its right, b in the last one
    per_bin = d.counts.sum(axis=0, dtype=np.int64)
    k = np.searchsorted(edges, Y, side="left")                 # Y is edges[k] exactly
    assert np.array_equal(edges[k], Y)
    assert np.array_equal(per_bin, np.bincount(np.minimum(k, B - 1), minlength=B))


def test_a_constant_record():
    sps, T, c = 16, 40, 0.75
    y = np.full(sps + T * 2 * sps + 3, c)
    d = utils.eye_density(up(y), sps, None, 200, 5, colors=True)
    r = en.reference(y, sps, None, 200, 5)
    assert d.yedges[0] == c - 0.5 and d.yedges[-1] == c + 0.5 and d.yedges.tobytes() == r["yedges"].tobytes()
    assert np.array_equal(d.counts, r["counts"]) and np.count_nonzero(d.counts.sum(axis=0)) == 1      # one column of y
    assert np.array_equal(d.iy, r["iy"]) and not d.iy.any()
    assert d.colors.shape == (T * 2 * sps,) and not d.colors.any() and not r["colors"].any()


@pytest.mark.parametrize("B", (1, 200))
def test_two_to_the_twenty_equal_samples(B):
    sps = 16
    n = (1 << 20) + 4 * sps + sps                              # T P = 2^20 + 64 plotted points
    y = np.full(n, -2.5)
    d = utils.eye_density(up(y), sps, None, B, 0)
    X, Y, T = en.points(y, sps)
    want, _, _ = en.histogram(X, Y, B)
    assert np.array_equal(d.counts, want)
    if B == 1:
        assert int(d.counts[0, 0]) == T * 2 * sps > 1 << 20


@pytest.mark.parametrize("B", (1, 2, 200))
def test_a_range_that_overflows(B):
    """+-1.7e308 together: max - min is infinite.  Whatever NumPy does -- an error or a result -- the device path does."""
    sps, T = 2, 6
    y = np.tile([1.7e308, -1.7e308, 0.5], 20)[:sps + T * 2 * sps]
    X, Y, _ = en.points(y, sps)
    try:
        want, _, ye = en.histogram(X, Y, B)
        err = None
    except ValueError as e:
        err = str(e)
    if err is None:
        d = utils.eye_density(up(y), sps, None, B, 0)
        assert np.array_equal(d.counts, want) and d.yedges.tobytes() == ye.tobytes()
    else:
        with pytest.raises(ValueError) as ei:
            utils.eye_density(up(y), sps, None, B, 0)
        assert str(ei.value) == err


# ------------------------------------------------------------------------------------------------ non-finite values
def test_non_finite_values_among_the_plotted_points_and_outside_them():
    sps, T, B = 16, 300, 50
    P = 2 * sps
    y, _ = record(sps, T, tail=7, seed=5)
    first, last = sps // 2, sps // 2 + T * P - 1
    clean = utils.eye_density(up(y), sps, None, B, 2)
    for pos, bad in ((first, np.nan), ((first + last) // 2, np.nan), (last, np.nan), (first + 1234, np.inf), (last - 3, -np.inf)):
        v = y.copy()
        v[pos] = bad
        X, Y, _ = en.points(v, sps)
        with pytest.raises(ValueError) as numpys:
            en.histogram(X, Y, B)
        assert "is not finite" in str(numpys.value)
        with pytest.raises(ValueError) as ours:
            utils.eye_density(up(v), sps, None, B, 2)
        assert str(ours.value) == str(numpys.value)
    for pos in (0, first - 1, last + 1, y.size - 1):          # the truncated head, and beyond the last whole trace
        v = y.copy()
        v[pos] = np.nan
        d = utils.eye_density(up(v), sps, None, B, 2)
        assert np.array_equal(d.counts, clean.counts) and d.grid.tobytes() == clean.grid.tobytes() and d.yedges.tobytes() == clean.yedges.tobytes()
    # a NaN in the noise alone is a NaN of the plotted sum
    z = np.zeros_like(y)
    z[first + 5] = np.nan
    with pytest.raises(ValueError, match="is not finite"):
        utils.eye_density(electrical_signal.from_device(up(y), up(z)), sps, None, B, 2)


# ------------------------------------------------------------------------------------------------ blur and colours
@pytest.fixture(scope="module")
def blur_record():
    return record(16, 257, tail=9, seed=11)[0]


@pytest.mark.parametrize("B", (7, 8, 200, 350))
@pytest.mark.parametrize("sigma", (0, 0.5, 3, 5))
def test_blur_and_colours_within_their_bounds(blur_record, sigma, B):
    sps = 16
    d = utils.eye_density(up(blur_record), sps, None, B, sigma, colors=True)
    r = en.reference(blur_record, sps, None, B, sigma)
    assert np.array_equal(d.counts, r["counts"])
    bound = en.blur_bound(sigma, r["grid"])
    dev = float(np.abs(d.grid - r["grid"]).max())
    print(f"blur B={B} sigma={sigma} r={en.radius(sigma)}: max deviation {dev:.3e}, bound {bound:.3e}")
    m = margin("blur", dev, bound)
    margin("scipy_vs_restatement", float(np.abs(en.blur_restated(r["counts"], sigma) - r["grid"]).max()), bound)
    assert d.grid.shape == (B, B) and d.grid.dtype == np.float64 and m <= 1.0
    # the plotted points, their indices (exact) and their colours
    assert np.array_equal(d.x, r["X"]) and np.array_equal(d.y, r["Y"])
    assert np.array_equal(d.ix, r["ix"]) and np.array_equal(d.iy, r["iy"])
    if r["span"] == 0:
        assert not d.colors.any()
    else:
        cb = 3 * bound / r["span"]
        cdev = float(np.abs(d.colors - r["colors"]).max())
        print(f"colour B={B} sigma={sigma}: max deviation {cdev:.3e}, bound {cb:.3e}")
        assert margin("colour", cdev, cb) <= 1.0
        assert d.colors.min() == 0.0 and d.colors.max() == 1.0


def test_colour_indices_with_noise_and_few_traces():
    for sps, T, B in ((2, 1, 8), (3, 2, 7), (64, 3, 200)):
        y, z = record(sps, T, tail=1, noise=True, seed=13)
        d = device_density(y, z, sps, None, B, 0.5, colors=True)
        r = en.reference(y + z, sps, None, B, 0.5)
        assert np.array_equal(d.y, r["Y"]) and np.array_equal(d.ix, r["ix"]) and np.array_equal(d.iy, r["iy"])
        assert r["span"] > 0 and np.abs(d.colors - r["colors"]).max() <= 3 * en.blur_bound(0.5, r["grid"]) / r["span"]


def test_two_calls_give_the_same_bits(blur_record):
    z = 0.05 * np.random.default_rng(2).standard_normal(blur_record.size)
    arg = electrical_signal.from_device(up(blur_record), up(z))
    a = utils.eye_density(arg, 16, None, 200, 5, colors=True)
    b = utils.eye_density(arg, 16, None, 200, 5, colors=True)
    for k in ("counts", "grid", "colors", "y", "iy"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ------------------------------------------------------------------------------------------------ residency
def test_a_device_record_stays_on_the_device(blur_record):
    s = up(blur_record)
    sig = electrical_signal.from_device(s, up(np.zeros_like(blur_record)))
    t0 = dict(_lib.TRANSFERS)
    utils.eye_density(sig, 16)
    t1 = dict(_lib.TRANSFERS)
    assert t1["h2d"] == t0["h2d"] and 0 < t1["d2h"] - t0["d2h"] <= 2
    utils.eye_density(s, 16, colors=True)
    t2 = dict(_lib.TRANSFERS)
    assert t2["h2d"] == t1["h2d"] and 0 < t2["d2h"] - t1["d2h"] <= 5
    assert sig.on_device


def test_a_host_signal_never_touches_the_gpu(blur_record, monkeypatch):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the host path called {name}")
    monkeypatch.setattr(_lib, "api", Untouchable())
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the host path loaded the library")))
    t0 = dict(_lib.TRANSFERS)
    z = np.full_like(blur_record, 0.01)
    d = utils.eye_density(electrical_signal(blur_record, z), 16, 100, 50, 2, colors=True)
    r = en.reference(blur_record + z, 16, 100, 50, 2)
    assert _lib.TRANSFERS == t0
    assert np.array_equal(d.counts, r["counts"]) and np.array_equal(d.grid, r["grid"]) and np.array_equal(d.colors, r["colors"])


def test_a_complex_record_is_a_type_error(blur_record):
    c = _lib.DeviceArray.from_host(blur_record.astype(np.complex128))
    for arg in (c, electrical_signal.from_device(c), blur_record.astype(np.complex128)):
        with pytest.raises(TypeError, match=r"\.real.*\.abs\(\)"):
            utils.eye_density(arg, 16)


# ------------------------------------------------------------------------------------------------ plots
@pytest.fixture
def agg():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    yield plt
    plt.close("all")
    gv.default()


@pytest.mark.parametrize("style", ("density", "dot", "line"))
def test_plot_eye_draws_what_eye_density_computed(agg, style):
    gv(sps=16, R=1e9)
    y, z = record(16, 12, tail=3, noise=True, seed=17)
    sig = electrical_signal.from_device(up(y), up(z))
    d = utils.eye_density(sig, 16, 4096, 200, 5, colors=True)
    fig, ax = agg.subplots()
    t0 = _lib.TRANSFERS["h2d"]
    assert sig.plot_eye(style=style, ax=ax) is sig
    assert _lib.TRANSFERS["h2d"] == t0 and sig.on_device
    assert ax.get_title() == "Eye Diagram (12 traces)" and ax.get_xlabel() == "Time (2-symbol segment)" and ax.get_ylabel() == "Amplitude"
    assert ax.get_xlim() == (-1.0, 1.0) and ax.get_ylim() == (d.extent[2], d.extent[3])
    if style == "density":
        (im,) = ax.images
        assert np.array_equal(np.asarray(im.get_array()), d.grid.T) and tuple(im.get_extent()) == d.extent and im.origin == "lower"
        assert im.get_cmap().name == "jet"
    elif style == "dot":
        (sc,) = ax.collections
        assert np.array_equal(np.asarray(sc.get_offsets()), np.column_stack([d.x, d.y])) and np.array_equal(np.asarray(sc.get_array()), d.colors)
        assert np.array_equal(sc.get_sizes(), [0.1]) and sc.get_alpha() == 0.9
    else:
        assert len(ax.collections) == 12
        cmap = agg.cm.jet
        for i in (0, 11):
            lc = ax.collections[i]
            seg = np.asarray(lc.get_segments())
            assert seg.shape == (31, 2, 2)
            assert np.array_equal(seg[:, 0, 0], d.x[:31]) and np.array_equal(seg[:, 0, 1], d.y[32 * i:32 * i + 31])
            assert np.array_equal(seg[:, 1, 1], d.y[32 * i + 1:32 * i + 32])
            want = cmap(d.colors[32 * i:32 * i + 31])
            want[:, 3] = 0.05
            assert np.allclose(lc.get_colors(), want, rtol=0, atol=1e-15) and lc.get_alpha() == 0.05 and np.array_equal(lc.get_linewidths(), [1])


def test_plot_eye_caps_the_traces_at_4096(agg):
    gv(sps=2, R=1e9)
    y, _ = record(2, 4100, tail=0, seed=19)
    sig = electrical_signal.from_device(up(y))
    fig, ax = agg.subplots()
    assert sig.plot_eye(n_traces=100000, style="density", ax=ax) is sig
    assert ax.get_title() == "Eye Diagram (4096 traces)"
    d = utils.eye_density(sig, 2, 4096)
    assert d.n_traces == 4096 and np.array_equal(np.asarray(ax.images[0].get_array()), d.grid.T)
    fig2, ax2 = agg.subplots()
    sig.plot_eye(style="dot", ax=ax2)
    assert len(ax2.collections[0].get_offsets()) == 4096 * 4
    with pytest.raises(ValueError, match="Invalid style 'dots'. Choose from 'line', 'dot', or 'density'."):
        sig.plot_eye(style="dots", ax=ax2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sig.plot_eye(cmap="no_such_map", style="density", ax=ax2)
    assert any("no_such_map" in str(x.message) for x in w) and ax2.images[-1].get_cmap().name == "viridis"


def test_zz_write_the_margins():
    """Last in the file: the largest measured deviation over its bound, with the bound beside it (EYE_DENSITY_MARGINS names the file)."""
    assert MARGINS["blur"][1] is not None, "the blur sweep has not run"
    lines = ["# tests/test_eye_density_gpu.py: largest measured deviation / bound over the sweep, and the bound at that case"]
    for k, (m, b) in MARGINS.items():
        lines.append(f"{k:24s} margin {m:.4f}   bound {b:.6e}")
    print("\n".join(lines))
    path = os.environ.get("EYE_DENSITY_MARGINS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert MARGINS["blur"][0] <= 1.0 and MARGINS["colour"][0] <= 1.0
