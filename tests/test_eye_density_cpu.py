"""CPU-side checks of the eye diagram (opticomlib_amd.utils.eye_density / eyediagram, electrical_signal.plot_eye, csrc/eye_density.hip): the host path
draws what the reference drew (tests/golden/eyediagram_*.npz, recorded by tests/golden/make_golden_eyediagram.py), the integer rules the kernels
compile hold against brute force under AddressSanitizer / UBSan (tests/eye_density_host.cpp), and the C ABI carries the new entry points.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eye_density_numpy as en
import eyediagram_cases as ec
import opticomlib_amd as oa
from opticomlib_amd import _lib, utils
from opticomlib_amd.typing import electrical_signal, gv, optical_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssfm_eye_density_range", "ssfm_eye_density")


@pytest.fixture
def agg():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    yield plt
    plt.close("all")
    gv.default()


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_the_host_path_draws_what_the_reference_drew(agg, golden_dir, name):
    want = np.load(os.path.join(golden_dir, f"eyediagram_{name}.npz"))
    y, z = ec.record(name)
    assert np.array_equal(want["in_signal"], y) and (z is None) == ("in_noise" not in want.files)
    if z is not None:
        assert np.array_equal(want["in_noise"], z)
    gv.default()
    got = ec.run(name, utils.eyediagram, electrical_signal, gv)
    assert str(got["kind"]) == str(want["kind"])
    if str(want["kind"]) == "error":
        assert str(got["error_type"]) == str(want["error_type"]) and str(got["error_text"]) == str(want["error_text"])
        return
    assert set(got) == set(want.files) - {"versions", "in_signal", "in_noise"}
    c = ec.CASES[name]
    sigma, B = c["kw"].get("grid_sigma", 5), c["kw"].get("N_grid_bins", 200)
    # the blur bound of this case, from NumPy / SciPy on this machine
    r = en.reference(y if z is None else y + z, c["sps"], min(c["kw"].get("n_traces", 4096), 4096) if c["call"] == "plot_eye" else c["kw"].get("n_traces"), B, sigma)
    bound = en.blur_bound(sigma, r["grid"])
    for k in ("title", "xlabel", "ylabel", "origin", "cmap", "first_capstyle", "first_joinstyle", "last_capstyle", "last_joinstyle", "grid_on",
              "n_images", "n_collections"):                            # strings and integers: equal
        if k in got:
            assert got[k].tolist() == want[k].tolist(), k
    for k in ("xlim", "ylim", "extent", "offsets", "sizes", "alpha", "first_segments", "last_segments", "first_linewidth", "last_linewidth",
              "first_alpha", "last_alpha"):                            # floats the blur never touches: equal
        if k in got:
            assert np.array_equal(got[k], want[k]), k
    if "image" in got:                                                 # floats that pass through the blur
        assert got["image"].shape == want["image"].shape == (B, B)
        assert np.abs(got["image"] - want["image"]).max() <= bound
    if "colour_array" in got:
        tol = 3 * bound / r["span"] if r["span"] else 0.0
        assert np.abs(got["colour_array"] - want["colour_array"]).max() <= tol
    for k in ("first_colors", "last_colors"):                          # RGBA from the colour map's 256-entry table: at most one entry apart
        if k in got:
            assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max() <= 0.05, k


def test_eye_density_on_the_host_is_numpy_and_scipy():
    y, z = ec.record("sps16_noise_line_cap")
    d = utils.eye_density(electrical_signal(y, z), 16, 4, 50, 2, colors=True)
    r = en.reference(y + z, 16, 4, 50, 2)
    assert isinstance(d, utils.EyeDensity) and d.n_traces == 4
    assert d.counts.dtype == np.uint32 and np.array_equal(d.counts, r["counts"]) and np.array_equal(d.grid, r["grid"])
    assert d.xedges.tobytes() == r["xedges"].tobytes() and d.yedges.tobytes() == r["yedges"].tobytes()
    assert np.array_equal(d.x, r["X"]) and np.array_equal(d.y, r["Y"]) and np.array_equal(d.ix, r["ix"]) and np.array_equal(d.iy, r["iy"])
    assert np.array_equal(d.colors, r["colors"]) and d.extent == (r["X"].min(), r["X"].max(), r["Y"].min(), r["Y"].max())
    plain = utils.eye_density(list(y), 16, 4, 50, 2)
    assert plain.colors is None and plain.x is None and plain.grid.shape == (50, 50)
    with pytest.raises(TypeError, match=r"\.real.*\.abs\(\)"):
        utils.eye_density(y.astype(complex), 16)
    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        utils.eye_density(np.where(np.arange(y.size) == 50, np.nan, y), 16)
    assert oa.eye_density is utils.eye_density and oa.eyediagram is utils.eyediagram and {"eye_density", "eyediagram"} <= set(oa.__all__)


def test_the_restated_rules_are_numpys_and_scipys():
    """The host-side tables the kernels are handed: the bins of values among linspace edges, SciPy's weights, and the float64 restatement of the blur."""
    rng = np.random.default_rng(4)
    for B in (1, 2, 7, 8, 200, 350):
        v = rng.uniform(-0.3, 1.7, 4000)
        v[:2] = -0.3, 1.7
        edges = utils._hist_edges(v.min(), v.max(), B)
        v[2:B + 3] = edges                                              # the edge values themselves
        want = np.histogram(v, bins=B)
        assert want[1].tobytes() == edges.tobytes()
        assert np.array_equal(np.bincount(utils._hist_bins(edges, v), minlength=B), want[0])
        for sigma in (0, 0.5, 3, 5):
            c = rng.integers(0, 40, (B, B)).astype(np.float64)
            ref = en.gaussian_filter(c, sigma=sigma)
            assert np.abs(en.blur_restated(c, sigma) - ref).max() <= en.blur_bound(sigma, ref)
            r, w = utils._gauss_weights(sigma)
            assert r == en.radius(sigma) and (w is None) == (sigma == 0)
    assert utils._hist_edges(2.0, 2.0, 4).tolist() == [1.5, 1.75, 2.0, 2.25, 2.5]


def test_plot_eye_is_electrical_only_and_caps_the_traces(agg):
    assert not hasattr(optical_signal, "plot_eye")
    assert "plot_eye" not in electrical_signal.__doc__.split("Not provided:")[1]
    gv(sps=2, R=1e9)
    y = np.random.default_rng(1).standard_normal(2 + 4100 * 4)
    sig = electrical_signal(y)
    fig, ax = agg.subplots()
    assert sig.plot_eye(style="density", ax=ax, N_grid_bins=16) is sig
    assert ax.get_title() == "Eye Diagram (4096 traces)"
    fig, ax = agg.subplots()
    assert sig.plot_eye(n_traces=5000, style="dot", ax=ax, N_grid_bins=16) is sig
    assert len(ax.collections[0].get_offsets()) == 4096 * 4
    with pytest.warns(UserWarning, match="no_such_map"):
        sig.plot_eye(cmap="no_such_map", style="density", ax=ax, N_grid_bins=16)
    assert ax.images[-1].get_cmap().name == "viridis"
    created = utils.eyediagram(y[:200], 2, style="density", N_grid_bins=8)          # no axes given: a new figure's
    assert created.figure.get_dpi() == 100 and created.get_title() == "Eye Diagram (49 traces)"


# ------------------------------------------------------------------------------------------------ the kernels' integer rules under the sanitizers
def test_bin_rule_reflect_index_and_geometry_against_brute_force(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "eye_density_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{os.path.join(ROOT, 'opticomlib_amd', 'csrc')}", "-o", exe, os.path.join(ROOT, "tests", "eye_density_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout[-2000:] + out.stderr[-4000:]
    src = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "eye_density.hip")).read()
    assert '#include "eye_density.inc"' in src                       # the kernels compile the same text
    for rule in ("eye_bin(", "eye_reflect(", "eye_geometry(", "eye_grid_index("):
        assert rule in src.split('#include "eye_density.inc"')[1], rule


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_carries_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    assert "#define SSFM_ABI_VERSION 3" in hdr
    vers = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ssfm_\*;", vers)                    # the map exports the ssfm_ prefix: the new names fall under it
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and f"SSFM_API int {s}(int device" not in hdr and s in _lib.SYMBOLS and s in names, s
        assert getattr(lib, s).argtypes == _lib.SYMBOLS[s][1]
    assert {n for n in names if n.startswith("ssfm_eye_density")} == set(NEW_SYMBOLS)
    assert lib.ssfm_abi_version() == 3
    mk = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "Makefile")).read()
    assert "eye_density.hip" in mk and "eye_density.inc" in mk
    assert utils.EYE_CHUNK_POINTS == int(re.search(r"kChunkPoints = (\d+);", open(os.path.join(ROOT, "opticomlib_amd", "csrc", "eye_density.hip")).read()).group(1))
