"""CPU-side checks of ``eye.plot`` (opticomlib_amd.typing.eye.plot / show, EyeShowOptions, opticomlib_amd.utils.eye_fold_density, the fold entry
points of csrc/eye_density.hip): the host path draws what the reference drew (tests/golden/eyeplot_*.npz, recorded by
tests/golden/make_golden_eye_plot.py), the fold's index rules hold against brute force under AddressSanitizer / UBSan (tests/eye_plot_host.cpp),
and the C ABI carries the new entry points.  No GPU."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eye_plot_cases as pc
import eye_plot_numpy as pn
import opticomlib_amd as oa
from opticomlib_amd import _lib, utils
from opticomlib_amd.typing import EyeShowOptions, eye

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssfm_eye_fold_range", "ssfm_eye_fold_density")


@pytest.fixture
def agg():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    yield plt
    plt.close("all")


def case_bounds(name):
    """``(bound, vspan)`` of a case's picture from NumPy / SciPy on this machine: the blur bound of its grid and max - min of its counts."""
    c = pc.CASES[name]
    r = pn.reference(pc.record(name), c["sps"], c.get("resamp"))
    return pn.blur_bound(r["grid"]), float(r["counts"].max() - r["counts"].min())


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_host_path_draws_what_the_reference_drew(agg, golden_dir, name):
    want = np.load(os.path.join(golden_dir, f"eyeplot_{name}.npz"))
    c = pc.CASES[name]
    if not c.get("empty"):
        kw = pc.eye_kwargs(name, reference=True)
        assert np.array_equal(want["in_y"], kw["y"])
        assert json.loads(str(want["in_scalars"])) == {k: v for k, v in kw.items() if k not in ("y", "t")}
    got = pc.run(name, eye, EyeShowOptions)
    assert str(got["kind"]) == str(want["kind"]), got.get("error_text")
    if str(want["kind"]) == "error":
        assert str(got["error_type"]) == str(want["error_type"]) and str(got["error_text"]) == str(want["error_text"])
        return
    bound, vspan = case_bounds(name)
    stored = {k: want[k] for k in want.files if k not in ("versions", "in_y", "in_scalars", "kind")}
    got.pop("kind")
    pn.compare(got, stored, bound, vspan, smooth_hist=c["kw"].get("smooth", True) and bool(c["opts"].get("histogram") or c["opts"].get("all_none")),
               cmap=c["kw"].get("cmap", "winter"))


def test_the_goldens_hold_the_cases_they_are_meant_to(golden_dir):
    """What makes a case hard is in its fixture: no drawn trace, a partial last trace, an empty window, NaN colours, shared columns."""
    g = lambda name: np.load(os.path.join(golden_dir, f"eyeplot_{name}.npz"))
    assert int(g("sps2_n2_lines_hist")["ax0_n_collections"]) == 0 and int(g("sps2_n2_lines_hist")["ax1_n_patches"]) == 1
    assert np.isnan(g("sps2_n2_lines_hist")["ax1_patch0_xy"]).any() and np.isnan(g("empty_window")["ax1_patch0_xy"]).any()      # 0 / 0: no point in the window
    assert int(g("sps3_lines")["ax0_n_collections"]) == (6 * 3 - 3) // 6 == 2
    assert int(g("sps16_lines")["ax0_n_collections"]) == (64 * 16 - 16) // 32 == 31                                         # 1008 points: 31 traces and a half
    assert int(g("resamp32_lines_hist")["ax0_n_collections"]) == (16 * 32 - 8) // 16 == 31 and g("resamp32_lines_hist")["ax0_first_segments"].shape == (15, 2, 2)
    assert not g("const_lines_hist")["ax0_first_colors"][:, :3].any()                                                          # NaN colours: the map's "bad" entry
    assert g("sps256_lines_hist")["ax0_first_segments"].shape == (511, 2, 2)
    assert int(g("no_y_left")["ax0_n_lines"]) == 0 and str(g("no_threshold")["error_type"]) == "TypeError"
    assert str(g("err_style")["error_type"]) == "TypeError" and str(g("err_empty")["error_text"]) == "Empty eye diagram object."


def test_eye_fold_density_on_the_host_is_numpy_and_scipy():
    for name, window in (("sps16_lines_hist", (-0.05, 0.05)), ("resamp32_lines_hist", (-0.2, 0.01)), ("sps3_lines", (0.3, 0.4)), ("sps2_n2_smooth", None)):
        c = pc.CASES[name]
        y = pc.record(name)
        e = eye(**pc.eye_kwargs(name))
        d = utils.eye_fold_density(e, colors=True, hist=window)
        r = pn.reference(y, c["sps"], c.get("resamp"), window)
        assert isinstance(d, utils.EyeFoldDensity) and d.n_traces == r["n_traces"] and d.extent == r["extent"]
        assert d.counts.dtype == np.uint32 and np.array_equal(d.counts, r["counts"]) and np.array_equal(d.grid, r["grid"])
        assert d.xedges.tobytes() == r["xedges"].tobytes() and d.yedges.tobytes() == r["yedges"].tobytes()
        k = r["k"]
        assert np.array_equal(d.x, r["t"][:k]) and np.array_equal(d.y, r["y"][:k]) and np.array_equal(d.ix, r["it"][:k]) and np.array_equal(d.iy, r["iy"][:k])
        assert np.array_equal(d.colors, r["colors"][:k], equal_nan=True)
        if window is None:
            assert d.hist_counts is None and d.hist_edges is None and d.n_masked is None
        else:
            assert np.array_equal(d.hist_counts, r["hist_counts"]) and d.hist_edges.tobytes() == r["hist_edges"].tobytes() and d.n_masked == r["n_masked"]
    plain = utils.eye_fold_density(e)
    assert plain.colors is None and plain.x is None and plain.grid.shape == (350, 350)
    assert oa.eye_fold_density is utils.eye_fold_density and {"eye_fold_density", "EyeShowOptions"} <= set(oa.__all__) and "eye_fold_density" in utils.__all__


def test_the_host_tables_are_the_restatements(agg):
    """What the device path hands the kernels -- each phase's column, colour index and mask -- against the reference's per-point expressions."""
    for sps, s, n in ((2, 2, 4), (3, 3, 18), (16, 16, 1024), (256, 256, 2048), (8, 32, 512), (16, 16, 1000), (4, 4, 7)):
        t_, y_ = pn.fold(np.arange(n, dtype=np.float64), sps, s)
        tg = np.linspace(-1, 1 - 1 / s, 2 * s)
        window = (-0.3, 0.26)
        m, xe, xbin, xidx, mask = utils._fold_tables(tg, len(t_), window)
        H, xe_np, _ = np.histogram2d(t_, y_, bins=350)
        assert xe.tobytes() == xe_np.tobytes() and m == min(len(t_), 2 * s)
        phase = np.arange(len(t_)) % (2 * s)
        assert np.array_equal(np.bincount(xbin[phase], minlength=350), H.sum(axis=1))
        assert np.all(np.diff(xbin) >= 0) and xbin.min() >= 0 and xbin.max() < 350
        with np.errstate(all="ignore"):
            it = np.clip(((t_ - t_.min()) / (t_.max() - t_.min()) * 349).astype(int), 0, 349)
        assert np.array_equal(xidx[phase], it)
        assert np.array_equal(mask[phase].astype(bool), (t_ > window[0]) & (t_ < window[1]))


def test_errors_are_raised_before_anything_is_computed():
    for e in (eye(), eye(sps=4, y=np.zeros(16)), eye(y=np.zeros(16), t_opt=0.0)):
        with pytest.raises(ValueError, match=r"^Empty eye diagram object\.$"):
            utils.eye_fold_density(e)
        with pytest.raises(ValueError, match=r"^Empty eye diagram object\.$"):
            e.plot()
    kw = pc.eye_kwargs("sps16_lines")
    for bad in (np.nan, np.inf, -np.inf):
        y = kw["y"].copy()
        y[500] = bad
        with pytest.raises(ValueError, match=r"autodetected range of \[.*\] is not finite"):
            utils.eye_fold_density(eye(**dict(kw, y=y)))
    y = kw["y"].copy()
    y[:16] = np.nan                                                  # outside the fold: the first sps samples are not plotted
    clean = utils.eye_fold_density(eye(**kw))
    assert np.array_equal(utils.eye_fold_density(eye(**dict(kw, y=y))).counts, clean.counts)


def test_show_options_and_signatures_are_the_references():
    o = EyeShowOptions()
    assert vars(o) == dict(averages=False, threshold=False, cross_points=False, legends=False, t_opt=False, histogram=False)
    assert all(vars(EyeShowOptions(all_none=True)).values())
    assert vars(EyeShowOptions(t_opt=False, histogram=True, all_none=True)) == dict(averages=True, threshold=True, cross_points=True, legends=True,
                                                                                     t_opt=False, histogram=True)
    assert list(inspect.signature(EyeShowOptions.__init__).parameters) == ["self", "averages", "threshold", "cross_points", "legends", "t_opt", "histogram", "all_none"]
    p = inspect.signature(eye.plot).parameters
    assert list(p) == ["self", "show_options", "hlines", "vlines", "style", "cmap", "smooth", "title", "savefig", "ax"]
    assert (p["hlines"].default, p["vlines"].default, p["style"].default, p["cmap"].default, p["smooth"].default, p["title"].default, p["savefig"].default,
            p["ax"].default) == ([], [], "dark", "winter", True, "", None, None)
    assert vars(p["show_options"].default) == vars(o)
    assert oa.EyeShowOptions is EyeShowOptions and callable(eye.show)
    assert "__str__" not in vars(eye) and "print" not in vars(eye)


def test_plot_on_given_axes_and_savefig(agg, tmp_path):
    e = eye(**pc.eye_kwargs("sps16_smooth"))
    fig, ax = agg.subplots()
    before = agg.get_fignums()
    assert e.plot(ax=ax, savefig=str(tmp_path / "eye.png")) is e
    assert agg.get_fignums() == before and len(ax.images) == 1 and os.path.getsize(tmp_path / "eye.png") > 0
    assert ax.get_xlabel() == r"Time [$t/T_{slot}$]" and ax.get_ylabel() == "Amplitude [V]"
    assert isinstance(e.__dict__["_y"], np.ndarray)


# ------------------------------------------------------------------------------------------------ the fold's index rules under the sanitizers
def test_fold_index_drawn_rule_and_mask_against_brute_force(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "eye_plot_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{os.path.join(ROOT, 'opticomlib_amd', 'csrc')}", "-o", exe, os.path.join(ROOT, "tests", "eye_plot_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout[-2000:] + out.stderr[-4000:]
    src = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "eye_density.hip")).read()
    for rule in ("eye_fold_sample(", "eye_fold_phase(", "eye_fold_drawn(", "eye_fold_masked(", "eye_fold_check(", "EyeFold"):
        assert rule in src.split('#include "eye_density.inc"')[1], rule
    inc = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "eye_density.inc")).read()
    for fn in re.findall(r"EYE_HD inline \w+(?: \w+)* (eye_fold_\w+)\(", inc):          # every fold function is one a kernel or an entry point calls
        assert fn + "(" in src, fn


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_carries_the_fold_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    assert "#define SSFM_ABI_VERSION 3" in hdr
    vers = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ssfm_\*;", vers)                    # the map exports the ssfm_ prefix: the new names fall under it
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert f"SSFM_API int {s}(" in hdr and s in _lib.SYMBOLS and s in names, s
        assert getattr(lib, s).argtypes == _lib.SYMBOLS[s][1]
    assert {n for n in names if n.startswith("ssfm_eye_fold")} == set(NEW_SYMBOLS)
    assert {n for n in names if n.startswith("ssfm_")} == set(_lib.SYMBOLS)
    assert set(re.findall(r"\bssfm_eye_fold\w*", hdr)) == set(NEW_SYMBOLS)       # every name the header writes is a symbol
    assert re.search(r"typing\.py:2577-2808 \(eye\.plot.*ssfm_eye_fold_range", hdr)   # the reference-line table
    assert lib.ssfm_abi_version() == 3
    assert (utils.EYE_PLOT_BINS, utils.EYE_PLOT_SIGMA, utils.EYE_PLOT_HIST_BINS) == (350, 3, 200) and utils.EYE_PLOT_BINS <= utils.EYE_MAX_BINS
