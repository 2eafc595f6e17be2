"""The cases behind tests/golden/eyeplot_*.npz: what tests/golden/make_golden_eye_plot.py runs on the reference's ``eye.plot`` and
tests/test_eye_plot_cpu.py / tests/test_eye_plot_gpu.py on this library's.  A case: the record (``sps`` samples per slot, ``nslots`` slots,
``resamp``: samples per slot of the record and of its time grid instead, ``const``: every sample that value), the eye's scalars that differ from
:data:`SCALARS`, the ``EyeShowOptions`` (``opts``) and ``plot``'s other arguments (``kw``).  ``sub7``: the stored image and alpha array are
``[::7, ::7]`` of the drawn ones, with their sums beside them (a 350 x 350 float64 image that does not compress is 980 kB).  The files are
``eyeplot_*``, not ``eye_plot_*``: tests/test_eye_cpu.py takes every ``eye_*.npz`` for a fixture of ``GET_EYE``."""
import numpy as np

ALL = dict(all_none=True)
SCALARS = dict(t_left=-0.5, t_right=0.5, t_opt=0.0, t_dist=1.0, t_span0=-0.05, t_span1=0.05, y_left=0.5, y_right=0.5, mu0=0.0, mu1=1.0, s0=0.1, s1=0.1,
               threshold=0.5)

CASES = {
    "sps2_n2_smooth": dict(sps=2, nslots=2, opts=dict(), kw=dict()),                                       # 2 points, 0 drawn traces
    "sps2_n2_lines_hist": dict(sps=2, nslots=2, opts=dict(histogram=True), kw=dict(smooth=False)),         # ... and nothing within the span
    "sps3_lines": dict(sps=3, nslots=6, opts=ALL, kw=dict(smooth=False)),
    "sps16_smooth": dict(sps=16, nslots=64, opts=dict(), kw=dict(), sub7=True),
    "sps16_smooth_hist": dict(sps=16, nslots=64, opts=ALL, kw=dict(title="of the case"), sub7=True),
    "sps16_lines": dict(sps=16, nslots=64, opts=dict(t_opt=True, averages=True), kw=dict(smooth=False, cmap="plasma")),
    "sps16_lines_hist": dict(sps=16, nslots=64, opts=ALL, kw=dict(smooth=False)),
    "sps16_light_lines": dict(sps=16, nslots=64, opts=ALL, kw=dict(style="light", hlines=[0.25, 0.75], vlines=[-0.25], smooth=False)),
    "sps16_light_smooth": dict(sps=16, nslots=64, opts=dict(threshold=True, legends=True), kw=dict(style="light", hlines=[0.2], vlines=[0.1, 0.3]), sub7=True),
    "sps256_smooth_hist": dict(sps=256, nslots=8, opts=dict(histogram=True), kw=dict(), sub7=True),        # 2 sps >= 350: phases share columns
    "sps256_lines_hist": dict(sps=256, nslots=8, opts=dict(histogram=True), kw=dict(smooth=False)),
    "resamp32_lines_hist": dict(sps=8, resamp=32, nslots=16, opts=ALL, kw=dict(smooth=False)),             # L = 16 != P = 64
    "resamp32_smooth_hist": dict(sps=8, resamp=32, nslots=16, opts=dict(histogram=True), kw=dict(), sub7=True),
    "const_lines_hist": dict(sps=16, nslots=8, const=0.75, opts=dict(histogram=True), kw=dict(smooth=False)),
    "const_smooth_hist": dict(sps=16, nslots=8, const=0.75, opts=dict(histogram=True), kw=dict()),
    "empty_window": dict(sps=16, nslots=64, scalars=dict(t_opt=1 / 32, t_dist=1e-6, t_span0=1 / 32 - 5e-8, t_span1=1 / 32 + 5e-8),
                         opts=dict(histogram=True, t_opt=True), kw=dict(smooth=False)),
    "no_y_left": dict(sps=16, nslots=16, scalars=dict(y_left=None, y_right=None), opts=dict(cross_points=True), kw=dict()),
    "no_threshold": dict(sps=16, nslots=16, scalars=dict(threshold=None), opts=dict(threshold=True), kw=dict()),
    "err_style": dict(sps=16, nslots=16, opts=dict(), kw=dict(style="neon")),
    "err_empty": dict(empty=True, opts=dict(), kw=dict()),
}


def record(name):
    """The eye's record ``y`` of a case (float64, ``nslots * (resamp or sps)`` samples): an OOK-like signal, one level per slot plus noise."""
    c = CASES[name]
    s = c.get("resamp") or c["sps"]
    n = c["nslots"] * s
    if "const" in c:
        return np.full(n, float(c["const"]))
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    return np.repeat(rng.integers(0, 2, c["nslots"]).astype(np.float64), s) + 0.1 * rng.standard_normal(n)


def eye_kwargs(name, y=None, reference=False):
    """The keyword arguments that build the case's eye: the reference's takes its time grid ``t``, this library's the number of slots behind it.
    ``y``: the record to hand over instead of the host array (a DeviceArray)."""
    c = CASES[name]
    if c.get("empty"):
        return {}
    sps = c["sps"]
    s = c.get("resamp") or sps
    kw = dict(SCALARS, sps=sps, dt=1e-9 / sps, y=record(name) if y is None else y, i=sps // 2, execution_time=0.0)
    kw.update(c.get("scalars", {}))
    if "resamp" in c:
        kw["sps_resamp"] = s
    if reference:
        kw["t"] = np.kron(np.ones(c["nslots"] // 2), np.linspace(-1, 1 - 1 / s, 2 * s))
    else:
        kw["_nslots"] = c["nslots"]
    return kw


def _stored_image(a, sub7):
    a = np.asarray(a, dtype=np.float64)
    return (a[::7, ::7], np.array(a.sum())) if sub7 else (a, np.array(a.sum()))


def artists(fig, sub7=False):
    """The data of what was drawn on the figure: arrays and strings only."""
    from matplotlib.collections import LineCollection
    out = {"n_axes": np.array(len(fig.axes)), "suptitle": np.array(fig._suptitle.get_text() if fig._suptitle is not None else "")}
    for k, ax in enumerate(fig.axes):
        p = f"ax{k}_"
        out.update({p + "xlabel": np.array(ax.get_xlabel()), p + "ylabel": np.array(ax.get_ylabel()), p + "title": np.array(ax.get_title()),
                    p + "xlim": np.array(ax.get_xlim(), dtype=np.float64), p + "ylim": np.array(ax.get_ylim(), dtype=np.float64),
                    p + "xticks": np.array(ax.get_xticks(), dtype=np.float64), p + "facecolor": np.array(ax.get_facecolor(), dtype=np.float64),
                    p + "n_images": np.array(len(ax.images)), p + "n_collections": np.array(len(ax.collections)),
                    p + "n_lines": np.array(len(ax.lines)), p + "n_patches": np.array(len(ax.patches)),
                    p + "legend": np.array([t.get_text() for t in ax.get_legend().get_texts()] if ax.get_legend() else [], dtype=str)})
        if ax.images:
            im = ax.images[0]
            image, total = _stored_image(im.get_array(), sub7)
            alpha, alpha_total = _stored_image(im.get_alpha(), sub7)
            out.update({p + "image": image, p + "image_sum": total, p + "image_alpha": alpha, p + "image_alpha_sum": alpha_total,
                        p + "extent": np.array(im.get_extent(), dtype=np.float64), p + "origin": np.array(im.origin),
                        p + "cmap": np.array(im.get_cmap().name), p + "interpolation": np.array(str(im.get_interpolation()))})
        lcs = [c for c in ax.collections if isinstance(c, LineCollection)]
        assert len(lcs) == len(ax.collections)
        for tag, lc in (("first", lcs[0]), ("last", lcs[-1])) if lcs else ():
            out.update({p + f"{tag}_segments": np.asarray(lc.get_segments(), dtype=np.float64), p + f"{tag}_colors": np.asarray(lc.get_colors(), dtype=np.float64),
                        p + f"{tag}_linewidth": np.asarray(lc.get_linewidths(), dtype=np.float64), p + f"{tag}_alpha": np.array(lc.get_alpha())})
        for i, ln in enumerate(ax.lines):
            q = p + f"line{i}_"
            from matplotlib.colors import to_rgba
            out.update({q + "x": np.asarray(ln.get_xdata(), dtype=np.float64), q + "y": np.asarray(ln.get_ydata(), dtype=np.float64),
                        q + "color": np.array(to_rgba(ln.get_color()), dtype=np.float64), q + "linestyle": np.array(str(ln.get_linestyle())),
                        q + "marker": np.array(str(ln.get_marker())), q + "alpha": np.array(np.nan if ln.get_alpha() is None else ln.get_alpha()),
                        q + "label": np.array(str(ln.get_label()))})
        for i, pa in enumerate(ax.patches):                          # the step histogram: one polygon
            out.update({p + f"patch{i}_xy": np.asarray(pa.get_xy(), dtype=np.float64),
                        p + f"patch{i}_edgecolor": np.array(pa.get_edgecolor(), dtype=np.float64), p + f"patch{i}_fill": np.array(bool(pa.get_fill()))})
    return out


def run(name, eye, EyeShowOptions, y=None, reference=False):
    """Run a case on an implementation under a non-interactive backend; returns the dict that is stored (``kind`` 'plot' or 'error')."""
    import warnings
    import matplotlib.pyplot as plt
    c = CASES[name]
    plt.close("all")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                          # (0 / 0 of a constant record or an empty histogram: the picture is the outcome)
            e = eye(**eye_kwargs(name, y, reference))
            ret = e.plot(EyeShowOptions(**c["opts"]), **c["kw"])
            assert ret is e
            out = {"kind": np.array("plot"), **artists(plt.gcf(), c.get("sub7", False))}
    except Exception as ex:          # noqa: BLE001 -- the type and text are the recorded outcome
        out = {"kind": np.array("error"), "error_type": np.array(type(ex).__name__), "error_text": np.array(str(ex))}
    finally:
        plt.close("all")
    return out
