"""The cases behind tests/golden/eyediagram_*.npz: what tests/golden/make_golden_eyediagram.py runs on the reference's ``eyediagram`` / ``plot_eye`` and
tests/test_eye_density_cpu.py on this library's host path.  A case: ``call`` ('eyediagram' on an array, 'plot_eye' on an electrical_signal with
``gv.sps = sps``), the record (``traces`` whole traces after the cut plus ``tail`` samples; ``const``: every sample that value; ``n``: that many
samples instead), ``noise``, and the arguments."""
import numpy as np

CASES = {
    "sps2_t1_dot": dict(call="eyediagram", sps=2, traces=1, tail=1, kw=dict(N_grid_bins=8, grid_sigma=5, style="dot")),
    "sps3_t2_line": dict(call="eyediagram", sps=3, traces=2, tail=0, kw=dict(N_grid_bins=8, grid_sigma=5, style="line", cmap="plasma")),
    "sps3_t300_dot": dict(call="eyediagram", sps=3, traces=300, tail=4, kw=dict(style="dot")),
    "sps16_t300_density": dict(call="plot_eye", sps=16, traces=300, tail=9, kw=dict(style="density")),
    "sps16_noise_line_cap": dict(call="plot_eye", sps=16, traces=6, tail=3, noise=True, kw=dict(n_traces=4, style="line", N_grid_bins=50, grid_sigma=2)),
    "sps16_noise_density_kw": dict(call="plot_eye", sps=16, traces=5, tail=0, noise=True,
                                   kw=dict(style="density", N_grid_bins=8, grid_sigma=5, cmap="viridis", xlabel="t", ylabel="v",
                                           title="{num_traces} of them", xlim=(-0.5, 0.5), ylim=(-1, 2), grid=False)),
    "const_dot": dict(call="eyediagram", sps=16, traces=3, tail=0, const=0.75, kw=dict(style="dot")),
    "const_density": dict(call="eyediagram", sps=2, traces=2, tail=0, const=-1.0, kw=dict(style="density", N_grid_bins=8, grid_sigma=0.5)),
    "err_too_short": dict(call="eyediagram", sps=16, n=8, kw=dict()),
    "err_few_points": dict(call="eyediagram", sps=16, n=40, kw=dict()),
    "err_no_trace": dict(call="eyediagram", sps=16, traces=3, tail=0, kw=dict(n_traces=0)),
    "err_style": dict(call="eyediagram", sps=2, traces=2, tail=0, kw=dict(style="dots")),
}


def record(name):
    """``(signal, noise or None)`` of a case, float64."""
    c = CASES[name]
    sps = c["sps"]
    n = c["n"] if "n" in c else 2 * (sps // 2) + c["traces"] * 2 * sps + c["tail"]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    if "const" in c:
        y = np.full(n, float(c["const"]))
    else:
        y = rng.integers(0, 2, n).astype(np.float64) + 0.1 * rng.standard_normal(n)
    z = 0.05 * rng.standard_normal(n) if c.get("noise") else None
    return y, z


def artists(ax):
    """The data of what was drawn on ``ax``: arrays and strings only."""
    out = {"title": np.array(ax.get_title()), "xlabel": np.array(ax.get_xlabel()), "ylabel": np.array(ax.get_ylabel()),
           "xlim": np.array(ax.get_xlim(), dtype=np.float64), "ylim": np.array(ax.get_ylim(), dtype=np.float64),
           "grid_on": np.array(any(line.get_visible() for line in ax.get_xgridlines())),
           "n_images": np.array(len(ax.images)), "n_collections": np.array(len(ax.collections))}
    if ax.images:
        im = ax.images[0]
        out.update(image=np.asarray(im.get_array(), dtype=np.float64), extent=np.array(im.get_extent(), dtype=np.float64), origin=np.array(im.origin),
                   cmap=np.array(im.get_cmap().name))
    from matplotlib.collections import LineCollection
    if ax.collections and not isinstance(ax.collections[0], LineCollection):
        sc = ax.collections[0]
        out.update(offsets=np.asarray(sc.get_offsets(), dtype=np.float64), colour_array=np.asarray(sc.get_array(), dtype=np.float64),
                   sizes=np.asarray(sc.get_sizes(), dtype=np.float64), alpha=np.array(sc.get_alpha()), cmap=np.array(sc.get_cmap().name))
    elif ax.collections:
        for tag, lc in (("first", ax.collections[0]), ("last", ax.collections[-1])):
            out.update({f"{tag}_segments": np.asarray(lc.get_segments(), dtype=np.float64), f"{tag}_colors": np.asarray(lc.get_colors(), dtype=np.float64),
                        f"{tag}_linewidth": np.asarray(lc.get_linewidths(), dtype=np.float64), f"{tag}_alpha": np.array(lc.get_alpha()),
                        f"{tag}_capstyle": np.array(str(lc.get_capstyle())), f"{tag}_joinstyle": np.array(str(lc.get_joinstyle()))})
    return out


def run(name, eyediagram, electrical_signal, gv):
    """Run a case on an implementation under a non-interactive backend; returns the dict that is stored (``kind`` 'plot' or 'error')."""
    import matplotlib.pyplot as plt
    c = CASES[name]
    y, z = record(name)
    fig, ax = plt.subplots()
    try:
        if c["call"] == "plot_eye":
            gv(sps=c["sps"], R=1e9)
            sig = electrical_signal(y) if z is None else electrical_signal(y, z)
            ret = sig.plot_eye(ax=ax, **c["kw"])
            assert ret is sig
        else:
            ret = eyediagram(y, c["sps"], ax=ax, **c["kw"])
            assert ret is ax
        out = {"kind": np.array("plot"), **artists(ax)}
    except Exception as e:          # noqa: BLE001 -- the type and text are the recorded outcome
        out = {"kind": np.array("error"), "error_type": np.array(type(e).__name__), "error_text": np.array(str(e))}
    finally:
        plt.close(fig)
    return out
