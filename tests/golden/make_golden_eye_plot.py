#!/usr/bin/env python3
"""Generate the fixtures of ``eye.plot``, ``eyeplot_*.npz``, by importing the reference and running every case of ``tests/eye_plot_cases.py``
on its ``typing.eye(**kw).plot(...)`` under the Agg backend (a development host only).  The eye is built from a synthetic record and stated
scalars: no ``GET_EYE`` runs.

    python tests/golden/make_golden_eye_plot.py [--reference ../reference]

Each file holds data only: the record (``in_y``) and the eye's scalars (``in_scalars``, JSON), and of what the reference drew, per axes, the
image array with its extent and alpha array, the number of line collections with the first and the last one's segments and colours, every line's
data, colour and linestyle, the step histogram's polygon, labels, limits, ticks, legend texts and the figure's title -- or the exception's type
and text -- and the NumPy / SciPy / matplotlib versions.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

os.environ["MPLBACKEND"] = "Agg"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402
import eye_plot_cases as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    _, typing = import_reference(args.reference)
    import matplotlib
    import scipy
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}; matplotlib {matplotlib.__version__}")
    for name in pc.CASES:
        out = pc.run(name, typing.eye, typing.EyeShowOptions, reference=True)
        kw = pc.eye_kwargs(name, reference=True)
        extra = {"in_scalars": np.array(json.dumps({k: v for k, v in kw.items() if k not in ("y", "t")}, sort_keys=True))}
        if "y" in kw:
            extra["in_y"] = kw["y"]
        path = os.path.join(HERE, f"eyeplot_{name}.npz")
        np.savez_compressed(path, versions=versions, **extra, **out)
        print(name, str(out["kind"]), str(out.get("error_text", "")), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
