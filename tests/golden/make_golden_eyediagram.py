#!/usr/bin/env python3
"""Generate the fixtures of the eye diagram, ``eyediagram_*.npz``, by importing the reference and running every case of
``tests/eyediagram_cases.py`` on its ``eyediagram`` / ``electrical_signal.plot_eye`` under the Agg backend (a development host only).

    python tests/golden/make_golden_eyediagram.py [--reference ../reference]

Each file holds data only: the record (``in_signal``, ``in_noise``), and of what the reference drew the image array with its extent and origin,
the scatter's offsets, colour array, sizes and alpha, the number of line collections with the first and the last one's segments, colours,
linewidth and alpha, the title, labels and limits -- or the exception's type and text -- and the NumPy / SciPy versions.
"""
from __future__ import annotations

import argparse
import os
import sys

os.environ["MPLBACKEND"] = "Agg"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402
import eyediagram_cases as ec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    _, typing = import_reference(args.reference)
    from opticomlib import utils
    import matplotlib
    import scipy
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}; matplotlib {matplotlib.__version__}")
    for name in ec.CASES:
        typing.gv.default()
        out = ec.run(name, utils.eyediagram, typing.electrical_signal, typing.gv)
        y, z = ec.record(name)
        extra = {"in_signal": y}
        if z is not None:
            extra["in_noise"] = z
        path = os.path.join(HERE, f"eyediagram_{name}.npz")
        np.savez_compressed(path, versions=versions, **extra, **out)
        print(name, str(out["kind"]), str(out.get("error_text", "")), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
