#!/usr/bin/env python3
"""Generate the fixtures of the optical_signal algebra, ``optical_*.npz``, by importing the reference and running every case of
``tests/optical_cases.py`` on its classes (a development host only).

    python tests/golden/make_golden_optical.py [--reference ../reference]

``optical_inputs.npz`` holds the operands (``<name>/signal``, ``<name>/noise``; the electrical ones as ``el:<name>/...``; the host arrays by
their names); ``optical_<group>.npz`` holds, per case, what the reference returned -- ``<case>|kind`` ('signal', 'bits', 'array' or 'error')
with the arrays that go with it, or the exception's type and text.  Data only, at most 2 x 257 samples per operand.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402
import optical_cases as oc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    _, typing = import_reference(args.reference)
    import scipy
    typing.gv.default()
    v = oc.namespace(typing.optical_signal, typing.electrical_signal)
    groups = {g: {} for g in oc.GROUPS}
    kinds = {}
    for cid, fn in oc.cases():
        group, name = cid.split("/", 1)
        res = oc.outcome(fn, v, typing.NULL)
        kinds[str(res["kind"])] = kinds.get(str(res["kind"]), 0) + 1
        for k, a in res.items():
            groups[group][f"{name}|{k}"] = a
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}")
    ins = {k: a for k, a in oc.arrays().items()}
    for prefix, items in (("", oc.inputs()), ("el:", oc.electrical())):
        for name, (s, n) in items.items():
            ins[prefix + name + "/signal"] = s
            if n is not None:
                ins[prefix + name + "/noise"] = n
    np.savez_compressed(os.path.join(HERE, "optical_inputs.npz"), versions=versions, **ins)
    for g, d in groups.items():
        path = os.path.join(HERE, f"optical_{g}.npz")
        np.savez_compressed(path, versions=versions, **d)
        print(g, len({k.split("|")[0] for k in d}), "cases", os.path.getsize(path), "bytes")
    print(kinds)


if __name__ == "__main__":
    main()
