#!/usr/bin/env python3
"""Generate the fixtures of the binary_sequence algebra, ``bits_*.npz``, by importing the reference and running every case of
``tests/bits_cases.py`` on its class (a development host only).

    python tests/golden/make_golden_bits.py [--reference ../reference]

``bits_inputs.npz`` holds the operands by their names (the string operand as a 0-d string array); ``bits_<group>.npz`` holds, per case, what the
reference returned -- ``<case>|kind`` ('bits', 'int', 'signal', 'array' or 'error') with the array that goes with it, or the exception's type
and text.  Data only, at most 300 bits per operand.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

from make_golden import import_reference  # noqa: E402
import bits_cases as bc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPTICOMLIB_REFERENCE", "../reference"))
    args = ap.parse_args()
    _, typing = import_reference(args.reference)
    import scipy
    typing.gv.default()
    v = bc.namespace(typing.binary_sequence, typing.gv)
    groups = {g: {} for g in bc.GROUPS}
    kinds = {}
    for cid, fn in bc.cases():
        group, name = cid.split("/", 1)
        res = bc.outcome(fn, v)
        kinds[str(res["kind"])] = kinds.get(str(res["kind"]), 0) + 1
        for k, a in res.items():
            groups[group][f"{name}|{k}"] = a
    versions = np.array(f"numpy {np.__version__}; scipy {scipy.__version__}")
    ins = {k: np.asarray(a) for k, a in bc.arrays().items()}
    ins.update(bc.inputs())
    np.savez_compressed(os.path.join(HERE, "bits_inputs.npz"), versions=versions, **ins)
    for g, d in groups.items():
        path = os.path.join(HERE, f"bits_{g}.npz")
        np.savez_compressed(path, versions=versions, **d)
        print(g, len({k.rsplit("|", 1)[0] for k in d}), "cases", os.path.getsize(path), "bytes")
    print(kinds)


if __name__ == "__main__":
    main()
