#!/usr/bin/env python3
"""Where the K of tests/psd_numpy.py comes from: SciPy's own float64 Welch against the long-double reference on every input of
tests/test_psd_edges_gpu.py, in the unit of the bound, r = max_k |p_scipy - p_ref| / (u T A_k).  No GPU: the module's bodies run with
SciPy in the device's place, so every input, segment count and bin subset is the test's own (the SciPy-only inputs get 16 seeded bins of
the reference here, 4 at nperseg = 2^21).

    python tools/psd_bound_survey.py [raw_margins.txt]

prints the largest r per group of cases and overall; K = ceil(4 x that)."""
import collections
import math
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(raw):
    os.environ["SSFM_MARGINS_FILE"] = raw
    os.environ["SSFM_MARGINS_ONLY"] = "1"
    import test_psd_edges_gpu as T
    from opticomlib_amd import utils

    def scipy_as_device(x, L):
        p = T.scipy_psd(x, L)
        return p.astype(np.float32) if np.asarray(x).dtype == np.complex64 else p
    T.device_psd, T.device_psd_f64 = scipy_as_device, T.scipy_psd
    for L in T.POW2:
        for kind in T.KINDS:
            for domain in T.DOMAINS:
                T.run_route1(L, kind, domain)
        print("route 1", L, flush=True)
    for case in T.BIG_SPLITS:
        T.run_route1_target(*case, survey_bins=16)
    for P in range(1, 16):
        T.run_route2(P)
    print("route 2", flush=True)
    for L in T.SEAM_L:
        T.run_route3_seams(L, lambda b: setattr(utils, "CHUNK_BYTES", b))
    for case in T.ROW_LIMITS:
        T.run_row_limit(*case, survey_bins=16)
    T.run_size_limit(survey_bins=16)
    worst = collections.OrderedDict()
    for line in open(raw):
        if " scipy r " not in line:                  # (the `sg.welch r` records are SciPy's own mean; not what K is measured on)
            continue
        what, _s, measured, _b, _q = line.split(" | ", 1)[1].rsplit(" | ", 4)
        key = re.sub(r"\b(n|chunk)=\d+ ", "", what.split(" scipy r ")[0])
        key = re.sub(r" (white|tone|float64|complex64|complex128|\(float64 result\))", "", key)
        worst[key] = max(worst.get(key, 0.0), float(measured))
    for k, v in worst.items():
        print(f"{k:40s} r = {v:.3f}")
    r = max(worst.values())
    print(f"max r = {r:.3f}  ->  K = ceil(4 r) = {math.ceil(4 * r)}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(tempfile.mkdtemp(), "psd_survey_margins.txt"))
