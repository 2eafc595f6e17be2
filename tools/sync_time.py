#!/usr/bin/env python3
"""Time the data-aided receiver on the GPU: lab.SYNC and lab.GET_EYE_v2 on a PRBS-15 x 16 record (524 272 samples) with a transmitted word of
l = 8176 samples (511 slots), against the SciPy restatement (tests/sync_numpy.py) on the same host and against GET_EYE here.

Per function: the wall time of a call on device-resident inputs after a first call (a host clock around work that ends in a device
synchronise), the time between two HIP events on the default stream around the call (torch), both over --reps calls; the kernel launches and
blocking host waits per call are the code's own counts.  The CPU figure is the median wall time of the restatement on the host's arrays.

    python tools/sync_time.py [--reps 20] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opticomlib_amd as oa  # noqa: E402
import sync_numpy as sn  # noqa: E402
from opticomlib_amd import _lib, lab  # noqa: E402

# launches / blocking host waits per call, counted in lab.py and csrc/sync.hip, csrc/eye.hip, csrc/ssfm_host.hip
COUNTS = {
    "SYNC": "13 launches (template 1, table 4, load 1, convolution 3, peak 4; + 1 for the cut), 2 waits (the plan's stream, the state read) + 1 for the cut",
    "GET_EYE_v2": "2 prepare + 7 levels + 2 count + 3 split = 14 launches, 5 waits (two prepares, three state reads)",
    "GET_EYE": "see eye.round_trips",
}


def timed(fn, reps):
    import torch
    fn()                                                        # first call: plans, tables, code objects
    fn()
    wall, ev = [], []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        res = fn()
        end.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(start.elapsed_time(end))
    return res, float(np.median(wall)), float(np.min(wall)), float(np.median(ev))


def cpu_timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return res, float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    sps, nslots = 16, 2 ** 15 - 1
    oa.gv(sps=sps, R=1e9, N=nslots)
    tx = oa.PRBS(order=15)                                      # device-resident
    word = oa.binary_sequence.from_device(_lib.DeviceArray.from_host(tx.data[:511].copy(), np.uint8))
    sig = oa.DAC(tx, pulse_shape="gaussian")
    rng = np.random.default_rng(0)
    delay = 3001
    v = np.roll(np.real(np.asarray(sig.signal)), delay) + rng.normal(0, 0.05, sig.size)
    rec = oa.devices._wrap_out(oa.electrical_signal, _lib.DeviceArray.from_host(v, np.float64), oa.NULL)
    bits_h, word_h = np.asarray(tx.data), np.asarray(tx.data[:511])
    lines = [f"record: PRBS-15 x {sps} = {v.size} samples, gaussian pulses, noise sigma 0.05, delay {delay}; word: 511 slots, l = {511 * sps} samples",
             f"{a.reps} timed calls after two untimed ones; wall = host clock around the call and a device synchronise, event = HIP events on the default stream"]
    (s_dev, i), w, wmin, e = timed(lambda: lab.SYNC(rec, word), a.reps)
    r, c, cmin = cpu_timed(lambda: sn.sync(v, word_h, sps), a.reps)
    assert i == r["i"] == delay, (i, r["i"])
    lines.append(f"SYNC        device wall median {w:.3f} ms (min {wmin:.3f}), event median {e:.3f} ms; SciPy restatement median {c:.3f} ms (min {cmin:.3f}); i = {i}; {COUNTS['SYNC']}")
    vs = np.asarray(s_dev.signal)
    shifted = np.roll(bits_h, 0)
    srec = oa.devices._wrap_out(oa.electrical_signal, _lib.DeviceArray.from_host(vs, np.float64), oa.NULL)
    for ns in (4096, 1 << 15):
        ev2, w, wmin, e = timed(lambda: lab.GET_EYE_v2(srec, tx, ns), a.reps)
        r, c, cmin = cpu_timed(lambda: sn.get_eye_v2(vs, shifted, sps, ns), a.reps)
        assert abs(ev2.mu1 - r["mu1"]) < 1e-9
        lines.append(f"GET_EYE_v2  nslots {ns}: device wall median {w:.3f} ms (min {wmin:.3f}), event median {e:.3f} ms; SciPy restatement median {c:.3f} ms (min {cmin:.3f}); "
                     f"{COUNTS['GET_EYE_v2']}")
        eb, w, wmin, e = timed(lambda: oa.GET_EYE(srec, ns), a.reps)
        lines.append(f"GET_EYE     nslots {ns}: device wall median {w:.3f} ms (min {wmin:.3f}), event median {e:.3f} ms; round trips {eb.round_trips}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
