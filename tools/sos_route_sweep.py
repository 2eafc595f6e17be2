"""The SOS filter on every route of tests/test_sos_edges_gpu.py's ROUTES table, in one process: sections 1, 2 and 4, real and complex, 2 rows of
2 groups + 1 sample of the route's layout; host buffers once, device buffers once out of place and once in place.  Prints the route each call
reported and a SHA-256 of its result -- two libraries with the same device code and tables print the same lines (dev aid for host-side changes):
    [SSFM_LIB=/other/_ssfm_amd.so] python tools/sos_route_sweep.py            (also under rocprofv3 --kernel-trace --stats -- python ...)
    [SSFM_LIB=...] python tools/sos_route_sweep.py --time [calls]              wall time per device call at the sizes where a call is a latency chain"""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scipy.signal as sg
from opticomlib_amd import _lib

KNOBS = ("SSFM_SOS_ONE_LAUNCH", "SSFM_SOS_NEAR", "SSFM_SOS_MEET", "SSFM_SOS_LONG_CHUNK", "SSFM_SOS_PATIENCE_US", "SOS_WAVES_FORCE")


def pin(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


def design(order, wn=0.07):
    sos = sg.bessel(order, wn, "low", norm="mag", output="sos")
    return sos, sg.sosfilt_zi(sos)


def device_call(sos, zi, x, in_place):
    xd = _lib.DeviceArray.from_host(np.ascontiguousarray(x))
    yd = xd if in_place else _lib.DeviceArray(x.shape, x.dtype)
    try:
        _lib.sosfiltfilt_device(sos, zi, xd.ptr, yd.ptr, x.shape[-1], x.size // x.shape[-1], np.iscomplexobj(x))
        return yd.to_host()
    finally:
        xd.free()
        if not in_place:
            yd.free()


def sweep():
    from test_sos_edges_gpu import ROUTES, ORDER_OF
    for name, (env, _, (W, L)) in ROUTES.items():
        for ns in (1, 2, 4):
            for cplx in (False, True):
                sos, zi = design(ORDER_OF[(ns, cplx)])
                n = 2 * 64 * W * L + 1
                rng = np.random.default_rng(ns + 10 * cplx)
                x = rng.standard_normal((2, n)) + (1j * rng.standard_normal((2, n)) if cplx else 0)
                pin(env)
                for how in ("host", "device", "in place"):
                    y = _lib.sosfiltfilt(sos, zi, x) if how == "host" else device_call(sos, zi, x, how == "in place")
                    r = _lib.sosfiltfilt_last_route()
                    print(f"{name} | sections {ns} {'complex' if cplx else 'real'} {how}: route {r} sha256 {hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()}")


def timing(calls):
    pin({})
    sos, zi = design(4)
    rng = np.random.default_rng(1)
    for what, shape, cplx in (("2^14 complex x 2", (2, 1 << 14), True), ("2^16 real", (1, 1 << 16), False), ("2^20 complex x 2", (2, 1 << 20), True)):
        x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        xd, yd = _lib.DeviceArray.from_host(np.ascontiguousarray(x)), _lib.DeviceArray(x.shape, x.dtype)
        call = lambda: _lib.sosfiltfilt_device(sos, zi, xd.ptr, yd.ptr, shape[-1], shape[0], cplx)
        for _ in range(20):
            call()
        best = []
        for _ in range(3):
            t = time.perf_counter()
            for _ in range(calls):
                call()
            best.append((time.perf_counter() - t) / calls * 1e6)
        print(f"wall {what}: {min(best):.2f} us per call (three loops of {calls}: {' '.join('%.2f' % b for b in best)}); kernels {_lib.sosfiltfilt_last_ms() * 1e3:.1f} us, route {_lib.sosfiltfilt_last_route()}")
        xd.free()
        yd.free()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        timing(int(sys.argv[2]) if len(sys.argv) > 2 else 300)
    else:
        sweep()
