"""Every engine's launchers once, for comparing two builds of the library dispatch by dispatch (profiles/launchers_trace.txt).

    [SSFM_LIB=/other/_ssfm_amd.so] rocprofv3 --kernel-trace -f csv -d DIR -- python3 tools/launcher_walk.py --out DIR/outputs.txt
    python3 tools/launcher_walk.py --compare DIR_A DIR_B

The walk prints one line per run: its name, the engine the plan names, whether it fell back, the launch count and the sha256 of the output.  The
comparison reads the two kernel traces in dispatch order as (kernel name, grid, workgroup, LDS bytes, scratch bytes) and the two outputs files.
All of a step's launches are issued from the calling thread (SSFM_LANE_THREADS=0), so that the order of dispatches does not depend on two threads' luck.
"""
import csv
import glob
import hashlib
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk(out_path):
    for k in [k for k in os.environ if k.startswith("SSFM_") and k != "SSFM_LIB"]:
        del os.environ[k]
    os.environ["SSFM_LANE_THREADS"] = "0"
    import numpy as np
    import opticomlib_amd as oa
    from opticomlib_amd import _lib, workloads
    from opticomlib_amd.typing import gv, optical_signal

    gv(**workloads.BENCH_GV)
    lines = []

    def note(name, info, launches, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        lines.append(f"{name:44s} engine={info['engine']:22s} fell_back={int(info['fell_back'])} launches={launches:4d} sha256={h.hexdigest()}")
        print(lines[-1], flush=True)

    def with_env(env):
        for k in ("SSFM_SMALL", "SSFM_MEDIUM", "SSFM_MEDIUM_ADAPT", "SSFM_PHASE_TABLE", "SSFM_SPLIT_ABOVE", "SSFM_ADAPT_FUSED"):
            os.environ.pop(k, None)
        os.environ.update(env)
        oa.devices.release_plans()              # (a plan reads its knobs when it is made)

    def plan_run(name, log2n, rows, prec, env, adaptive=False):
        with_env(env)
        n = 1 << log2n
        a = workloads.qpsk_field(max(n, 1 << 12), seed=log2n, power_w=8e-3, n_pol=2)[:, :n]
        a = np.concatenate([a, 0.5 * a])[:rows]
        p = _lib.Plan(n, rows, prec)
        try:
            p.set_linear_operator(oa.devices.linear_operator(n, gv.dt, 0.2, -21.7, 0.13, prec))
            p.set_field(a)
            if adaptive:
                steps, z, _ = p.propagate_adaptive(1.3, 2.0, 0.004, False)
                extra = (np.asarray(z),)
            else:
                p.propagate_fixed(1.3, np.array([0.5] * 5 + [0.25], dtype=np.float32 if prec == _lib.C64 else np.float64))
                extra = ()
            f = p.get_field()
            note(name, p.last_run_info(), p.last_propagate_ms()[1], f, *extra)
        finally:
            p.close()

    def fiber_run(name, n, npol, M, plan_prec, env, **kw):
        with_env(env)
        a = workloads.qpsk_field(1 << max(12, (n - 1).bit_length()), seed=n % 997, power_w=4e-3, n_pol=2)[:npol, :n]
        out = oa.FIBER(optical_signal(a if npol > 1 else a[0]), **kw)
        p = oa.devices.get_plan(M, npol, plan_prec, 0)
        note(name + " (" + str(out.engine) + ")", p.last_run_info(), p.last_propagate_ms()[1], out.signal)

    C64, C128 = _lib.C64, _lib.C128
    off = dict(SSFM_SMALL="0", SSFM_MEDIUM="0")
    plan_run("two-kernel 2^18 x 2 c64", 18, 2, C64, {})
    plan_run("two-kernel 2^14 x 2 c128", 14, 2, C128, {})
    plan_run("two-kernel 2^12 x 2 c64, value tables", 12, 2, C64, dict(off, SSFM_PHASE_TABLE="0"))
    plan_run("small 2^10 x 3 c64", 10, 3, C64, {})
    plan_run("small 2^9 x 2 c128", 9, 2, C128, {})
    plan_run("small 2^13 x 1 c64", 13, 1, C64, dict(SSFM_MEDIUM="0"))
    plan_run("small adaptive 2^9 x 2 c64", 9, 2, C64, {}, adaptive=True)
    plan_run("small adaptive 2^11 x 1 c128", 11, 1, C128, {}, adaptive=True)
    plan_run("medium 2^14 x 2, phase tables", 14, 2, C64, {})
    plan_run("medium 2^14 x 2, value tables", 14, 2, C64, dict(SSFM_PHASE_TABLE="0"))
    plan_run("medium 2^12 x 2 (64 x 64)", 12, 2, C64, dict(SSFM_SMALL="0"))
    plan_run("medium 2^16 x 2, a launch per row", 16, 2, C64, {})
    plan_run("medium adaptive 2^14 x 2", 14, 2, C64, {}, adaptive=True)
    plan_run("medium adaptive 2^12 x 2 (64 x 64)", 12, 2, C64, dict(SSFM_SMALL="0"), adaptive=True)
    plan_run("adaptive, two launches per step 2^18 x 2", 18, 2, C64, {}, adaptive=True)
    plan_run("adaptive, three launches per step 2^18 x 2", 18, 2, C64, dict(SSFM_ADAPT_FUSED="0"), adaptive=True)
    smf = workloads.SMF
    fiber_run("chirp small 200 x 2", 200, 2, 512, C64, {}, length=3.0, h=0.5, **smf)
    fiber_run("chirp small adaptive 200 x 2", 200, 2, 512, C64, {}, length=2.0, phi_max=0.004, **smf)
    fiber_run("chirp small 1000 x 2 c128", 1000, 2, 2048, C128, {}, length=3.0, h=0.5, precision="complex128", **smf)
    fiber_run("chirp medium 3000 x 2", 3000, 2, 8192, C64, {}, length=3.0, h=0.5, **smf)
    fiber_run("chirp medium adaptive 3000 x 2", 3000, 2, 8192, C64, {}, length=2.0, phi_max=0.004, **smf)
    fiber_run("chirp line 3000 x 2 c128", 3000, 2, 8192, C128, {}, length=3.0, h=0.5, precision="complex128", **smf)
    fiber_run("complex64 on the complex128 line 100003 x 2", 100003, 2, 1 << 18, C128, {}, length=3.0, h=0.5, **smf)
    plan_run("split 2^21 x 1 c64", 21, 1, C64, dict(SSFM_SPLIT_ABOVE="20"))
    plan_run("split adaptive 2^21 x 1 c64", 21, 1, C64, dict(SSFM_SPLIT_ABOVE="20"), adaptive=True)
    oa.devices.release_plans()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def dispatches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"{directory}: {len(files)} kernel traces")
    rows = list(csv.DictReader(open(files[0])))
    col = lambda *parts: [c for c in rows[0] if all(p in c.lower() for p in parts)]
    keys = col("kernel_name") + col("grid_size") + col("workgroup_size") + (col("lds") or col("group_segment")) + (col("scratch") or col("private_segment"))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return keys, [tuple(r[k] for k in keys) for r in rows]


def compare(dir_a, dir_b):
    ka, a = dispatches(dir_a)
    kb, b = dispatches(dir_b)
    print("columns:", ", ".join(ka))
    print(f"dispatches: {len(a)} against {len(b)}; distinct kernels: {len({r[0] for r in a})} against {len({r[0] for r in b})}")
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    print("sequence in dispatch order:", "identical" if ka == kb and first is None else f"FIRST DIFFERENCE at dispatch {first}: {a[first:first + 1]} against {b[first:first + 1]}")
    ca, cb = Counter(a), Counter(b)
    print("as multisets:", "identical" if ca == cb else f"DIFFERENT: {list((ca - cb).items())[:5]} against {list((cb - ca).items())[:5]}")
    oa_, ob_ = (open(os.path.join(d, "outputs.txt")).read().splitlines() for d in (dir_a, dir_b))
    bad = [(x, y) for x, y in zip(oa_, ob_) if x != y]
    print(f"outputs: {len(oa_)} against {len(ob_)} runs,", "every line (engine, fall-back flag, launch count, sha256 of the output) equal" if not bad and len(oa_) == len(ob_) else f"DIFFERENT: {bad[:3]}")
    for line in oa_:
        print("   ", line)
    return 0 if (ka == kb and first is None and ca == cb and not bad and len(oa_) == len(ob_)) else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    walk(sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else None)
