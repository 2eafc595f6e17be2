"""The four-step transform (csrc/ssfm_kernels.hpp k_time / k_freq) and the tables it is consumed through, held bin by bin and sample by sample to the
bounds derived in tests/fft_numpy.py, at every plan shape: log2 n = 8 ... 22, both precisions, every (SSFM_E, SSFM_EF) pair, 1, 2 and 3 rows.

A  Plan.debug_fft against the closed form (impulses) and the long-double transform (tones, white noise): every bin, and normwise.
B  apply_transfer, transfer_table + apply_table (slots 0 and 1) and table_from_field: a circular shift of impulses (exact expectation, every sample),
   a seeded unit-modulus table on an impulse (every bin of the returned field's long-double spectrum), the same with two entries exchanged on
   the host -- which must fail at exactly those two bins -- and split plans through get_field.
C  the operator tables of every fixed-step engine: gamma = 0, D~ = i theta / h, two and three steps from an impulse, every bin against
   exp(i m theta_k) w[(j k) % n]; the engine that ran is asserted.
D  the any-length transform (_ChirpZ.fourier, the signals' ('w') / ('t')) on both sides of every change of its plan's size, at the suite's own
   1e-13 max|X|, on inputs on which that bites.

Every test pins the knobs it depends on and deletes the others, makes its plans itself (never the cached get_plan) and closes them.  The worst
measured / bound of every comparison goes through tests/margins.py (digest: profiles/fft_margins.txt)."""
import numpy as np
import pytest
import scipy.fft

import fft_numpy as fn
import margins
import opticomlib_amd as oa
from opticomlib_amd import _lib, optical_signal
from opticomlib_amd.devices import _ChirpZ

pytestmark = pytest.mark.gpu

KNOBS = ("SSFM_E", "SSFM_EF", "SSFM_EF_FLY", "SSFM_SMALL", "SSFM_MEDIUM", "SSFM_MEDIUM_SPLIT", "SSFM_PHASE_TABLE", "SSFM_FORCE_FLY", "SSFM_SPLIT_ABOVE",
         "SSFM_SPLIT_LOG2M")
PREC = {fn.C64: "c64", fn.C128: "c128"}
PLANS = [(L, prec, pair) for L in range(8, 23) for prec in (fn.C64, fn.C128) for pair in (fn.PAIRS if L <= 20 else (None,))]
ROWS = (1, 2, 3)


def plan_id(v):
    L, prec, pair = v
    return f"{L}-{PREC[prec]}-" + ("default" if pair is None else f"E{pair[0]}-Ef{pair[1]}")


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def set_knobs(monkeypatch, pair=None, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if pair is not None:
        monkeypatch.setenv("SSFM_E", str(pair[0]))
        monkeypatch.setenv("SSFM_EF", str(pair[1]))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def tag(sh, pair="-"):
    return f"log2n={sh['log2n']} {PREC[sh['prec']]} E={sh['E']} Ef={sh['Ef']}" + (" (default)" if pair is None else "")


def stack(n, names, cd):
    return np.stack([fn.make_input(n, nm) for nm in names]).astype(cd)


def impulses(n, positions, cd):
    x = np.zeros((len(positions), n), cd)
    x[np.arange(len(positions)), positions] = 1
    return x


class Failures(list):
    """Collects (what, measured / bound) and records every ratio: a test states all its violations at once."""

    def check(self, what, ratio):
        margins.record(what, None, ratio, 1.0)
        print(f"{what}: {ratio:.4f}")
        if not ratio <= 1.0:
            self.append((what, ratio))


# ------------------------------------------------------------------------------------------- A: the forward transform
@pytest.mark.parametrize("case", PLANS, ids=plan_id)
def test_forward_transform_every_bin(case, monkeypatch):
    log2n, prec, pair = case
    sh = fn.shape(log2n, prec, pair)
    n, cd, coeff = sh["n"], fn.CDTYPE[prec], fn.fwd_coeff(sh)
    names = fn.input_names(sh)
    set_knobs(monkeypatch, pair)
    bad = Failures()
    for rows in ROWS:
        worst = {}
        p = _lib.Plan(n, rows, prec)
        try:
            for batch in fn.batches(names, rows):
                p.set_field(stack(n, batch, cd))
                X = p.debug_fft()
                for r, nm in enumerate(batch):
                    pb, nw = fn.forward_errors(X[r], nm, n, coeff)
                    worst[nm[0], "per bin"] = max(worst.get((nm[0], "per bin"), 0.0), pb)
                    if nw is not None:
                        worst[nm[0], "normwise"] = max(worst.get((nm[0], "normwise"), 0.0), nw)
        finally:
            p.close()
        for (kind, how), r in worst.items():
            bad.check(f"A {tag(sh, pair)} nrows={rows} {kind} {how}", r)
    if pair is None:                        # NumPy's own transform of the same inputs against the same bound, beside the device's
        worst = {}
        for nm in names:
            X = scipy.fft.fft(fn.make_input(n, nm).astype(cd))          # (pocketfft, as numpy.fft; single precision for complex64 in every version)
            assert X.dtype == cd
            pb, nw = fn.forward_errors(X, nm, n, coeff)
            worst[nm[0], "per bin"] = max(worst.get((nm[0], "per bin"), 0.0), pb)
            if nw is not None:
                worst[nm[0], "normwise"] = max(worst.get((nm[0], "normwise"), 0.0), nw)
        for (kind, how), r in worst.items():
            margins.record(f"A {tag(sh, pair)} numpy {kind} {how}", None, r, 1.0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------- B: table order and the inverse
def apply_paths(p, H, x):
    """y = ifft(H fft(x)) by the three ways a host table reaches k_freq."""
    p.set_field(x)
    p.apply_transfer(H)
    yield "apply_transfer", p.get_field()
    for slot in (0, 1):
        p.transfer_table(H, slot)
        p.set_field(x)
        p.apply_table(slot)
        yield f"transfer_table slot {slot}", p.get_field()


@pytest.mark.parametrize("case", PLANS, ids=plan_id)
def test_tables_and_inverse_every_sample_and_bin(case, monkeypatch):
    log2n, prec, pair = case
    sh = fn.shape(log2n, prec, pair)
    n, cd = sh["n"], fn.CDTYPE[prec]
    full = log2n <= fn.FULL_MAX_LOG2
    pos = fn.impulse_positions(sh, full)
    t_host = fn.back_coeff(sh, fn.tau_host(sh))                       # ||x||_2 = 1 throughout
    t_field = fn.back_coeff(sh, fn.fwd_coeff(sh))                     # a table the device transformed itself: every entry within fwd_coeff ||impulse||_1
    rng = np.random.default_rng(fn.seed_of("shift", n))
    shifts = (2 * int(rng.integers(0, n // 2)) + 1, n // 2 - 1)
    H, _ = fn.unit_table(n, fn.seed_of("table", n), prec)
    pair_ab = fn.swap_pair(H, fn.seed_of("pair", n))
    set_knobs(monkeypatch, pair)
    bad = Failures()
    shift_tables = [(s, fn.shift_table(n, s, prec)) for s in shifts]
    for rows in ROWS:
        p = _lib.Plan(n, rows, prec)
        try:
            # 1. circular shifts: the impulse at j comes back at (j + s) % n, every sample within the time-domain bound
            #    (above 2^16: one batch per row count -- the three impulses dealt over them -- and one slot for table_from_field)
            worst = {}
            for s, Hs in shift_tables:
                for batch in (fn.batches(pos, rows) if full else [[pos[(rows - 1 + r) % len(pos)] for r in range(rows)]]):
                    x = impulses(n, batch, cd)
                    want = impulses(n, [(j + s) % n for j in batch], np.float64)
                    for path, y in apply_paths(p, Hs, x):
                        d = np.abs(y - want)
                        worst[path] = max(worst.get(path, 0.0), float(d.max()) / t_host, float(np.sqrt((d * d).sum(axis=-1)).max()) / t_host)
                    for slot in ((0, 1) if full else ((rows - 1) % 2,)):          # the table made on the device from the impulse at s (row 0)
                        p.set_field(impulses(n, [s] + [(s + 1 + r) % n for r in range(rows - 1)], cd))
                        p.table_from_field(slot)
                        p.set_field(x)
                        p.apply_table(slot)
                        d = np.abs(p.get_field() - want)
                        worst["table_from_field"] = max(worst.get("table_from_field", 0.0), float(d.max()) / t_field,
                                                        float(np.sqrt((d * d).sum(axis=-1)).max()) / t_field)
            for path, r in worst.items():
                bad.check(f"B {tag(sh, pair)} shift, every sample: {path}", r)
            # 2. a seeded unit-modulus table on impulses: every bin of the returned field's long-double spectrum
            batch = [pos[(rows + r) % len(pos)] for r in range(rows)]
            for i, (path, y) in enumerate(apply_paths(p, H, impulses(n, batch, cd))):
                if not full and i != rows - 1:                      # (above 2^16: path i with i + 1 rows, its last row)
                    continue
                for r in (range(rows) if full else (rows - 1,)):
                    v, ratio = fn.spectrum_violations(y[r], H, batch[r], np.sqrt(n) * t_host)
                    bad.check(f"B {tag(sh, pair)} unit table, every bin: {path}", ratio)
            # 3. the same comparison must see ONE misplaced entry: two entries exchanged on the host fail at exactly those two bins
            if rows == 1:
                p.set_field(impulses(n, batch, cd))
                p.apply_transfer(fn.swapped(H, pair_ab))
                v, ratio = fn.spectrum_violations(p.get_field()[0], H, batch[0], np.sqrt(n) * t_host)
                margins.record(f"B {tag(sh, pair)} unit table, two entries exchanged (must exceed 1)", None, ratio, 1.0)
                assert sorted(v.tolist()) == sorted(pair_ab) and ratio > 1, (pair_ab, v[:8], ratio)
        finally:
            p.close()
    assert not bad, bad


@pytest.mark.parametrize("log2n, prec, above", [(21, fn.C64, 20), (21, fn.C128, 20), (22, fn.C64, 20), (22, fn.C128, 20), (23, fn.C64, None)],
                         ids=["21-c64", "21-c128", "22-c64", "22-c128", "23-c64-real"])
def test_split_plans_transfer_every_sample_and_bin(log2n, prec, above, monkeypatch):
    """k_make_split_table + split_freq: apply_transfer on plans of 2 and 4 sub-sequences (SSFM_SPLIT_ABOVE=20) and on a real split plan of 2^23 x 1."""
    sh = fn.split_shape(log2n, prec)
    n, cd = sh["n"], fn.CDTYPE[prec]
    rows = 1 if above is None else 2
    t_host = fn.back_coeff(sh, fn.tau_host(sh))
    set_knobs(monkeypatch, None, **({} if above is None else {"SSFM_SPLIT_ABOVE": above}))
    pos = [n - 1, n // 2 - 1][:rows]
    s = 2 * int(np.random.default_rng(fn.seed_of("shift", n)).integers(0, n // 2)) + 1
    H, _ = fn.unit_table(n, fn.seed_of("table", n), prec)
    pair_ab = fn.swap_pair(H, fn.seed_of("pair", n))
    bad = Failures()
    p = _lib.Plan(n, rows, prec)
    try:
        for call in (p.debug_fft, lambda: p.transfer_table(H, 0), lambda: p.table_from_field(0)):          # direct plans only
            with pytest.raises(_lib.SsfmError):
                call()
        x = impulses(n, pos, cd)
        for sft in (s, n // 2 - 1):
            p.set_field(x)
            p.apply_transfer(fn.shift_table(n, sft, prec))
            d = np.abs(p.get_field() - impulses(n, [(j + sft) % n for j in pos], np.float64))
            bad.check(f"B split log2n={log2n} {PREC[prec]} R={sh['R']} shift, every sample", max(float(d.max()), float(np.sqrt((d * d).sum(axis=-1)).max())) / t_host)
        p.set_field(x)
        p.apply_transfer(H)
        v, ratio = fn.spectrum_violations(p.get_field()[rows - 1], H, pos[rows - 1], np.sqrt(n) * t_host)
        bad.check(f"B split log2n={log2n} {PREC[prec]} R={sh['R']} unit table, every bin", ratio)
        if above is not None:                                       # (the 2^23 plan: one long-double transform of that size is enough)
            p.set_field(x)
            p.apply_transfer(fn.swapped(H, pair_ab))
            v, ratio = fn.spectrum_violations(p.get_field()[0], H, pos[0], np.sqrt(n) * t_host)
            margins.record(f"B split log2n={log2n} {PREC[prec]} R={sh['R']} unit table, two entries exchanged (must exceed 1)", None, ratio, 1.0)
            assert sorted(v.tolist()) == sorted(pair_ab) and ratio > 1, (pair_ab, v[:8], ratio)
    finally:
        p.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------- C: the operator tables of the propagation engines
TWO_KERNEL_SIZES = (8, 12, 17, 18, 20, 21)


def fly_shape(L, prec, ef):
    """Rows that form exp(D~ h) in the kernel hold SSFM_EF_FLY points per thread, except in the 16-byte-unit layout, whose order is tied to Ef: the
    complex64 plans of 2^12 ... 2^20 points keep Ef whatever the knob says (PlanT::init), so their two fly cases run the same rows and differ from
    each other only where the knob is honoured -- complex64 at 2^8, and every complex128 size.  They stay: they are the cases that found the knob
    pairing bins with other bins' operators in that layout, and they would find it again."""
    sh = fn.shape(L, prec)
    return sh if sh["u16"] else fn.shape(L, prec, (sh["E"], ef))


ROUTES = {}          # name -> (knobs, precisions -> sizes, engine, rows, the shape the bound is written for)
ROUTES["small"] = (dict(SSFM_SMALL=1, SSFM_MEDIUM=0), {fn.C64: (8, 13), fn.C128: (8, 12)}, "small", 1, lambda L, prec: fn.small_shape(L, prec))
ROUTES["medium"] = (dict(SSFM_MEDIUM=1), {fn.C64: (13, 17)}, "medium", 1, lambda L, prec: fn.shape(L, prec))
ROUTES["value tables"] = (dict(SSFM_SMALL=0, SSFM_MEDIUM=0, SSFM_PHASE_TABLE=0), {fn.C64: TWO_KERNEL_SIZES, fn.C128: TWO_KERNEL_SIZES}, "two_kernel", 2,
                          lambda L, prec: fn.shape(L, prec))
ROUTES["phase tables"] = (dict(SSFM_SMALL=0, SSFM_MEDIUM=0, SSFM_PHASE_TABLE=1), {fn.C64: TWO_KERNEL_SIZES, fn.C128: TWO_KERNEL_SIZES}, "two_kernel", 2,
                          lambda L, prec: fn.shape(L, prec))
for ef in (8, 16):
    ROUTES[f"fly Ef={ef}"] = (dict(SSFM_SMALL=0, SSFM_MEDIUM=0, SSFM_FORCE_FLY=1, SSFM_EF_FLY=ef), {fn.C64: TWO_KERNEL_SIZES, fn.C128: TWO_KERNEL_SIZES}, "two_kernel", 2,
                              lambda L, prec, ef=ef: fly_shape(L, prec, ef))
ROUTES["split"] = (dict(SSFM_SPLIT_ABOVE=20), {fn.C64: (21,), fn.C128: (21,)}, "split", 2, lambda L, prec: fn.split_shape(L, prec))
ROUTE_CASES = [(name, prec, L) for name, r in ROUTES.items() for prec, sizes in r[1].items() for L in sizes]


@pytest.mark.parametrize("route, prec, log2n", ROUTE_CASES, ids=[f"{r.replace(' ', '-').replace('=', '')}-{PREC[p]}-{L}" for r, p, L in ROUTE_CASES])
def test_operator_tables_of_every_engine(route, prec, log2n, monkeypatch):
    knobs, sizes, engine, rows, shape_of = ROUTES[route]
    sh = shape_of(log2n, prec)
    n, cd = sh["n"], fn.CDTYPE[prec]
    h = 0.5                                                           # a power of two: D~ = i theta / h and D~ h are exact in the plan's type
    theta = np.random.default_rng(fn.seed_of("table", n)).uniform(-np.pi, np.pi, n).astype(_lib._RDTYPE[prec])
    tau = fn.tau_device(sh, np.pi, phase_table=(route == "phase tables" or (route in ("medium", "split") and prec == fn.C64)))
    pos = [n - 1, n // 2 - 1][:rows]
    set_knobs(monkeypatch, None, **knobs)
    bad = Failures()

    def run(p, th, m):
        p.set_linear_operator((1j * th.astype(np.float64) / h).astype(cd))
        p.set_field(impulses(n, pos, cd))
        p.propagate_fixed(0.0, np.full(m, h))
        info = p.last_run_info()
        if info["fell_back"]:                                       # the one-launch engine's workgroups did not meet: the run was repeated, and is compared
            assert engine == "medium" and info["fallbacks_total"] >= 1, info
        else:
            assert info["engine"] == engine, (info, engine)         # otherwise the case is vacuous
        return p.get_field()

    p = _lib.Plan(n, rows, prec)
    try:
        for m in (2, 3):
            y = run(p, theta, m)
            r = m % rows                                             # (one row per run goes through the long-double transform)
            v, ratio = fn.spectrum_violations(y[r], fn.expi(theta, m), pos[r], np.sqrt(n) * fn.back_coeff(sh, tau, m))
            bad.check(f"C {route} log2n={log2n} {PREC[prec]} m={m}, every bin", ratio)
        if log2n == min(sizes[prec]):                                # once per route and precision: one misplaced entry is seen, at exactly its two bins
            a, b = fn.swap_pair(fn.expi(theta).astype(np.complex128), fn.seed_of("pair", n))
            y = run(p, fn.swapped(theta, (a, b)), 2)
            v, ratio = fn.spectrum_violations(y[0], fn.expi(theta, 2), pos[0], np.sqrt(n) * fn.back_coeff(sh, tau, 2))
            margins.record(f"C {route} log2n={log2n} {PREC[prec]} m=2, two entries exchanged (must exceed 1)", None, ratio, 1.0)
            assert sorted(v.tolist()) == sorted((a, b)) and ratio > 1, ((a, b), v[:8], ratio)
    finally:
        p.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------- D: the any-length transform
LENGTHS = (2, 3, 127, 128, 129, 2048, 2049, 4099, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 21)


def any_length_inputs(n):
    """(name, x, fft(x) in long double): the impulse at n - 1, the tone on bin n - 1, white noise; complex64 values."""
    out = []
    for name in (("impulse", n - 1), ("tone", n - 1), ("white", 1)):
        x = fn._make_input(n, name)
        out.append((name[0], x, fn.impulse_spectrum_any(n, n - 1) if name[0] == "impulse" else fn.ld_fft_raw(x)))
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_any_length_transform_both_directions(n, monkeypatch):
    set_knobs(monkeypatch, None)
    inputs = any_length_inputs(n)
    back = (-np.arange(n)) % n                                        # ifft(x)[m] = fft(x)[-m mod n] / n, exactly
    bad = Failures()
    for rows in ROWS:
        for members in ([[0], [1], [2]] if rows == 1 else [[0, 1], [2, 0]] if rows == 2 else [[0, 1, 2]]):
            x = np.stack([inputs[i][1] for i in members])
            for inverse in (False, True):
                if rows < 3:                                         # the signals' own call: one or two polarisations
                    got = optical_signal(x[0] if rows == 1 else x)("t" if inverse else "w").signal.reshape(rows, n)
                else:
                    buf = _lib.DeviceArray.from_host(np.ascontiguousarray(x), np.complex128, 0)
                    with _ChirpZ(n, rows, 0) as eng:
                        got = eng.fourier(buf, inverse).to_host()
                    buf.free()
                assert got.dtype == np.complex128
                for r, i in enumerate(members):
                    ref = inputs[i][2][back] / fn.LD(n) if inverse else inputs[i][2]
                    ratio = float(np.max(np.abs(got[r].astype(fn.CLD) - ref)) / (1e-13 * np.max(np.abs(ref))))
                    bad.check(f"D len={n} nrows={rows} {'ifft' if inverse else 'fft'} {inputs[i][0]} [max |d| / (1e-13 max |X|)]", ratio)
    assert not bad, bad


def test_any_length_transform_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError, match="no CPU fallback"):
        optical_signal(np.ones((1 << 21) + 1, np.complex64))("w")
