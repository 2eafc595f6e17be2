"""Every adaptive engine's step sizes held to the rule h = phi_max / (|gamma| max|A|^2), peak by peak: the z log of every engine against the float64
restatement of tests/adaptive_numpy.py, on pulse fields whose maximum sits where a reduction can lose it -- the first and last sample of a row, of a tile
and of a sub-sequence, the second row, a row that takes the maximum over part-way, a peak that walks through the wrap-around, falls, or grows.

Engines (adaptive_numpy.ENGINES / CHIRP_LINES, the smallest shapes that still reach each reduction): k_small_adapt; the launch-per-pass engine's slots
(plain END / BEGIN and the tile-private unit layout); the fused column kernel with at most 64 workgroups and with the wgmax words (128 and 512 workgroups);
the one-XCD engine; the split plans' pass; the chirp-z lines in one launch (small, medium) and launch per pass (k_chirp_post / k_chirp_absmax: the
complex128 line, and the line of a complex64 caller of more than 65536 samples, which holds complex64 values between float64 passes).  The medium chirp
line holds 2^17 points in all rows, so its 65536-sample case is one row (2049 samples: two rows).

Every test makes its plans itself and closes them, pins the knobs it depends on and deletes the others, and asserts through last_run_info() that the
intended engine ran and did not fall back.

Bounds (adaptive_numpy.z_bounds; none is taken from a device's output): z[1], a pure function of the input, 5 roundings of the plan's real type; z[k], k >= 2,
complex64: 4 x max(oracle_off, (5 + k) 2^-24), oracle_off the distance of the reference's own complex64 run from the restatement; complex128: 2 TOL_C128.  Step
counts are equal (the cases leave the last, clamped step 17 ... 71 % of the step the rule gave: tests/test_adaptive_steps_cpu.py).  End fields: tol(steps) in complex64,
1e-7 in complex128, against the truth moved to the pulse's place.  The worst measured / bound of every test goes through tests/margins.py (digest:
profiles/adaptive_step_margins.txt)."""
import numpy as np
import pytest

import adaptive_numpy as an
import margins
import opticomlib_amd as oa
from opticomlib_amd import _lib
from opticomlib_amd.accuracy import TOL_C128, tol

pytestmark = pytest.mark.gpu

PREC = {an.C64: "c64", an.C128: "c128"}
CD = {an.C64: np.complex64, an.C128: np.complex128}
RT = {an.C64: np.float32, an.C128: np.float64}
ROWS = [(e, p, n, r) for e, (_, shapes) in an.ENGINES.items() for p, n, r in shapes]
# (line, the caller's precision, n, rows, SSFM_CHIRP_SMALL, the engine last_run_info names)
ROWS += [("chirp_small_c64", an.C64, 1000, 2, 1, "chirp_small_adaptive"), ("chirp_small_c64", an.C64, 2048, 2, 1, "chirp_small_adaptive"),
         ("chirp_medium_c64", an.C64, 2049, 2, 1, "chirp_medium_adaptive"), ("chirp_medium_c64", an.C64, 65536, 1, 1, "chirp_medium_adaptive"),
         ("chirp_long_c64", an.C64, 65537, 2, 1, "chirp_steps"), ("chirp_line_c128", an.C128, 1000, 2, 1, "chirp_small_adaptive"),
         ("chirp_line_c128", an.C128, 1000, 2, 0, "chirp_steps")]


def row_id(v):
    return f"{v[0]}-{PREC[v[1]]}-{v[2]}x{v[3]}" + (f"-small{v[4]}" if len(v) > 4 and v[0] == "chirp_line_c128" else "")


ROW_IDS = [row_id(v) for v in ROWS]


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


@pytest.fixture(scope="module", autouse=True)
def _drop_truths():
    yield
    an.clear_caches()


def operator(n, kw, prec):
    return oa.devices.linear_operator(n, an.DT, kw["alpha"], kw["beta_2"], kw["beta_3"], prec)


class Pow2:
    """A power-of-two plan on one of the engines of adaptive_numpy.ENGINES: ssfm_adaptive_begin / _run / _finish, the z log from _finish's z_out."""

    def __init__(self, engine, prec, n, rows):
        self.engine, self.prec, self.n, self.rows, self.op = engine, prec, n, rows, None
        self.p = _lib.Plan(n, rows, prec)

    def run(self, a, kw):
        op = (kw["alpha"], kw["beta_2"], kw["beta_3"])
        if op != self.op:
            self.p.set_linear_operator(operator(self.n, kw, self.prec))
            self.op = op
        self.p.set_field(a)
        steps, z, _ = self.p.propagate_adaptive(kw["gamma"], kw["length"], kw["phi_max"], False)
        info = self.p.last_run_info()
        assert info["engine"] == self.engine and not info["fell_back"], (info["engine"], info["fell_back"], self.engine)
        return steps, z, self.p.get_field()

    def close(self):
        self.p.close()


class Chirp:
    """A chirp-z line of n samples per row on a plan of M >= 2 n - 1 points, through the entries that return the z log without a capture:
    ssfm_chirp_propagate_c64 (the one-launch complex64 lines) and ssfm_chirp_propagate (the complex128 plan's lines; f32: a complex64 caller's step rule)."""

    def __init__(self, line, prec, n, rows, engine):
        self.line, self.prec, self.n, self.rows, self.engine = line, prec, n, rows, engine
        self.one_launch_c64 = line in ("chirp_small_c64", "chirp_medium_c64")
        M = 1 << max(8 if line != "chirp_medium_c64" else 13, (2 * n - 2).bit_length())
        self.p = _lib.Plan(M, rows, an.C64 if self.one_launch_c64 else an.C128)
        self.ld = np.complex64 if self.one_launch_c64 else np.complex128              # the line's type
        self.chirp = _lib.chirp_device(n, False, 0)
        if self.one_launch_c64:
            self.chirp = self.chirp.astype(np.complex64)
        else:
            self.p.chirp_setup(n)
            self.P = _lib.DeviceArray((rows, n), np.float64, 0)

    def run(self, a, kw):
        rt = RT[self.prec]
        A = _lib.DeviceArray.from_host(np.ascontiguousarray(a, dtype=self.ld), self.ld, 0)
        Dt = _lib.DeviceArray.from_host(np.asarray(operator(self.n, kw, self.prec), dtype=self.ld), self.ld, 0)
        g, L, phi = float(rt(kw["gamma"])), float(rt(kw["length"])), float(rt(kw["phi_max"]))
        if self.one_launch_c64:
            got = self.p.chirp_propagate_c64(A, self.chirp, Dt, g, None, length=L, phi_max=phi, max_steps=1 << 10)
            assert got is not None, "the one-launch line gave the field back"
        else:
            got = self.p.chirp_propagate(A, self.P, self.chirp, Dt, g, None, length=L, phi_max=phi, f32=self.prec == an.C64, max_steps=1 << 10)
        info = self.p.last_run_info()
        assert info["engine"] == self.engine and not info["fell_back"], (info["engine"], info["fell_back"], self.engine)
        y = A.to_host().reshape(self.rows, self.n)
        A.free()
        Dt.free()
        return got[0], got[1], y

    def close(self):
        self.chirp.free()
        if not self.one_launch_c64:
            self.P.free()
        self.p.close()


class runner:
    def __init__(self, row, monkeypatch):
        for k in an.KNOBS:
            monkeypatch.delenv(k, raising=False)
        if row[0] in an.ENGINES:
            knobs = an.ENGINES[row[0]][0]
        else:
            knobs = dict(an.CHIRP_LINES[row[0]][0], SSFM_CHIRP_SMALL=row[4])
        for k, v in knobs.items():
            monkeypatch.setenv(k, str(v))
        self.row = row

    def __enter__(self):
        row = self.row
        self.r = Pow2(*row) if row[0] in an.ENGINES else Chirp(row[0], row[1], row[2], row[3], row[5])
        return self.r

    def __exit__(self, *exc):
        self.r.close()
        return False


# ----------------------------------------------------------------------------------------------------------------- geometry
def geometry(row):
    """(C, N2, extra positions) of the plan a row runs on: C columns per k_time tile, N2 row points (csrc/ssfm_route.hpp plan_shape); a split plan: those of
    its sub-sequences, and the first and last sample of every sub-sequence and of the sub-sequence length M."""
    engine, prec, n = row[0], row[1], row[2]
    C = 16 if prec == an.C64 else 8
    extra = []
    m = n
    if engine == "split_adaptive":
        m = 1 << 20
        R = n // m
        extra = list(range(R)) + [m - 1, m]
    k = m.bit_length() - 1
    k1 = min(k // 2, 8) if k <= 20 else 9
    return C, m >> k1, extra


def positions(row, short=False):
    n = row[2]
    if row[0] not in an.ENGINES:
        return [0, 1, n // 2, n - 2, n - 1]                  # a chirp line: the samples from n to the line's size are padding and must not count
    C, N2, extra = geometry(row)
    if short or n >= (1 << 20):                              # (16 ... 32 MiB per upload)
        return sorted(set([0, N2, n - 1] + extra))
    return sorted(set([0, 1, C - 1, C, N2 - 1, N2, n // 2 - 1, n // 2, n - N2, n - C, n - 1] + extra))


# ----------------------------------------------------------------------------------------------------------------- the comparison
class Worst:
    """The worst measured / bound of a test per quantity; every violation is stated at the end."""

    def __init__(self, what):
        self.what, self.worst, self.bad = what, {}, []

    def z(self, where, steps, z, zt, prec, off):
        assert steps == len(zt) - 1 and len(z) == len(zt), (self.what, where, steps, len(zt) - 1, z, zt)
        assert z[0] == 0.0
        r = an.z_distance(z, zt) / an.z_bounds(len(zt) - 1, prec, off, TOL_C128)
        for name, v in (("z[1]", float(r[0])), ("z[k>=2]", float(r[1:].max()))):
            self.worst[name] = max(self.worst.get(name, 0.0), v)
            if not v <= 1.0:
                self.bad.append((where, name, v, list(z), list(zt)))

    def field(self, where, y, truth, bound):
        v = margins.relmax(y, truth) / bound
        self.worst["field"] = max(self.worst.get("field", 0.0), v)
        if not v <= 1.0:
            self.bad.append((where, "field", v))

    def close(self, steps):
        for name, v in self.worst.items():
            margins.record(f"{self.what} {name}", steps, v, 1.0)
            print(f"{self.what} {name}: {v:.4f}")
        assert not self.bad, self.bad


def field_bound(prec, steps):
    return tol(steps) if prec == an.C64 else 1e-7


def static_run(r, w, row, case, where, centre, at_row, backward=False, field=True):
    engine, prec, n, rows = row[:4]
    kw = dict(an.STATIC[case]["kw"])
    if backward:
        kw["gamma"] = -kw["gamma"]
    zt, At, _, _ = an.static_truth(case, n, prec, backward)
    off = an.case_oracle_off(case, n, 1)[0] if prec == an.C64 else 0.0
    a = an.shifted(an.static_field(case, n, 1, 0, 0), rows, at_row, centre).astype(CD[prec])
    steps, z, y = r.run(a, kw)
    w.z(where, steps, z, zt, prec, off)
    if field:
        w.field(where, y, an.shifted(At, rows, at_row, centre), field_bound(prec, len(zt) - 1))
    return z


# ----------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_static_peak_positions(row, monkeypatch):
    """The decay case with the pulse centred in turn on every edge sample of the plan's geometry, in every row, the other rows dark: one truth per
    (n, precision) serves all of them.  A maximum that loses a tile, a row, a sub-sequence or counts the padding shows as another step size."""
    w = Worst(f"static {row_id(row)}")
    with runner(row, monkeypatch) as r:
        for at_row in range(row[3]):
            for c in positions(row):
                static_run(r, w, row, "decay", (at_row, c), c, at_row)
    w.close(len(an.static_truth("decay", row[2], row[1])[0]) - 1)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_growing_peak(row, monkeypatch):
    """The growth case, a pulse in the first tile and one in the last: a stale or late maximum gives steps that are too long."""
    w = Worst(f"growth {row_id(row)}")
    with runner(row, monkeypatch) as r:
        for at_row, c in ((0, 5), (row[3] - 1, row[2] - 3)):
            static_run(r, w, row, "growth", (at_row, c), c, at_row)
    w.close(len(an.static_truth("growth", row[2], row[1])[0]) - 1)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_travelling_peak(row, monkeypatch):
    """The travel case: row 0's peak walks through the wrap-around and several tiles, row 1 takes the maximum over part-way (one-row shapes: row 0's pulse
    alone).  z at every step."""
    engine, prec, n, rows = row[:4]
    zt, At, _, _ = an.travel_truth(n, rows, prec)
    off = an.case_oracle_off("travel", n, rows)[0] if prec == an.C64 else 0.0
    a = np.zeros((rows, n), CD[prec])
    a[: min(rows, 2)] = an.travel_field(n, min(rows, 2))
    truth = np.zeros((rows, n), np.complex128)
    truth[: min(rows, 2)] = At
    w = Worst(f"travel {row_id(row)}")
    with runner(row, monkeypatch) as r:
        steps, z, y = r.run(a, an.travel_kw(rows))
    w.z("travel", steps, z, zt, prec, off)
    w.field("travel", y, truth, field_bound(prec, len(zt) - 1))
    w.close(len(zt) - 1)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_backward(row, monkeypatch):
    """gamma < 0 on the decay case, against the restatement of the backward run (not against the forward run): |gamma| in the rule."""
    w = Worst(f"backward {row_id(row)}")
    with runner(row, monkeypatch) as r:
        static_run(r, w, row, "decay", "backward", row[2] // 2 - 1, row[3] - 1, backward=True)
    w.close(len(an.static_truth("decay", row[2], row[1], True)[0]) - 1)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_dark_field(row, monkeypatch):
    """An all-zero field: the rule gives h = inf, clamped to the length -- one step, z = [0, L], the output exactly zero and finite."""
    engine, prec, n, rows = row[:4]
    with runner(row, monkeypatch) as r:
        steps, z, y = r.run(np.zeros((rows, n), CD[prec]), an.DARK_KW)
    assert steps == 1 and list(z) == [0.0, float(RT[prec](an.DARK_KW["length"]))], (steps, z)
    assert np.isfinite(y).all() and not y.any()


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_twice_on_one_plan(row, monkeypatch):
    """The decay case, the growth case and the decay case again on ONE plan: the third z log equals the first bit for bit -- no slot, epoch word or control
    block leaks from one run into the next -- and all three are the rule's."""
    w = Worst(f"twice {row_id(row)}")
    c, at_row = row[2] - 1, row[3] - 1
    with runner(row, monkeypatch) as r:
        z1 = static_run(r, w, row, "decay", "first", c, at_row, field=False)
        static_run(r, w, row, "growth", "second", 7, 0, field=False)
        z3 = static_run(r, w, row, "decay", "third", c, at_row, field=False)
    np.testing.assert_array_equal(z3, z1)
    w.close(len(z1) - 1)
