"""The restatement of the adaptive step rule (tests/adaptive_numpy.py) held to the two statements the suite already trusts, the conditions its four cases
must meet at every size the GPU file (tests/test_adaptive_steps_gpu.py) runs, and the proof that the GPU file's bounds can see a faulty maximum: every
mutant of the maximum is rejected by at least one case at every size class.  No GPU.

A mutant is REJECTED by a case when its step count differs from the truth's, or when some z[k] is at least 100 x the complex64 GPU bound of that k away
(adaptive_numpy.z_bounds with the case's oracle_off).  Which case rejects which mutant (this file's own run; the figure is max_k distance / bound, "steps" a
different step count; the same at n = 256, 1000, 4096, 16384 and 131072 to the digits shown, but for the travel case's drop_subseq):

  mutant        decay, row 1 of 2, sample n-1   decay, sample 0   growth, sample 5   travel, 2 rows    decay backward, sample 0
  row0          steps                           -                 -                  steps             -
  drop_tail     1.3e4                           -                 -                  -                 -
  drop_first    -                               1.3e4             -                  -                 1.3e4
  drop_subseq   1.3e4                           -                 2.3e4              1.9e2 ... 5.6e2   -
  padding       8.9e3                           8.9e3             -                  steps             9.0e3
  running       steps                           steps             -                  steps             steps
  late1         3.5e4                           3.5e4             3.8e4              steps             3.5e4
  late2         steps                           steps             6.3e4              steps             steps
  f16           2.9e2                           2.9e2             1.4e3              2.9e2             2.9e2
  signed_gamma  -                               -                 -                  -                 steps
(C = 16 samples dropped at the tail, the odd samples of R = 2 sub-sequences, a padding value of 0.8 of the input's peak power.  The weakest rejection, f16, is
a z[1] that is 8.6e-5 off against a bound of 3.0e-7.)
The reference's own complex64 run is 0 ... 6.9e-7 from the restatement in z at the powers of two (oracle_off; 1.0e-6 at 65537 and 1.5e-6 at 2049 samples, where its own
single-precision transform of an awkward length moves the maxima), so the complex64 bound on the last z[k] is 2.4e-6 ... 3.1e-6 at the powers of two and 5.9e-6 at its widest."""
import os
import sys

import numpy as np
import pytest

import adaptive_numpy as an
from oracle import ssfm_numpy as orc
from opticomlib_amd.accuracy import TOL_C128

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag"))
import fuzz_cases                                                    # noqa: E402

@pytest.fixture(scope="module", autouse=True)
def _drop_truths():
    yield
    an.clear_caches()


CLASSES = (256, 1000, 4096, 16384, 131072)                            # one size per class: one workgroup, a chirp line, the small engines' limit, the fused / one-XCD engines' ends


def test_restatement_is_the_float64_solution_the_suite_states():
    """complex64 mode: z and the field equal fuzz_cases.truth_adaptive_f64 bit for bit (one and two rows, a static and the travelling case)."""
    for a, kw in ((an.static_field("decay", 1024, 1, 0, 77), an.DECAY["kw"]), (an.static_field("growth", 256, 2, 1, 255), an.GROWTH["kw"]),
                  (an.travel_field(1024, 2), an.travel_kw(2))):
        z, A, where = an.adaptive_truth(a, an.DT, kw, an.C64)
        zt, At = fuzz_cases.truth_adaptive_f64(a, an.DT, kw)
        np.testing.assert_array_equal(z, zt)
        np.testing.assert_array_equal(A, At)
        assert len(where) == len(z)


def test_restatement_in_float64_is_the_float64_twin():
    for a, kw in ((an.static_field("decay", 1024, 1, 0, 77), an.DECAY["kw"]), (an.travel_field(1024, 2), an.travel_kw(2))):
        z, A, _ = an.adaptive_truth(a, an.DT, kw, an.C128)
        ref = orc.fiber_c128(a, an.DT, **kw)
        assert np.max(np.abs(A - ref)) / np.max(np.abs(ref)) <= TOL_C128
        assert abs(z[-1] - kw["length"]) <= 1e-15 and np.all(np.diff(z) > 0)


@pytest.mark.parametrize("case", ["decay", "growth"])
def test_a_dark_background_makes_the_run_equivariant(case):
    """Sample 0 of row 0 against sample n - 1 of row 1: the z logs differ by exactly 0.0 (float32 rule; an ulp of the float64 one), the fields are each other's shift."""
    n, kw = 4096, an.STATIC[case]["kw"]
    for prec in an.BOTH:
        z0, A0, w0 = an.adaptive_truth(an.static_field(case, n, 1, 0, 0), an.DT, kw, prec)
        z1, A1, w1 = an.adaptive_truth(an.static_field(case, n, 2, 1, n - 1), an.DT, kw, prec)
        assert np.max(np.abs(z1 - z0)) <= (0.0 if prec == an.C64 else 2.0 ** -52 * z0[-1]), (prec, z1 - z0)          # (float64 rule: the last bit of the transform shows)
        assert z1[1] == z0[1]
        assert all(w == (1, (s - 1) % n) for w, (_, s) in zip(w1, w0))
        np.testing.assert_array_equal(A1[0], 0)
        assert np.max(np.abs(A1 - an.shifted(A0, 2, 1, n - 1))) <= 1e-13 * np.max(np.abs(A0))


def test_dark_field_is_one_step_of_the_whole_length():
    for prec in an.BOTH:
        z, A, _ = an.adaptive_truth(np.zeros((2, 256), np.complex64), an.DT, an.DARK_KW, prec)
        assert list(z) == [0.0, float(np.float32(an.DARK_KW["length"])) if prec == an.C64 else an.DARK_KW["length"]]
        assert np.isfinite(A).all() and not A.any()


def conditions(case, z, where, info, n, rows):
    h = np.diff(z)
    ratio = h[-1] / info["h_free"][-1]
    assert 0.10 <= ratio <= 0.90, (case, n, rows, ratio)            # a rounding-level difference in the maximum cannot change the step count
    assert len(h) >= 4
    pk = np.array(info["peak"])
    change = pk[1:] / pk[:-1] - 1
    if case == "decay":
        assert np.all(change <= -0.03), change
        assert np.all(np.diff(h[:-1]) > 0)
    if case == "growth":
        assert np.all(change >= 0.03), change
        assert np.all(np.diff(h[:-1]) < 0)
    if case == "travel":
        r0 = [s for r, s in where if r == 0]
        walk = [(b - a) % n for a, b in zip(r0[:-1], r0[1:])]
        assert r0[0] >= n - 64 and any(a > b for a, b in zip(r0[:-1], r0[1:])), where            # the wrap-around
        assert all(10 <= w <= 64 for w in walk) and len({s // 16 for s in r0}) >= 4, where          # tens of samples per step, through several tiles
        if rows >= 2:
            first = next(k for k, (r, _) in enumerate(where) if r == 1)
            assert all(r == 0 for r, _ in where[:first]) and all(r == 1 for r, _ in where[first:]), where
            assert 2 <= first <= len(h) - 2, where                  # the hand-over sets at least one step that is not the clamped one
    return ratio


@pytest.mark.parametrize("n, rows", an.SIZES, ids=[f"{n}x{r}" for n, r in an.SIZES])
def test_the_cases_meet_their_conditions_at_every_size_the_gpu_file_runs(n, rows):
    for case in ("decay", "growth", "travel"):
        for prec in an.BOTH:
            if prec == an.C128 and n > (1 << 17) and (case == "travel" or n < (1 << 21)):
                continue                                             # (complex128 runs of these sizes: only the static cases of the split plan)
            z, A, where, info = an.static_truth(case, n, prec) if case in an.STATIC else an.travel_truth(n, rows, prec)
            ratio = conditions(case, z, where, info, n, rows)
        off, steps = an.case_oracle_off(case, n, rows)
        zt = (an.static_truth(case, n, an.C64) if case in an.STATIC else an.travel_truth(n, rows, an.C64))[0]
        assert steps == len(zt) - 1, (case, n, rows, steps)
        b = an.z_bounds(steps, an.C64, off)
        print(f"{case} {n} x {rows}: {steps} steps, last step {ratio:.3f} of the rule's, oracle_off {off:.2e}, bound {b[0]:.2e} ... {b.max():.2e}")
        assert off <= 2e-6, (case, n, rows, off)                     # (the reference's own transform of an awkward length moves its maxima: 1.5e-6 at 2049 and 65537)


def _rejects(a, kw, mutant, zt, bound, **opt):
    z, _, _ = an.adaptive_truth(a, an.DT, kw, an.C64, mutant=mutant, **opt)
    if len(z) != len(zt):
        return "steps"
    r = float((an.z_distance(z, zt) / bound).max())
    return r if r >= 100 else None


@pytest.mark.parametrize("n", CLASSES)
def test_every_mutant_of_the_maximum_is_rejected_at_every_size_class(n):
    back = dict(an.DECAY["kw"], gamma=-an.DECAY["kw"]["gamma"])
    runs = {"decay r1 n-1": (an.static_field("decay", n, 2, 1, n - 1), an.DECAY["kw"], "decay"), "decay 0": (an.static_field("decay", n, 1, 0, 0), an.DECAY["kw"], "decay"),
            "growth 5": (an.static_field("growth", n, 1, 0, 5), an.GROWTH["kw"], "growth"), "travel": (an.travel_field(n, 2), an.travel_kw(2), "travel"),
            "backward": (an.static_field("decay", n, 1, 0, 0), back, "decay")}
    table = {}
    for name, (a, kw, case) in runs.items():
        zt, _, _ = an.adaptive_truth(a, an.DT, kw, an.C64)
        off, _ = an.case_oracle_off(case, n, 2)
        bound = an.z_bounds(len(zt) - 1, an.C64, off)
        assert _rejects(a, kw, None, zt, bound) is None
        for m in an.MUTANTS:
            table[m, name] = _rejects(a, kw, m, zt, bound, C=16, R=2, r=1)
    for m in an.MUTANTS:
        row = {name: table[m, name] for name in runs if table[m, name] is not None}
        print(f"n={n} {m:13s}", {k: (v if v == 'steps' else f'{v:.1e}') for k, v in row.items()})
        assert row, (n, m)
    # what each case is there for
    assert table["running", "decay 0"] and table["late1", "growth 5"] and table["late2", "growth 5"] and table["row0", "travel"] and table["signed_gamma", "backward"]
    assert table["drop_tail", "decay r1 n-1"] and table["drop_first", "decay 0"] and table["drop_subseq", "decay r1 n-1"] and table["f16", "decay 0"]
