"""tests/sos_numpy.py without a GPU: the long-double reference against the plain serial loop and against the closed form of a constant, SciPy's
float64 sosfiltfilt and the repository's restatement of it under the per-sample bound (serial term alone) on every filter and kind of input
of tests/test_sos_edges_gpu.py, and the comparator against a planted seam fault one order inside what the normwise tolerance lets through."""
import numpy as np
import pytest
import scipy.signal as sg

import sos_numpy as sn
from oracle import filters_numpy as fo

ORDERS = (1, 2, 4, 5, 8)


def design(order, wn):
    sos = sg.bessel(order, wn, "low", norm="mag", output="sos")
    return sos, sg.sosfilt_zi(sos)


@pytest.mark.parametrize("order,wn", [(1, 0.2), (2, 0.3), (4, 0.2), (4, 0.07), (5, 0.07), (8, 0.07), (4, 0.02)])
def test_reference_against_the_serial_loop(order, wn):
    """filtfilt_ref == the long-double sample loop to the reference's floor, on every kind of input; the floor's constant is measured here."""
    sos, zi = design(order, wn)
    R = sn.responses(sos)
    n, worst = 600, 0.0
    for kind in sn.KINDS:
        x = sn.make_input(kind, n, 7, group_len=200)
        ref, ser = sn.filtfilt_ref(sos, zi, x), sn.filtfilt_serial(sos, zi, x)
        _, floor = sn.bound_row(sos, zi, x, parts=True)
        d = np.abs(ref - ser).astype(np.float64)
        unit = floor / sn.F_REF
        r = float(np.max(d / unit))
        worst = max(worst, r)
        print(f"order {order} Wn {wn} {kind}: max |ref - serial| / peak {float(d.max() / np.abs(ser).max()):.1e}, in units of the floor's {r:.2f} (F_REF = {sn.F_REF})")
        assert r <= sn.F_REF, (kind, r)
    assert R.len % 256 == 0


@pytest.mark.parametrize("order,wn", [(1, 0.3), (4, 0.07), (5, 0.02), (8, 0.07), (4, 0.004)])
def test_reference_of_a_constant_is_the_squared_dc_gain(order, wn):
    sos, zi = design(order, wn)
    c = 0.7353
    n = 4 * sn.responses(sos).len
    x = np.full(n, c)
    ref = sn.filtfilt_ref(sos, zi, x)
    want = sn.LD(c) * sn.dc_gain(sos) ** 2
    # two response lengths from either end what the ends ring with is below 1e-26 of the constant: the reference's own floor is all that is left
    # (towards the ends zi, sosfilt_zi's float64 steady state, shows what it misses of the exact one -- the reference takes it as given)
    mid = slice(n // 2 - 8, n // 2 + 8)
    _, floor = sn.bound_row(sos, zi, x, parts=True)
    d = np.abs(ref[mid] - want).astype(np.float64)
    print(f"order {order} Wn {wn}: |ref - c H(1)^2| / c at the middle {float(d.max() / c):.1e}, floor {float(floor[mid].max() / c):.1e}")
    assert np.all(d <= floor[mid])


@pytest.mark.parametrize("wn", sn.WNS)
@pytest.mark.parametrize("order", ORDERS)
def test_scipy_and_the_oracle_keep_the_serial_bound(order, wn):
    """A correct float64 implementation keeps the bound's serial term: SciPy's sosfiltfilt and oracle/filters_numpy.sosfiltfilt, every kind of input."""
    sos, zi = design(order, wn)
    n = 2400
    worst = 0.0
    for kind in sn.KINDS:
        x = sn.make_input(kind, n, 11 + order, pos=1535 - sn.edge_of(sos))
        ref = sn.filtfilt_ref(sos, zi, x)
        b = sn.bound_row(sos, zi, x)
        for name, got in (("scipy", sg.sosfiltfilt(sos, x)), ("oracle", fo.sosfiltfilt(sos, zi, x))):
            r = float(np.max(np.abs(got - ref).astype(np.float64) / b))
            worst = max(worst, r)
            print(f"order {order} Wn {wn} {kind} {name}: worst |d| / bound {r:.4f}; bound / peak {float(b.max() / np.abs(ref).max()):.1e}")
            assert r < 1.0, (kind, name, r)
    assert worst <= sn.R_SCIPY_MAX, worst


@pytest.mark.parametrize("layout", [(1, 12), (4, 18), (1, 18), (4, 12)])
@pytest.mark.parametrize("wn", [0.07, 0.2])
def test_comparator_sees_a_seam_fault_of_1e_12(wn, layout):
    """A start state off by 1e-12 of its magnitude at one group seam of the backward pass -- a tenth of what `within(.., 1e-11)` lets through --
    leaves the bound, and only in the samples just behind that seam; the clean result stays inside."""
    sos, zi = design(4, wn)
    W, L = layout
    group_len = 64 * W * L
    n = 3 * group_len + 40
    x = sn.make_input("walk", n, 5)
    good = sn.filtfilt_ref(sos, zi, x).astype(np.float64)
    worst, _, _ = sn.compare(good, sos, zi, x, layout)
    assert worst < 1.0
    assert sn.compare(sg.sosfiltfilt(sos, x), sos, zi, x, layout)[0] < 1.0
    m = n + 2 * sn.edge_of(sos)
    lead = -(-m // group_len) * group_len - m
    seam = 2 * group_len - lead                       # backward sample at which the device's third group starts
    bad, at = sn.planted_fault(sos, zi, x, seam)
    assert float(np.max(np.abs(bad - good)) / np.max(np.abs(good))) < 1e-11          # (the suite's normwise tolerance sees nothing)
    worst, k, ratio = sn.compare(bad, sos, zi, x, layout)
    out = np.flatnonzero(ratio[0] > 1.0)
    print(f"Wn {wn} layout {layout}: worst ratio {worst:.1f} at output {k}, seam at output {at}; {out.size} samples outside, {out.min()} .. {out.max()}")
    assert worst > 1.0
    assert out.max() <= at and out.min() > at - sn.responses(sos).len // 2          # behind the seam (the backward pass runs towards index 0), nowhere else
    assert at - out.max() < 8                                                          # ... starting right at it
