"""The zero-phase SOS filter (csrc/sos_filter.hip, sos_filter_impl.inc) held sample by sample to the bound of tests/sos_numpy.py against its
long-double reference, on every route of the dispatcher -- each case pins the knobs it depends on, deletes the others, and asserts with
_lib.sosfiltfilt_last_route() that the route it is about really ran.

A. every route x sections 1..4 x real / complex, at lengths on both sides of a group seam, and the sizes at which the code takes another path
   (the third table level of the three-launch form, the look-back's limit on groups per row, the one-wavefront long-chunk route at its
   natural size); a last test names the cells of the table that no case reported.
B. inputs on which a seam error shows (sos_numpy.KINDS) at Wn in {0.3, 0.07, 0.02, 0.004}.
C. rows: a zero row between two of magnitude 1e6 stays exactly zero; rows equal the same rows filtered alone, bit for bit.
D. state between calls: filters, lengths, shapes and buffers alternated in one process; in place on the device; a call after one that gave up.

Every comparison records the device's worst |d| / bound and, beside it, SciPy's float64 result against the serial term alone, through
tests/margins.py (digest: profiles/sos_margins.txt)."""
import numpy as np
import pytest
import scipy.signal as sg

import margins
import sos_numpy as sn
import opticomlib_amd as oa
from opticomlib_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("SSFM_SOS_ONE_LAUNCH", "SSFM_SOS_NEAR", "SSFM_SOS_MEET", "SSFM_SOS_LONG_CHUNK", "SSFM_SOS_PATIENCE_US", "SOS_WAVES_FORCE")
ORDER_OF = {(1, False): 1, (1, True): 2, (2, False): 4, (2, True): 4, (3, False): 5, (3, True): 6, (4, False): 8, (4, True): 8}
SEEN = set()            # (cell of the routes table as REPORTED, sections, complex)


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def pin(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# route of the table -> (knobs, what the accessor must report, (wavefronts, chunk) its sizes are laid out for)
ROUTES = {
    "three launches W=1": (dict(SOS_WAVES_FORCE="1", SSFM_SOS_ONE_LAUNCH="0"), dict(waves=1, chunk=12, launches=3), (1, 12)),
    "three launches W=4": (dict(SOS_WAVES_FORCE="4", SSFM_SOS_ONE_LAUNCH="0"), dict(waves=4, chunk=12, launches=3), (4, 12)),
    "one launch W=1 chunk 12": (dict(), dict(waves=1, chunk=12, launches=1, meet=False), (1, 12)),
    "one launch W=4 chunk 18": (dict(SOS_WAVES_FORCE="4"), dict(waves=4, chunk=18, launches=1, meet=False), (4, 18)),
    "one launch W=4 chunk 12": (dict(SOS_WAVES_FORCE="4", SSFM_SOS_LONG_CHUNK="0"), dict(waves=4, chunk=12, launches=1, meet=False), (4, 12)),
    "near look-back": (dict(), dict(launches=1, tagged=True, meet=False), (1, 12)),
    "all-totals look-back": (dict(SSFM_SOS_NEAR="0"), dict(launches=1, look=0, meet=False), (1, 12)),
    "single meeting": (dict(SSFM_SOS_MEET="1"), dict(launches=1, tagged=True, meet=True), (1, 12)),
}
TAGGED_ONLY = ("near look-back", "single meeting")          # cells with CH * K <= 8 only
NATURAL = "one launch W=1 chunk 18"


def cells_of(route):
    if route["launches"] == 3:
        return {f"three launches W={route['waves']}"}
    if route["meet"]:
        return {"single meeting"}
    return {f"one launch W={route['waves']} chunk {route['chunk']}", "near look-back" if route["look"] > 0 else "all-totals look-back"}


def expected_cells():
    out = set()
    for name in ROUTES:
        for ns in (1, 2, 3, 4):
            for cplx in (False, True):
                if name in TAGGED_ONLY and (2 if cplx else 1) * 2 * ns > 8:
                    continue
                out.add((name, ns, cplx))
    out.add((NATURAL, 2, True))
    return out


def design(order, wn):
    sos = sg.bessel(order, wn, "low", norm="mag", output="sos")
    return sos, sg.sosfilt_zi(sos)


def judge(got, sos, zi, x, route, what):
    """The device's result against the long-double reference under the bound of the layout that ran; SciPy's beside it under the serial term."""
    ns, cplx = sos.shape[0], np.iscomplexobj(x)
    assert route["sections"] == ns and route["channels"] == (2 if cplx else 1), route
    SEEN.update((c, ns, bool(cplx)) for c in cells_of(route))
    worst, k, _ = sn.compare(got, sos, zi, x, (route["waves"], route["chunk"]))
    scipy_r = sn.compare(sg.sosfiltfilt(sos, x, axis=-1), sos, zi, x)[0]
    dom = "complex" if cplx else "real"
    print(f"{what} {dom} n={x.shape[-1]}: route {route}; device worst |d| / bound {worst:.4f} at {k}; SciPy / serial term {scipy_r:.4f}")
    margins.record(f"{what} {dom} n={x.shape[-1]} scipy / long double [|d| / serial term]", None, scipy_r, 1.0)
    assert scipy_r < 1.0
    return margins.within(None, None, 1.0, what=f"{what} {dom} n={x.shape[-1]} device / long double [|d| / bound]", measured=worst)


def walk(rows, n, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n)).cumsum(axis=-1) * 0.05 + rng.standard_normal((rows, n))
    if cplx:
        x = x + 1j * (rng.standard_normal((rows, n)).cumsum(axis=-1) * 0.05 + rng.standard_normal((rows, n)))
    return x[0] if rows == 1 else x


def expect_route(route, expect):
    for k, v in expect.items():
        assert route[k] == v, (k, route, expect)


# ----------------------------------------------------------------------------------------------- A. routes
def route_cell(monkeypatch, name, ns, cplx):
    env, expect, (W, L) = ROUTES[name]
    wn = 0.02 if name == "near look-back" and ns <= 2 else 0.07          # (a look-back of two or three groups where the filter has one)
    sos, zi = design(ORDER_OF[(ns, cplx)], wn)
    assert sos.shape[0] == ns
    pin(monkeypatch, **env)
    group, edge = 64 * W * L, sn.edge_of(sos)
    groups = 4 if name == "near look-back" else 2
    for n in (groups * group - 2 * edge, groups * group - 2 * edge + 1):          # the padded row ends with a group, and one sample into the next
        x = walk(1, n, cplx, n + ns)
        got = _lib.sosfiltfilt(sos, zi, x)
        route = _lib.sosfiltfilt_last_route()
        expect_route(route, expect)
        if name == "near look-back":
            assert route["look"] >= 1
        assert judge(got, sos, zi, x, route, f"route {name} sections {ns} look {route['look']}")


@pytest.mark.parametrize("name,ns,cplx", sorted(c for c in expected_cells() if c[0] != NATURAL),
                         ids=lambda v: ("complex" if v else "real") if isinstance(v, bool) else str(v))
def test_every_route_under_the_per_sample_bound(name, ns, cplx, monkeypatch):
    route_cell(monkeypatch, name, ns, cplx)


def test_one_wavefront_long_chunk_at_its_natural_size(monkeypatch):
    """Not forceable: the dispatcher takes one wavefront with chunk 18 where the short chunk's grid is not resident and the long one's is."""
    sos, zi = design(4, 0.07)
    pin(monkeypatch)
    tried = []
    for n in (1500003, 1600003, 1700003, 1800003, 1950003, 2100003):
        x = walk(1, n, True, n)
        got = _lib.sosfiltfilt(sos, zi, x)
        route = _lib.sosfiltfilt_last_route()
        tried.append((n, route["waves"], route["chunk"], route["launches"]))
        if (route["waves"], route["chunk"], route["launches"]) == (1, 18, 1):
            print(f"one wavefront, chunk 18: first at n = {n} of {tried}")
            assert judge(got, sos, zi, x, route, f"route {NATURAL} sections 2 look {route['look']}")
            return
    pytest.fail(f"no length took one wavefront with the long chunk: {tried}")


@pytest.mark.parametrize("what,order,cplx,n,env,expect", [
    # more than 64 groups: the three-launch form's third table level
    ("third level W=1", 4, False, 49152 + 1500, dict(SOS_WAVES_FORCE="1", SSFM_SOS_ONE_LAUNCH="0"), dict(waves=1, chunk=12, launches=3)),
    ("third level W=4", 4, True, 196608 + 1500, dict(SOS_WAVES_FORCE="4", SSFM_SOS_ONE_LAUNCH="0"), dict(waves=4, chunk=12, launches=3)),
    # kLookIter x kGroup = 128 groups of one wavefront: at the limit with every total; past it only the near look-back stays in one wavefront
    ("128 groups flagged", 8, True, 98304 - 2 * 27 - 5, dict(), dict(waves=1, chunk=12, launches=1, look=0, tagged=False)),
    ("129 groups flagged", 8, True, 98304 - 2 * 27 + 5, dict(), dict(look=0, tagged=False)),
    ("128 groups tagged, every total", 4, False, 98304 - 2 * 15 - 5, dict(SSFM_SOS_NEAR="0"), dict(waves=1, chunk=12, launches=1, look=0, tagged=True)),
    ("129 groups tagged, every total", 4, False, 98304 - 2 * 15 + 5, dict(SSFM_SOS_NEAR="0"), dict(look=0)),
    ("129 groups near", 4, True, 98304 - 2 * 15 + 5, dict(), dict(waves=1, chunk=12, launches=1, look=1, tagged=True)),
])
def test_sizes_at_which_the_code_takes_another_path(what, order, cplx, n, env, expect, monkeypatch):
    sos, zi = design(order, 0.07)
    pin(monkeypatch, **env)
    x = walk(1, n, cplx, n)
    got = _lib.sosfiltfilt(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    expect_route(route, expect)
    if what.startswith("129 groups") and "near" not in what:          # past the limit without the near look-back: not one wavefront in one launch
        assert (route["waves"], route["launches"]) != (1, 1), route
    assert judge(got, sos, zi, x, route, f"size {what}")


# ----------------------------------------------------------------------------------------------- B. inputs on which a seam error shows
@pytest.mark.parametrize("layout", [(1, 12), (4, 18)], ids=["W1c12", "W4c18"])
@pytest.mark.parametrize("wn", sn.WNS)
@pytest.mark.parametrize("kind", sn.KINDS)
def test_inputs_on_which_a_seam_error_shows(kind, wn, layout, monkeypatch):
    W, L = layout
    sos, zi = design(4, wn)
    pin(monkeypatch, **({} if W == 1 else dict(SOS_WAVES_FORCE="4")))
    group, edge = 64 * W * L, sn.edge_of(sos)
    n = 3 * group + 40 - 2 * edge
    if kind == "impulse":          # on the last sample of a chunk, of a wavefront's 64 chunks, of a group, and on the first sample of the next
        pads = (group + 5 * L - 1, group + 64 * L - 1, 2 * group - 1, 2 * group)
        x = np.stack([sn.make_input(kind, n, 0, pos=p - edge) for p in pads])
    else:
        x = sn.make_input(kind, n, 17, group_len=group)
    got = _lib.sosfiltfilt(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    expect_route(route, dict(waves=W, chunk=L, launches=1, meet=False))
    assert judge(got, sos, zi, x, route, f"input {kind} Wn={wn} layout {W}x{L} look {route['look']}")


@pytest.mark.parametrize("kind", ["walk", "const", "big"])
def test_single_meeting_two_groups_deep(kind, monkeypatch):
    """The single-meeting kernel where the look-back is two groups (its `deep` branch): order 2 at Wn = 0.02."""
    sos, zi = design(2, 0.02)
    pin(monkeypatch, SSFM_SOS_MEET="1")
    n = 5 * 768 + 40
    x = sn.make_input(kind, n, 23)
    got = _lib.sosfiltfilt(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    expect_route(route, dict(waves=1, chunk=12, launches=1, meet=True, look=2))
    assert judge(got, sos, zi, x, route, f"input {kind} Wn=0.02 single meeting look 2")


# ----------------------------------------------------------------------------------------------- C. rows
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(ROUTES))
def test_rows_do_not_touch_each_other(name, cplx, monkeypatch):
    """A zero row between two of magnitude 1e6 stays exactly zero, and every row equals the same row filtered alone, bit for bit."""
    env, expect, (W, L) = ROUTES[name]
    sos, zi = design(4, 0.07)
    pin(monkeypatch, **env)
    n = 2 * 64 * W * L + 100          # three groups per row
    x = 1e6 * walk(3, n, cplx, 31)
    x[1] = 0
    got = _lib.sosfiltfilt(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    expect_route(route, expect)
    assert not got[1].any(), np.abs(got[1]).max()
    assert judge(got, sos, zi, x, route, f"rows {name}")
    for i in range(3):
        alone = _lib.sosfiltfilt(sos, zi, x[i])
        r1 = _lib.sosfiltfilt_last_route()
        assert r1 == route, (r1, route)
        assert np.array_equal(got[i], alone), (i, np.abs(got[i] - alone).max())


# ----------------------------------------------------------------------------------------------- D. state between calls
def _device_call(sos, zi, x, in_place=False):
    xd = _lib.DeviceArray.from_host(np.ascontiguousarray(x))
    yd = xd if in_place else _lib.DeviceArray(x.shape, x.dtype)
    try:
        _lib.sosfiltfilt_device(sos, zi, xd.ptr, yd.ptr, x.shape[-1], x.size // x.shape[-1], np.iscomplexobj(x))
        return yd.to_host(), xd.to_host()
    finally:
        xd.free()
        if not in_place:
            yd.free()


def test_filters_lengths_shapes_and_buffers_alternated(monkeypatch):
    """Two filters of one order, a third of another, two lengths, both forced shapes, the single-meeting kernel (its maps depend on where the
    row ends), host and device buffers: every call gives the bits it gave in the other order (table_key, meet_key, the tagged-totals buffer growing, the call tag)."""
    filters = [design(4, 0.07), design(4, 0.2), design(5, 0.07)]
    lengths = (1600, 9301)
    xs = {n: walk(2, n, True, n) for n in lengths}
    configs = [(f, n, env, dev) for f in range(3) for n in lengths
               for env in (dict(SOS_WAVES_FORCE="1"), dict(SOS_WAVES_FORCE="4"), dict(SOS_WAVES_FORCE="1", SSFM_SOS_MEET="1"))
               for dev in (False, True)]

    def call(cfg):
        f, n, env, dev = cfg
        pin(monkeypatch, **env)
        sos, zi = filters[f]
        y = _device_call(sos, zi, xs[n])[0] if dev else _lib.sosfiltfilt(sos, zi, xs[n])
        route = _lib.sosfiltfilt_last_route()
        assert route["waves"] == int(env["SOS_WAVES_FORCE"]) and route["launches"] == 1, (cfg, route)
        assert route["meet"] == ("SSFM_SOS_MEET" in env and filters[f][0].shape[0] == 2), (cfg, route)
        return y

    first = {i: call(c) for i, c in enumerate(configs)}                      # filter by filter, length by length
    order = np.random.default_rng(3).permutation(len(configs))
    for rnd in range(2):
        for i in (order if rnd == 0 else order[::-1]):
            assert np.array_equal(call(configs[i]), first[i]), configs[i]
    for i, c in enumerate(configs):                                          # ... and the bits are right ones
        if not c[3] and "SSFM_SOS_MEET" not in c[2]:
            sos, zi = filters[c[0]]
            assert sn.compare(first[i], sos, zi, xs[c[1]], (int(c[2]["SOS_WAVES_FORCE"]), 12 if c[2]["SOS_WAVES_FORCE"] == "1" else 18))[0] <= 1.0


@pytest.mark.parametrize("name", [k for k in ROUTES if not k.startswith("three")])
def test_in_place_on_the_device(name, monkeypatch):
    """Every one-launch route writes an in-place call's result to scratch first (`overlap`): same bits as out of place."""
    env, expect, (W, L) = ROUTES[name]
    sos, zi = design(4, 0.07)
    pin(monkeypatch, **env)
    x = walk(2, 2 * 64 * W * L + 77, True, 41)
    want, kept = _device_call(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    expect_route(route, expect)
    assert np.array_equal(kept, x)
    got, _ = _device_call(sos, zi, x, in_place=True)
    assert _lib.sosfiltfilt_last_route() == route
    assert np.array_equal(got, want)
    assert judge(got, sos, zi, x, route, f"in place {name}")


def test_recovery_after_giving_up(monkeypatch):
    """Two calls with a patience of 1 us (either form may run; the result is right and the input untouched), then one with the default
    patience, which takes one launch again."""
    sos, zi = design(4, 0.1)
    n = 1 << 17
    x = walk(2, n, True, 11)
    pin(monkeypatch)
    _lib.sosfiltfilt(sos, zi, x)
    assert _lib.sosfiltfilt_last_launches() == 1
    monkeypatch.setenv("SSFM_SOS_PATIENCE_US", "1")
    for i in range(2):
        got, kept = _device_call(sos, zi, x, in_place=False)
        route = _lib.sosfiltfilt_last_route()
        assert route["launches"] in (1, 3)
        assert np.array_equal(kept, x)
        assert judge(got, sos, zi, x, route, f"patience 1 us call {i} launches {route['launches']}")
    monkeypatch.delenv("SSFM_SOS_PATIENCE_US")
    got = _lib.sosfiltfilt(sos, zi, x)
    route = _lib.sosfiltfilt_last_route()
    assert route["launches"] == 1, route
    assert judge(got, sos, zi, x, route, "after giving up")


# ----------------------------------------------------------------------------------------------- the table's cells
def test_every_cell_of_the_routes_table_was_seen(monkeypatch):
    """By route AS REPORTED.  (Run alone, this test first runs the cells nobody has reported yet.)"""
    for name, ns, cplx in sorted(expected_cells() - SEEN):
        if name == NATURAL:
            test_one_wavefront_long_chunk_at_its_natural_size(monkeypatch)
        else:
            route_cell(monkeypatch, name, ns, cplx)
    missing = sorted(expected_cells() - SEEN)
    assert not missing, f"cells of the routes table that no call reported: {missing}"
