"""The coherent QAM receiver on the MI355X (csrc/coherent.hip, opticomlib_amd/coherent.py) against the NumPy float64 restatement
tests/coherent_numpy.py: the phase search at every tile seam and limit, its unwrap across tiles, an outlier, exact ties, the mapper and the decisions
at every boundary, and the receiver end to end.  float64 on both sides.  The seeded inputs are those test_coherent_cpu.py holds to a smallest gap
above 1e-6 and a boundary margin above 1e-9 a, so the integers are compared exactly and no symbol is excused; a failure message prints the gap for
the reader, nothing more."""
import numpy as np
import pytest

import coherent_numpy as cn
import margins
import opticomlib_amd as oa
from opticomlib_amd import _lib, coherent
from opticomlib_amd.devices import _stack_rows
from opticomlib_amd.typing import binary_sequence, electrical_signal, gv, optical_signal
from test_coherent_cpu import SEAMS, SEEDED, big_record, seam_record, seeded, staircase_record

pytestmark = pytest.mark.gpu

T = coherent.CPR_TILE
BOUND = 1e-12          # |symbols - restatement| / peak: about ten roundings of 1.1e-16 give under 1e-14; two orders of margin


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no MI355X visible: the gpu-marked tests must run on the GPU box")
    yield
    oa.devices.release_plans()


def run(y, M, B, W, scale):
    """CPR of a host record with explicit scales -> host (symbols, phase, index), each of the record's shape."""
    z, phase, index = coherent.CPR(y, M, B, W, scale=scale)
    assert z.on_device and isinstance(phase, _lib.DeviceArray) and isinstance(index, _lib.DeviceArray) and index.dtype == np.int32
    return np.asarray(z.signal), phase.to_host(), index.to_host()


def same_as_restatement(y, M, B, W, what):
    """One or two rows, each against the restatement of scale * row: index exact, phase within 4 ulp, symbols within BOUND of the peak, bits exact."""
    y = np.asarray(y)
    rows = np.atleast_2d(y)
    scale = np.array([cn.scale_of(r.astype(np.complex128)) for r in rows])
    z, phase, index = (np.atleast_2d(a) for a in run(y, M, B, W, scale))
    for r, row in enumerate(rows):
        want = cn.bps(row.astype(np.complex128) * scale[r], M, B, W)
        bad = np.nonzero(index[r] != want["index"])[0]
        assert bad.size == 0, (what, r, "index differs at", bad[:8].tolist(), "gap there", want["gap"][bad[:8]].tolist())
        assert np.all(np.abs(phase[r] - want["phase"]) <= 4 * np.spacing(np.abs(want["phase"]))), (what, r, "phase")
        assert margins.within(z[r], want["symbols"], BOUND, what=f"cpr {what} row {r}"), (what, r, margins.relmax(z[r], want["symbols"]))
        bits = coherent.QAM_DECODER(z[r], M)
        assert isinstance(bits._raw(), _lib.DeviceArray)
        np.testing.assert_array_equal(bits.data, cn.decode(want["symbols"], M), err_msg=f"{what} row {r}")
    return index


# ------------------------------------------------------------------------------------------------ kernel against the restatement
def test_the_seeded_records_equal_the_restatement():
    for name in SEEDED:
        y, s, bits, M, B, W = seeded(name)
        same_as_restatement(y, M, B, W, name)


def test_every_tile_seam_and_limit_in_both_types():
    for i, (n, M, B, W) in enumerate(SEAMS):
        for dtype in (np.complex128, np.complex64):
            same_as_restatement(seam_record(n, M, i, dtype), M, B, W, f"n={n} M={M} B={B} W={W} {dtype.__name__}")


def test_two_rows_with_different_content_are_independent():
    for (n, M, B, W), dtype in (((2 * T + 32 + 1, 64, 32, 32), np.complex128), ((T + 1, 16, 32, 32), np.complex64)):
        y = np.stack([seam_record(n, M, 50, dtype), 0.3 * seam_record(n, M, 51, dtype)])
        two = same_as_restatement(y, M, B, W, f"two rows n={n} {dtype.__name__}")
        one = same_as_restatement(y[1], M, B, W, "the second row alone")
        np.testing.assert_array_equal(two[1], one[0])


def test_the_strided_read_with_an_offset_a_remainder_and_a_wide_pitch():
    """The kernel's own load: symbol k of row r is scale[r] x[r pitch + start + k step]."""
    n, M, B, W, start, step = T + 7, 16, 32, 32, 3, 5
    pitch = start + n * step + 11                               # the last symbol is not the row's last sample, and the step leaves a remainder
    rng = np.random.default_rng(9)
    for dtype in (np.complex128, np.complex64):
        field = (rng.standard_normal((2, pitch)) + 1j * rng.standard_normal((2, pitch))).astype(dtype)
        rows = [seam_record(n, M, 60 + r, dtype) for r in range(2)]
        for r in range(2):
            field[r, start:start + n * step:step] = rows[r]
        x = _lib.DeviceArray.from_host(field, None, 0)
        power = coherent._row_power(x, 2, n, start, step, pitch)
        want_power = [float(np.mean(np.abs(r.astype(np.complex128)) ** 2)) for r in rows]
        np.testing.assert_allclose(power, want_power, rtol=1e-13)
        scale = np.array([cn.scale_of(r.astype(np.complex128)) for r in rows])
        index, phase, z = coherent._search(x, 2, n, start, step, pitch, scale, M, B, W, 0)
        index, z = index.to_host(), z.to_host()
        for r in range(2):
            want = cn.bps(rows[r].astype(np.complex128) * scale[r], M, B, W)
            np.testing.assert_array_equal(index[r], want["index"], err_msg=f"{dtype.__name__} row {r}")
            assert margins.within(z[r], want["symbols"], BOUND, what=f"strided {dtype.__name__} row {r}")
    with pytest.raises(ValueError):
        coherent._search(x, 2, n, start, step, start + (n - 1) * step, scale, M, B, W, 0)      # the last symbol would lie in the next row


def test_sector_crossings_on_tile_seams_carry_the_turns_across_tiles():
    y, c, B = staircase_record()
    jumps = np.nonzero(np.diff(c // B))[0] + 1
    assert T - 1 in jumps and 2 * T in jumps and 3 * T in jumps          # the last symbol of a tile, the first of the next, and one back down
    z, phase, index = run(y, 4, B, 0, [1.0])
    np.testing.assert_array_equal(index, c)
    np.testing.assert_array_equal(index, cn.bps(y, 4, B, 0)["index"])
    np.testing.assert_array_equal(phase, (c - B // 2) * cn.phase_step(B))


def test_65536_symbols_in_two_rows():
    y, c, M, B, W = big_record()
    index = same_as_restatement(y, M, B, W, "2^16 x 2")
    assert index[0, -1] - index[0, 0] > 30 * B and index[1, 0] - index[1, -1] > 30 * B       # dozens of turns, carried over 256 tiles


# ------------------------------------------------------------------------------------------------ outlier, ties, determinism
def test_one_outlier_leaves_no_trace_outside_its_window():
    y, s, bits, M, B, W = seeded("qam16")
    y = y * cn.scale_of(y)
    k0 = y.size // 2
    hit = y.copy()
    hit[k0] = 1e8 * np.exp(0.3j)
    clean, dirty = run(y, M, B, W, [1.0])[2], run(hit, M, B, W, [1.0])[2]
    outside = np.abs(np.arange(y.size) - k0) > W
    np.testing.assert_array_equal(dirty[outside] % B, clean[outside] % B)
    assert np.any(dirty[~outside] % B != clean[~outside] % B)                      # (it was seen inside)


def test_exact_ties_take_the_first_phase():
    n, M, B, W = T + 5, 16, 8, 4
    z, phase, index = coherent.CPR(np.zeros(n, complex), M, B, W, normalize=False)
    assert not np.any(index.to_host()) and not np.any(np.asarray(z.signal)) and np.all(phase.to_host() == (0 - B // 2) * cn.phase_step(B))
    with pytest.raises(ValueError, match="zero power"):
        coherent.CPR(np.zeros(n, complex), M, B, W)
    y = seam_record(n, M, 70)
    y = y * cn.scale_of(y)
    k0 = T - 2                                                   # the silent window straddles the seam
    y[k0 - W:k0 + W + 1] = 0
    z, phase, index = run(y, M, B, W, [1.0])
    want = cn.bps(y, M, B, W)
    assert want["bhat"][k0] == 0 and index[k0] % B == 0
    np.testing.assert_array_equal(index, want["index"])
    assert not np.any(z[k0 - W:k0 + W + 1])


def test_two_runs_give_equal_bytes():
    y, s, bits, M, B, W = seeded("qam64")
    a, b = run(y, M, B, W, [0.9]), run(y, M, B, W, [0.9])
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


# ------------------------------------------------------------------------------------------------ mapper and decisions
def test_the_mapper_is_bit_equal_from_host_bits_and_from_device_bits():
    for M in cn.ORDERS:
        k = cn.bits_per_symbol(M)
        seq = oa.PRBS(15, len=k * (2 * T + 3))
        assert seq.on_device
        sym = coherent.QAM_ENCODER(seq, M)
        assert sym.on_device and sym._raw("signal").dtype == np.complex128
        bits = seq.data
        np.testing.assert_array_equal(sym.signal, cn.encode(bits, M))
        np.testing.assert_array_equal(coherent.QAM_ENCODER(bits, M).signal, cn.encode(bits, M))
        np.testing.assert_array_equal(coherent.QAM_DECODER(sym, M).data, bits)
    b = np.random.default_rng(1).integers(0, 2, (300, 2))
    np.testing.assert_array_equal(coherent.QAM_ENCODER(b.ravel(), 4).signal, ((2 * b[:, 0] - 1) + 1j * (2 * b[:, 1] - 1)) / np.sqrt(2))


def test_decisions_on_just_below_and_just_above_every_boundary():
    for M in cn.ORDERS:
        L, a, k = cn.side(M), cn.half_spacing(M), cn.bits_per_symbol(M)
        xs, levels = [0.0, -0.0, -9.0, 9.0, -1e300, 1e300], [L // 2, L // 2, 0, L - 1, 0, L - 1]
        for m in range(-(L // 2 - 1), L // 2):
            x = 2 * a * m
            xs += [x, x + 1e-9 * a, x - 1e-9 * a, np.nextafter(x, 10.0), np.nextafter(x, -10.0)]
            levels += [m + L // 2, m + L // 2, m + L // 2 - 1, None, None]               # an ulp beside: the rule's own float64 expression decides
        xs = np.array(xs)
        want = cn.level(xs, M)
        assert all(w is None or w == g for w, g in zip(levels, want))
        for re, im in ((xs, xs[::-1]), (xs[::-1], xs)):
            z = np.empty(xs.size, complex)
            z.real, z.imag = re, im                                                  # (assigned: -0.0 stays -0.0)
            got = coherent.QAM_DECODER(z, M).data.reshape(-1, k)
            np.testing.assert_array_equal(got.ravel(), cn.decode(z, M), err_msg=str(M))
            np.testing.assert_array_equal(cn.gray_decode(cn._to_int(got[:, : k // 2])), cn.level(z.real, M))


# ------------------------------------------------------------------------------------------------ the receiver, end to end
def transmitter(M, nsym, seed, lw=1e5):
    bits = oa.PRBS(7, len=nsym * cn.bits_per_symbol(M), seed=seed)
    sym = coherent.QAM_ENCODER(bits, M)
    return bits, sym, oa.LASER(0.0, lw=lw, rng="device") * coherent.SHAPE(sym, "rcos", beta=0.3)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("rows", [1, 2])
def test_back_to_back_link_has_no_bit_errors_and_moves_nothing_to_the_host(M, rows):
    nsym, sps = 2 * T + 9, 8
    gv(sps=sps, R=10e9, N=nsym)
    oa.device_rng_seed(5)
    before = dict(_lib.TRANSFERS)
    tx = [transmitter(M, nsym, 3 + r) for r in range(rows)]
    field = tx[0][2] if rows == 1 else optical_signal.from_device(_stack_rows([t[2]._raw("signal") for t in tx], np.complex128, 0, (2, nsym * sps)))
    assert field.on_device and field.shape == ((nsym * sps,) if rows == 1 else (2, nsym * sps))
    ref = tx[0][1] if rows == 1 else (tx[0][1], tx[1][0])                          # symbols for one row, bits for the other
    rx = coherent.DSP(field, M, ref=ref)
    assert _lib.TRANSFERS["d2h"] == before["d2h"]                                  # nothing came back: bits -> field -> bits stayed in GPU memory
    pick = (lambda v, r: v) if rows == 1 else (lambda v, r: v[r])
    host = np.atleast_2d(field.signal)
    assert _lib.TRANSFERS["d2h"] > before["d2h"]
    for r in range(rows):
        bits, sym, _ = tx[r]
        assert pick(rx.bits, r).on_device and pick(rx.symbols, r).on_device
        assert coherent.BER(bits, pick(rx.bits, r)) == 0.0
        assert pick(rx.quarter_turns, r) in (0, 1, 2, 3)
        want = cn.receive(host[r], sps, M, 32, 32, ref=np.asarray(sym.signal))
        assert abs(pick(rx.evm, r) - want["evm"]) <= 1e-9, (pick(rx.evm, r), want["evm"])
        assert pick(rx.quarter_turns, r) == want["quarter_turns"]
        assert abs(coherent.EVM(pick(rx.symbols, r), ref=sym) - pick(rx.evm, r)) <= 1e-15
    blind = coherent.DSP(field, M)                                                 # without ref the ambiguity remains and is said so
    assert pick(blind.quarter_turns, 0) is None and pick(blind.evm, 0) < 0.2


def test_through_fiber_and_dbp_the_receiver_is_the_restatement_of_the_downloaded_field():
    M, sps, nsym = 16, 8, 512
    gv(sps=sps, R=32e9, N=nsym)
    oa.device_rng_seed(6)
    tx = [transmitter(M, nsym, 21 + r, lw=2e5) for r in range(2)]
    field = optical_signal.from_device(_stack_rows([t[2]._raw("signal") for t in tx], np.complex128, 0, (2, nsym * sps)))
    fibre = dict(length=3.0, h=1.0, alpha=0.2, beta_2=-21.7, beta_3=0.13, gamma=1.3)
    back = oa.DBP(oa.FIBER(field, coupling="manakov", **fibre), coupling="manakov", **fibre)
    assert back.on_device and back.shape == (2, 1 << 12)
    rx = coherent.DSP(back, M, test_phases=32, window=32, ref=(tx[0][1], tx[1][1]))
    host = np.asarray(back.signal)
    for r in range(2):
        want = cn.receive(host[r], sps, M, 32, 32, ref=np.asarray(tx[r][1].signal))
        gap = float(want["gap"].min())
        np.testing.assert_array_equal(rx.bits[r].data, want["bits"], err_msg=f"row {r}, smallest gap {gap:.2e}")
        assert rx.quarter_turns[r] == want["quarter_turns"]
        assert margins.within(np.asarray(rx.symbols[r].signal), want["symbols"], BOUND, what=f"dsp after fiber + dbp, row {r}"), gap
        np.testing.assert_allclose(rx.phase[r].to_host(), want["phase"], rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ residency and refusals
def test_a_host_record_is_uploaded_once_and_a_record_on_another_gpu_is_refused():
    y, s, bits, M, B, W = seeded("qpsk")
    before = dict(_lib.TRANSFERS)
    z, phase, index = coherent.CPR(y, M, B, W)
    assert _lib.TRANSFERS["h2d"] == before["h2d"] + 1 and _lib.TRANSFERS["d2h"] == before["d2h"]
    assert z.on_device and z.execution_time > 0
    on = electrical_signal.from_device(_lib.DeviceArray.from_host(y, None, 0))
    before = dict(_lib.TRANSFERS)
    z2, _, index2 = coherent.CPR(on, M, B, W)
    assert _lib.TRANSFERS == before
    np.testing.assert_array_equal(index2.to_host(), index.to_host())
    for call in (lambda: coherent.CPR(on, M, B, W, device=1), lambda: coherent.QAM_DECODER(on, M, device=1), lambda: coherent.EVM(on, M=M, device=1),
                 lambda: coherent.DSP(optical_signal.from_device(on._raw("signal")), M, device=1)):
        with pytest.raises(ValueError, match="lies on GPU 0, not on GPU 1"):
            call()
    dev_bits = binary_sequence.from_device(_lib.DeviceArray.from_host(bits, np.uint8, 0))
    assert coherent.BER(dev_bits, coherent.QAM_DECODER(coherent.QAM_ENCODER(dev_bits, M), M)) == 0.0
