"""The coherent QAM receiver without a GPU: the NumPy restatement tests/coherent_numpy.py held to the model's own properties (constellation, Gray
code, jump rule, window truncation, noise-free recovery), the seeded cases of the GPU suite held to the two conditions under which integers of two
float64 implementations may be compared exactly, csrc/coherent_tiles.hpp held to brute force in a host program of its own under AddressSanitizer
and UBSan (tests/coherent_host.cpp), and the module's ABI and argument checks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import coherent_numpy as cn
import opticomlib_amd as oa
from opticomlib_amd import _lib, coherent
from opticomlib_amd.typing import gv, optical_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")
NEW_SYMBOLS = ("ssfm_qam_encode", "ssfm_qam_decide", "ssfm_qam_sums", "ssfm_cpr_power", "ssfm_cpr_search")
MIN_GAP, MIN_MARGIN = 1e-6, 1e-9           # above these an exact comparison of integers is fair; asserted here for every seeded case

# The seeded records of the GPU suite: name -> (n, M, SNR [dB], B, W, seed); every one has Wiener phase noise and a 3 rad ramp.
T = coherent.CPR_TILE
SEEDED = {
    "qpsk": (1500, 4, 15, 32, 16, 11),
    "qam16": (1500, 16, 22, 32, 32, 12),
    "qam64": (1500, 64, 28, 64, 32, 13),
}
# n at the tile seams x the limits of W and B x every M: not a full product, every value at a seam at least once
SEAMS = [(1, 4, 2, 0), (2, 16, 4, 1), (32, 64, 32, 32), (33, 256, 64, 32), (65, 4, 32, 32), (T - 1, 16, 64, 0), (T, 64, 2, 1), (T + 1, 256, 4, 32),
         (T + 32, 4, 32, 32), (T + 256, 16, 64, 256), (2 * T + 32 + 1, 64, 32, 32), (2 * T + 256 + 1, 256, 2, 256), (3 * T + 5, 16, 4, 256), (3 * T + 5, 64, 32, 1),
         (256, 4, 64, 256), (257, 16, 32, 256), (513, 256, 32, 256)]
SNR = {4: 15.0, 16: 22.0, 64: 28.0, 256: 34.0}


def seeded(name):
    n, M, snr, B, W, seed = SEEDED[name]
    y, s, bits, theta = cn.noisy_record(n, M, snr, seed)
    return y, s, bits, M, B, W


def seam_record(n, M, seed, dtype=np.complex128):
    """The record of a seam case: the values both sides read (rounded to `dtype` first)."""
    y = cn.noisy_record(n, M, SNR[M], 1000 + seed)[0].astype(dtype)
    return y


def _on_staircase(c, M, B, seed):
    """Noise-free random symbols turned by theta_k = (c_k - B / 2 + 0.2) pi / (2 B): a fifth of a step beside test phase c_k mod B."""
    s = cn.encode(np.random.default_rng(seed).integers(0, 2, c.size * cn.bits_per_symbol(M)).astype(np.uint8), M)
    return s * np.exp(1j * ((c - B / 2 + 0.2) * cn.phase_step(B)))


def staircase_record():
    """A QPSK record for W = 0 whose chosen phase is c_k mod B exactly, with sector crossings on the last symbol of tile 0 (upwards), on the first symbol
    of tile 2 (upwards) and on the first symbol of tile 3 (back down): (y, c, B); u_k = c_k."""
    B, n = 32, 3 * T + 5
    k = np.arange(n)
    c = np.where(k < T - 1, B - 1, np.where(k < 2 * T, np.minimum(B + (k - (T - 1)), 2 * B - 1), np.where(k < 3 * T, 2 * B, 2 * B - 1)))
    return _on_staircase(c, 4, B, 5), c, B


def big_record():
    """2^16 symbols x 2 rows of noise-free 16-QAM on a staircase of one test phase per 64 symbols, up in row 0 and down in row 1: 32 turns each, over
    256 tiles.  (y, c, M, B, W)."""
    M, B, W, n = 16, 32, 32, 1 << 16
    k = np.arange(n)
    c = np.stack([5 + k // 64, 1100 - k // 64])
    return np.stack([_on_staircase(c[0], M, B, 6), 0.5 * _on_staircase(c[1], M, B, 7)]), c, M, B, W


def fair(out, what):
    assert out["gap"].min() > MIN_GAP, (what, "gap", float(out["gap"].min()), int(out["gap"].argmin()))
    assert out["margin"] > MIN_MARGIN, (what, "margin", out["margin"])


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def test_constellation_has_unit_power_gray_neighbours_and_round_trips():
    for M in cn.ORDERS:
        pts, bits = cn.constellation(M)
        assert len(set(np.round(pts, 12))) == M
        assert abs(np.mean(np.abs(pts) ** 2) - 1.0) < 1e-14, M
        a, L = cn.half_spacing(M), cn.side(M)
        for i in range(M):                                        # nearest neighbours (distance 2 a) differ in exactly one bit
            near = np.nonzero(np.abs(np.abs(pts - pts[i]) - 2 * a) < 1e-12)[0]
            assert near.size in (2, 3, 4) or L == 2
            for j in near:
                assert int(np.sum(bits[i] != bits[j])) == 1, (M, i, j)
        rng = np.random.default_rng(M)
        b = rng.integers(0, 2, 4000 * cn.bits_per_symbol(M)).astype(np.uint8)
        np.testing.assert_array_equal(cn.decode(cn.encode(b, M), M), b)
        np.testing.assert_array_equal(cn.dec(cn.encode(b, M), M), cn.encode(b, M))
        np.testing.assert_array_equal(cn.gray_decode(cn.gray_encode(np.arange(L))), np.arange(L))


def test_qpsk_is_the_benchmark_fields_mapping():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (500, 2))
    want = ((2 * bits[:, 0] - 1) + 1j * (2 * bits[:, 1] - 1)) / np.sqrt(2)          # workloads.prbs_field / qpsk_field
    np.testing.assert_array_equal(cn.encode(bits.ravel().astype(np.uint8), 4), want)
    assert coherent._half_spacing(4) == 1 / np.sqrt(2) and all(coherent._half_spacing(M) == cn.half_spacing(M) for M in cn.ORDERS)


def test_decisions_on_and_beside_every_boundary():
    for M in cn.ORDERS:
        L, a = cn.side(M), cn.half_spacing(M)
        for m in range(-(L // 2 - 1), L // 2):
            x = 2 * a * m
            assert cn.level([x], M)[0] == m + L // 2 and cn.level([x + 1e-9 * a], M)[0] == m + L // 2 and cn.level([x - 1e-9 * a], M)[0] == m + L // 2 - 1
        np.testing.assert_array_equal(cn.level([0.0, -0.0, -9.0, 9.0, -np.inf, np.inf], M), [L // 2, L // 2, 0, L - 1, 0, L - 1])


def test_jump_rule_on_hand_made_sequences():
    B = 8
    #                 0  1  2  3  4  5  6  7  8  9
    b = np.array([0, 3, 7, 0, 4, 0, 7, 3, 7, 2])
    #   d:            -  3  4 -7  4 -4  7 -4  4 -5      2 d > 8: -1 ; 2 d < -8: +1 ; |d| = 4 = B / 2: no jump
    np.testing.assert_array_equal(cn.jumps(b, B), [0, 0, 0, 1, 0, 0, -1, 0, 0, 1])
    np.testing.assert_array_equal(cn.unwrap(b, B), b + B * np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 1]))
    np.testing.assert_array_equal(cn.jumps([5], B), [0])
    np.testing.assert_array_equal(cn.unwrap([1, 1, 1], 2), [1, 1, 1])
    np.testing.assert_array_equal(cn.jumps([0, 1, 0, 1], 2), [0, 0, 0, 0])             # B = 2: every step is |d| <= B / 2
    up = np.arange(40) % B                                                               # a steady climb wraps every B symbols
    np.testing.assert_array_equal(cn.unwrap(up, B), np.arange(40))
    np.testing.assert_array_equal(cn.unwrap(up[::-1].copy(), B), np.arange(39, -1, -1) - 32)


def test_window_truncation():
    assert cn.window(0, 5, 1) == (0, 1)
    for n, W in ((1, 0), (1, 7), (4, 7), (7, 7), (15, 7), (16, 7), (3, 256)):
        d = np.random.default_rng(n).random((n, 2))
        s = cn.window_sums(d, W)
        for k in range(n):
            lo, hi = cn.window(k, W, n)
            assert (lo, hi) == (max(0, k - W), min(n, k + W + 1))
            acc = np.zeros(2)
            for j in range(lo, hi):                              # the direct double loop, ascending j
                acc = acc + d[j]
            np.testing.assert_array_equal(s[k], acc)
    n, W = 15, 7                                                 # n = 2 W + 1: only the middle symbol sees the whole record
    assert [cn.window(k, W, n) for k in (0, 7, 14)] == [(0, 8), (0, 15), (7, 15)]


def test_a_noise_free_constant_rotation_is_recovered():
    for M, B in ((4, 32), (16, 32), (64, 64), (256, 16)):
        s = cn.encode(np.random.default_rng(M).integers(0, 2, 600 * cn.bits_per_symbol(M)).astype(np.uint8), M)
        for theta in (-0.7, -0.2, 0.0, 0.013, 0.3, 0.77):
            out = cn.bps(s * np.exp(1j * theta), M, B, 16)
            err = (out["phase"] - theta + np.pi / 4) % (np.pi / 2) - np.pi / 4
            assert np.max(np.abs(err)) <= np.pi / (4 * B) + 1e-12, (M, B, theta, float(np.max(np.abs(err))))
            assert np.all(out["index"] == out["index"][0])


def test_a_noise_free_ramp_across_five_sectors_is_followed_without_a_slip():
    for M, B in ((4, 32), (16, 32), (64, 64)):
        n = 4000
        s = cn.encode(np.random.default_rng(M + 1).integers(0, 2, n * cn.bits_per_symbol(M)).astype(np.uint8), M)
        for sign in (1.0, -1.0):
            theta = sign * np.linspace(0.0, 5 * np.pi / 2, n) + 0.1
            out = cn.bps(s * np.exp(1j * theta), M, B, 8)
            dev = (out["phase"] - out["phase"][0]) - (theta - theta[0])
            assert np.max(np.abs(dev)) <= np.pi / (2 * B) + 1e-12, (M, sign, float(np.max(np.abs(dev))))
            assert abs(int(out["index"][-1]) - int(out["index"][0])) >= 5 * B - 1


# ------------------------------------------------------------------------------------------------ the GPU suite's inputs are fair
def test_every_seeded_case_is_away_from_ties_and_boundaries_and_error_free():
    for name in SEEDED:
        y, s, bits, M, B, W = seeded(name)
        out = cn.bps(y * cn.scale_of(y), M, B, W)
        fair(out, name)
        z = cn.turn(out["symbols"], cn.quarter_turns(out["symbols"], s))
        assert int(np.sum(cn.decode(z, M) != bits)) == 0, name
    for i, (n, M, B, W) in enumerate(SEAMS):
        for dtype in (np.complex128, np.complex64):
            y = seam_record(n, M, i, dtype).astype(np.complex128)
            fair(cn.bps(y * cn.scale_of(y), M, B, W), (n, M, B, W, dtype.__name__))
    y, c, B = staircase_record()
    out = cn.bps(y, 4, B, 0)
    fair(out, "staircase")
    np.testing.assert_array_equal(out["index"], c)
    y, c, M, B, W = big_record()
    for r in range(2):
        out = cn.bps(y[r] * cn.scale_of(y[r]), M, B, W)
        fair(out, ("2^16", r))
        assert abs(int(out["index"][-1]) - int(out["index"][0])) > 30 * B
    # the records of the other GPU tests: two rows, the strided read, the silent window
    for seed, n, M, B, W in ((50, 2 * T + 32 + 1, 64, 32, 32), (51, 2 * T + 32 + 1, 64, 32, 32), (50, T + 1, 16, 32, 32), (51, T + 1, 16, 32, 32), (60, T + 7, 16, 32, 32),
                             (61, T + 7, 16, 32, 32)):
        for dtype in (np.complex128, np.complex64):
            y = seam_record(n, M, seed, dtype).astype(np.complex128)
            fair(cn.bps(y * cn.scale_of(y), M, B, W), (seed, n, M, B, W, dtype.__name__))
    y = seam_record(T + 5, 16, 70)
    y = y * cn.scale_of(y)
    y[T - 2 - 4:T - 2 + 4 + 1] = 0
    out = cn.bps(y, 16, 8, 4)
    assert out["gap"][T - 2] == 0 and np.delete(out["gap"], T - 2).min() > MIN_GAP        # the one exact tie, and no near-tie beside it


# ------------------------------------------------------------------------------------------------ the geometry header on the host
def test_the_tiles_header_against_brute_force_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "coherent_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", exe,
                    os.path.join(ROOT, "tests", "coherent_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.match(r"ok: \d+ checks", out.stdout), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(re.findall(r"\d+", out.stdout)[0]) > 1000000, out.stdout
    hdr = open(os.path.join(CSRC, "coherent_tiles.hpp")).read()
    for word in ("#include <hip", "__global__", "__device__", "hipStream", "dim3", "double2"):
        assert word not in hdr, word
    src = open(os.path.join(CSRC, "coherent.hip")).read()
    assert '#include "coherent_tiles.hpp"' in src
    for call in ("cpr::tile_begin(", "cpr::tile_end(", "cpr::halo_begin(", "cpr::halo_end(", "cpr::halo_base(", "cpr::window_begin(", "cpr::window_end(", "cpr::groups_of(",
                 "cpr::group_begin(", "cpr::group_end(", "cpr::grid_of(", "cpr::search_lds_bytes(", "cpr::jump_of(", "cpr::gray_decode(", "cpr::gray_encode(",
                 "cpr::level_of(", "cpr::level_amp(", "cpr::valid_search(", "cpr::valid_order("):
        assert call in src, call


# ------------------------------------------------------------------------------------------------ ABI and arguments
def test_the_abi_is_declared_bound_and_exported_and_the_tile_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "ssfm_amd.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"SSFM_API int %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "#define SSFM_ABI_VERSION 3" in hdr and lib.ssfm_abi_version() == 3
    assert "coherent" in oa.__all__ and oa.coherent is coherent
    tiles = open(os.path.join(CSRC, "coherent_tiles.hpp")).read()
    const = lambda name: int(eval(re.search(r"constexpr (?:int|int64_t) %s = ([^;]+);" % name, tiles).group(1).replace("int64_t(1)", "1")))      # noqa: E731
    assert coherent.CPR_TILE == const("kTile")
    assert (coherent._MAX_PHASES, coherent._MAX_WINDOW, coherent._MAX_SYMBOLS) == (const("kMaxPhases"), const("kMaxWindow"), const("kMaxSymbols"))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bcoherent\.hip\b", mk, re.M) and re.search(r"^HDR\s*:=.*\bcoherent_tiles\.hpp\b", mk, re.M)


def test_every_argument_error_comes_before_the_library_loads(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "_lib", None)
    y = np.exp(1j * np.arange(12.0))
    gv(sps=4, R=1e9)
    for kw in (dict(test_phases=31), dict(test_phases=66), dict(test_phases=0), dict(window=257), dict(window=-1)):
        with pytest.raises(ValueError):
            coherent.CPR(y, 16, **kw)
        with pytest.raises(ValueError):
            coherent.DSP(optical_signal(y), 16, **kw)
    for fn in (lambda: coherent.CPR(y, 8), lambda: coherent.QAM_ENCODER([0, 1, 0], 8), lambda: coherent.QAM_DECODER(y, 32), lambda: coherent.DSP(optical_signal(y), 8),
               lambda: coherent.EVM(y, M=5), lambda: coherent.EVM(y)):
        with pytest.raises(ValueError):
            fn()
    for bits, M in (([0, 1, 0], 4), ("0101011", 16), (np.zeros(13, np.uint8), 64), ([], 4)):
        with pytest.raises(ValueError, match="multiple of log2"):
            coherent.QAM_ENCODER(bits, M)
    with pytest.raises(ValueError, match=r"\(n,\) or \(2, n\)"):
        coherent.CPR(np.ones((3, 8), complex), 4)
    with pytest.raises(TypeError, match="complex record"):
        coherent.CPR(np.ones(8), 4)
    with pytest.raises(TypeError):
        coherent.DSP(y, 4)
    with pytest.raises(TypeError):
        coherent.CPR("0101", 4)
    with pytest.raises(ValueError):
        coherent.SHAPE(y, "triangle")
    with pytest.raises(ValueError):
        coherent.DSP(optical_signal(y), 4, instant=12)
    with pytest.raises(ValueError):
        coherent.BER([0, 1], [0, 1, 1])


def test_ber_of_host_sequences_needs_no_device():
    assert coherent.BER("0110", "0101") == 0.5 and coherent.BER([1, 1, 1], [1, 1, 1]) == 0.0
