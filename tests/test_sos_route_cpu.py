"""The zero-phase SOS filter's host side (opticomlib_amd/csrc/sos_route.hpp, sos_tables.hpp): which shape and form a call takes for every size, knob, give-up count and
capacity, the give-up state over 2100 calls, and the device tables bit for bit, against restatements typed from the dispatcher and the builders as they stood before the
headers existed -- in a host program of its own under AddressSanitizer / UBSan (tests/sos_route_host.cpp).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal as sg

import sos_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")
KNOBS = ("SSFM_SOS_ONE_LAUNCH", "SSFM_SOS_NEAR", "SSFM_SOS_MEET", "SSFM_SOS_LONG_CHUNK", "SSFM_SOS_PATIENCE_US", "SOS_WAVES_FORCE")
CONSTANTS = ("kWave", "kSmallChunks", "kMaxSections", "kLookIter", "kNear", "kNearCertain", "kMaxGiveUps", "kRestCalls", "kChunkShort", "kChunkLong", "kWavesSmall", "kWavesLarge")
ROUTE_FUNCTIONS = ("geometry", "refusal", "near_is_certain", "look_of_group_powers", "tick_before_form", "after_one_launch", "choose_shape", "choose_form", "fill_route")
TABLE_FUNCTIONS = ("matmul", "build_tables", "build_meet_tables")
ORDERS, WNS, LAYOUTS = (1, 2, 4, 5, 6, 8), (0.3, 0.07, 0.02, 0.004), ((1, 12), (4, 12), (1, 18), (4, 18))
# Eight of the 24 filters have a power of some layout's group map within a factor 100 of the 1e-40 threshold that `look` is measured with: each is replaced by
# the nearest cut-off that has none (the comparison with sos_numpy.look_of is about the rule, not about one rounding).
NEIGHBOUR = {(1, 0.02): 0.021, (1, 0.004): 0.0045, (2, 0.004): 0.0043, (4, 0.02): 0.019, (4, 0.004): 0.0046, (5, 0.004): 0.005, (6, 0.004): 0.0044, (8, 0.004): 0.0065}
MAX_LINES = 90


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _filters():
    out = []
    for order in ORDERS:
        for wn in WNS:
            sos = sg.bessel(order, NEIGHBOUR.get((order, wn), wn), "low", norm="mag", output="sos")
            out.append((sos, sg.sosfilt_zi(sos)))
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """The host program, built and run once: its output."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    tmp = tmp_path_factory.mktemp("sos_route")
    exe, data = str(tmp / "sos_route_host"), str(tmp / "filters.txt")
    with open(data, "w") as f:
        for sos, zi in _filters():
            f.write(" ".join([str(sos.shape[0])] + [float(v).hex() for v in sos.reshape(-1)] + [float(v).hex() for v in zi.reshape(-1)]) + "\n")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", exe,
                    os.path.join(ROOT, "tests", "sos_route_host.cpp")], check=True)
    return subprocess.run([exe, data], capture_output=True, text=True)


def test_shape_form_give_ups_and_tables_against_the_parents(host_run):
    out = host_run
    last = out.stdout.strip().split("\n")[-1]
    assert out.returncode == 0 and re.fullmatch(r"ok: \d+", last), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(last.split()[1]) > 100000, last


def test_look_is_the_depth_the_bound_assumes(host_run):
    """`look` of every filter and layout equals sos_numpy.look_of, and none of these filters has a group power within a factor 100 of the 1e-40
    threshold (the comparison is about the rule, not about one rounding)."""
    looks = {tuple(int(v) for v in l.split()[1:4]): int(l.split()[4]) for l in host_run.stdout.split("\n") if l.startswith("look ")}
    filters = _filters()
    assert len(looks) == len(filters) * len(LAYOUTS)
    for i, (sos, _) in enumerate(filters):
        for W, L in LAYOUTS:
            peaks = np.abs(sn.device_tables(sos, W, L).P[1, 1:]).max(axis=(1, 2))
            assert not ((peaks > sn.DROP / 100) & (peaks < sn.DROP * 100)).any(), (i, W, L, peaks[(peaks > sn.DROP / 100) & (peaks < sn.DROP * 100)])
            assert looks[(i, W, L)] == sn.look_of(sos, W, L), (i, W, L, looks[(i, W, L)], sn.look_of(sos, W, L))


def _functions(text):
    """(lines, first line) of every function defined at namespace or struct scope: from the line that opens its body to the closing brace at that line's indentation."""
    lines, out, i = text.split("\n"), [], 0
    while i < len(lines):
        l = lines[i]
        if re.match(r"^(    )?[A-Za-z].*\)\s*(const\s*)?\{\s*(//.*)?$", l) and not l.lstrip().startswith(("struct", "namespace", "//", "#", "if", "for", "while", "switch", "else")):
            pad = l[:len(l) - len(l.lstrip())]
            j = i + 1
            while j < len(lines) and not lines[j].startswith(pad + "}"):
                j += 1
            start = i
            while start > 0 and lines[start - 1].startswith(pad + "template"):
                start -= 1
            out.append((j - start + 1, l.strip()))
            i = j
        i += 1
    return out


def test_the_filter_uses_the_routes_it_tests():
    host = _read(CSRC, "sos_filter.hip")
    route, tables, inc = _read(CSRC, "sos_route.hpp"), _read(CSRC, "sos_tables.hpp"), _read(CSRC, "sos_filter_impl.inc")
    assert '#include "sos_route.hpp"' in host and '#include "sos_tables.hpp"' in host
    for name in ("choose_shape(", "choose_form(", "tick_before_form(", "after_one_launch(", "fill_route(", "look_of_group_powers(", "refusal(", "build_tables<", "build_meet_tables<"):
        assert name in host, name
    # every knob is read by the host file, by its name, for every call; the headers read none
    for knob in KNOBS:
        assert 'std::getenv("%s")' % knob in host, knob
        assert knob not in inc, knob
    for hdr in (route, tables):
        for word in ("#include <hip", "__global__", "__device__", "getenv", "hipMalloc"):
            assert word not in hdr, word
    assert "std::vector" not in route and "new " not in route and "malloc" not in route
    # one definition of each moved name under csrc/, and it is the header's
    sources = {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))}
    for name in CONSTANTS:
        where = [f for f, text in sources.items() if re.search(r"constexpr (int|long long) [^;()]*\b%s = " % name, text)]
        assert where == ["sos_route.hpp"], (name, where)
    for names, header in ((ROUTE_FUNCTIONS, "sos_route.hpp"), (TABLE_FUNCTIONS, "sos_tables.hpp")):
        for name in names:
            where = [f for f, text in sources.items() if re.search(r"^[\w<>:,\s\*&]*\b%s\([^;]*\) \{" % name, text, re.M)]
            assert where == [header], (name, where)
    where = [f for f, text in sources.items() if re.search(r"long long one_launch_capacity\(\) \{", text)]
    assert where == ["sos_filter_impl.inc"], where
    assert "sos_route.hpp" in _read(CSRC, "Makefile") and "sos_tables.hpp" in _read(CSRC, "Makefile")


def test_the_host_functions_keep_their_length():
    """No function of sos_filter.hip, or of the host glue of sos_filter_impl.inc, is longer than 90 lines."""
    host = _functions(_read(CSRC, "sos_filter.hip"))
    inc = _read(CSRC, "sos_filter_impl.inc")
    glue = _functions(inc[inc.index("host glue"):])
    assert len(host) >= 12 and len(glue) >= 3, (host, glue)
    longest = max(host + glue)
    assert longest[0] <= MAX_LINES, longest
