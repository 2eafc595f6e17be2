"""Lane health (opticomlib_amd/csrc/ssfm_lanes.hpp): the rule by which a two-lane plan rates its streams, looks at its long runs, heals a lane, drops to one
lane, comes back and hands its pair to the pool -- against a restatement typed from the host file as it stood before the header existed, event by event and
bit by bit, in a host program of its own under AddressSanitizer / UBSan (tests/lanes_host.cpp).  And: the host file asks the header and writes none of its
fields; ``_lib.RunInfo`` is the C struct.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")
FIELDS = ("lanes_active", "lanes_ok", "lanes_dropped", "lanes_remade", "lanes_share_queue", "lanes_from_pool", "lane_heals", "lane_strikes", "lane_suspect",
          "lane_dropped_runs", "lane_fault", "lane_alone_us", "lane_pair_us", "lane_last_us", "lane_score", "lane_check_pending", "lane_check_launches")
CONSTANTS = ("kLaneGoodRatio", "kLaneGoodRatioBig", "kLaneSlowRatio", "kLaneSuspectRatio", "kLaneDroppedCooldown", "kLaneProbeSteps", "kLaneHealsMax")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_lane_health_against_the_parents_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "lanes_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    "-o", exe, os.path.join(ROOT, "tests", "lanes_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.match(r"ok: \d+\n", out.stdout), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 1000000, out.stdout


def test_the_plan_asks_the_header_and_writes_none_of_its_fields():
    host = _read(CSRC, "ssfm_host.hip")
    assert '#include "ssfm_lanes.hpp"' in host
    start = host.index("template <typename T> struct PlanT")
    plan = host[start:host.index("\n};", start)]
    assert re.search(r"^    LaneHealth lanes;$", plan, re.M)
    for name in FIELDS:
        assert not re.search(r"^\s+(?:bool|int|float|int64_t)\s[^;()]*\b%s\b[^;()]*;" % name, plan, re.M), name
    # no field is assigned, counted up or down outside the header (`lanes.` or `P_->lanes.` in front or not)
    sources = {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))}
    for f, text in sources.items():
        if f == "ssfm_lanes.hpp":
            continue
        for name in FIELDS:
            for pattern in (r"\b%s\s*(=|\+=|\*=)[^=]" % name, r"(\+\+|--)\s*(\w+\.)?%s\b" % name, r"\b%s\s*(\+\+|--)" % name):
                assert not re.search(pattern, text), (f, name, re.search(pattern, text).group(0))
    # one definition of each constant under csrc/, and it is the header's; the host file does not even name them
    for name in CONSTANTS:
        where = [f for f, text in sources.items() if re.search(r"constexpr (float|int) %s = " % name, text)]
        assert where == ["ssfm_lanes.hpp"], (name, where)
        assert name not in host, name
    hdr = sources["ssfm_lanes.hpp"]
    for word in ("#include <hip", "__global__", "__device__", "getenv", "std::thread", "new ", "malloc"):
        assert word not in hdr, word
    assert re.search(r"^HDR\s*:=.*\bssfm_lanes\.hpp\b.*\bssfm_split\.hpp\b", _read(CSRC, "Makefile"), re.M)


C_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}


def test_python_and_c_lay_the_run_info_out_alike():
    """``_lib.RunInfo`` against ``ssfm_run_info`` of include/ssfm_amd.h: the same names in the same order, matching types, and the size the C layout gives
    (every member aligned to its own size, the struct to its widest member)."""
    from opticomlib_amd import _lib
    api = re.sub(r"/\*.*?\*/", "", _read(ROOT, "include", "ssfm_amd.h"), flags=re.S)
    body = re.search(r"typedef struct ssfm_run_info \{(.*?)\} ssfm_run_info;", api, re.S).group(1)
    members = [(m.group(2), m.group(1)) for m in re.finditer(r"^\s*(\w+)\s+(\w+);", body, re.M)]
    assert len(members) == len([l for l in body.split("\n") if l.strip()]) >= 17, body          # every line of the struct is one plain member
    assert [(n, C_TYPES[t]) for n, t in members] == list(_lib.RunInfo._fields_)
    offset = widest = 0
    for _, t in members:
        size = ctypes.sizeof(C_TYPES[t])
        offset = (offset + size - 1) // size * size + size
        widest = max(widest, size)
    assert ctypes.sizeof(_lib.RunInfo) == (offset + widest - 1) // widest * widest == 80
    assert _lib.RunInfo.lanes_from_pool.offset == 56 and _lib.RunInfo.lane_ratings_total.offset == 64
