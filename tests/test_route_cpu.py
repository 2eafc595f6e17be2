"""The shape of a plan and the routes of its entry points (opticomlib_amd/csrc/ssfm_route.hpp): N1 / N2 / E / Ef / Ef_fly / u16 / lanes / small for every
size and knob, and which engine a fixed-step or an adaptive call takes, against tables and restatements typed from the host file as it stood before the
header existed -- in a host program of its own under AddressSanitizer / UBSan (tests/route_host.cpp).  No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")
MOVED = ("small_supported", "small_points", "small_adapt_supported", "line_half_shape", "cols_per_tile", "u16_layout")
CONSTANTS = ("kLog2MaxDirect", "kMaxTables", "kSmallE16Min", "kSplitLog2M", "kSplitMaxR", "kAdaptSlots", "kAdaptWords", "kBarShards", "kBarWords", "medium_max_samples",
             "kMaxLanes")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_routes_against_the_parents_tables(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "route_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    "-o", exe, os.path.join(ROOT, "tests", "route_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.match(r"ok: \d+\n", out.stdout), out.stdout[-4000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 100000, out.stdout


def test_the_plan_uses_the_routes_it_tests():
    """The host file includes the header the program above checks; init, propagate_fixed and adaptive_begin* ask it; the predicates and constants that moved
    have no second definition under csrc/; the header is plain C++."""
    host = _read(CSRC, "ssfm_host.hip")
    assert '#include "ssfm_route.hpp"' in host

    def body(name):
        m = re.search(r"\n    int %s\(.*?\n    }\n" % name, host, re.S)
        assert m, name
        return m.group(0)
    assert "plan_shape<T>(" in body("init")
    assert "fixed_route<T>(" in body("propagate_fixed")
    assert "adaptive_route<T>(" in body("adaptive_begin")
    assert "adaptive_piece<T>(" in body("adaptive_begin_chunked")
    run = body("adaptive_run") + body("adaptive_chunks")
    assert "adaptive_one_launch(" in run and "adaptive_in_pieces(" in run and "adaptive_engine(" in run
    # last_engine: assigned once per entry point, from a route
    for name in ("propagate_fixed", "adaptive_run"):
        assert len(re.findall(r"\blast_engine = ", body(name))) == 1, name
    for name in ("adaptive_chunks", "run_deferred_small", "run_deferred_medium", "snapshots_small", "snapshots_every_step", "run_lanes", "adaptive_begin_chunked"):
        assert "last_engine =" not in body(name), name
    # every environment knob of plan creation is still read by the host file, by its name; the header reads none
    for knob in ("SSFM_SPLIT_ABOVE", "SSFM_SPLIT_LOG2M", "SSFM_E", "SSFM_EF", "SSFM_EF_FLY", "SSFM_LANES", "SSFM_SMALL", "SSFM_LANE_THREADS", "SSFM_ADAPT_FUSED", "SSFM_MEDIUM",
                 "SSFM_MEDIUM_ADAPT", "SSFM_MEDIUM_SPLIT", "SSFM_FUSED_PATIENCE_TICKS", "SSFM_PHASE_TABLE", "SSFM_FORCE_FLY", "SSFM_LANE_POOL_OFF"):
        assert 'std::getenv("%s")' % knob in host, knob
    hdr = _read(CSRC, "ssfm_route.hpp")
    for word in ("#include <hip", "__global__", "__device__", "getenv", "malloc", "new ", "std::vector", "std::string"):
        assert word not in hdr.replace("#define SSFM_HD __host__ __device__", ""), word
    # one definition of each moved name under csrc/, and it is the header's
    sources = {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))}
    for name in MOVED:
        where = [f for f, text in sources.items() if re.search(r"constexpr \w+ %s\(" % name, text)]
        assert where == ["ssfm_route.hpp"], (name, where)
    for name in CONSTANTS:
        where = [f for f, text in sources.items() if re.search(r"constexpr (int|long long) [^;()]*\b%s = " % name, text)]
        assert where == ["ssfm_route.hpp"], (name, where)
    assert '#include "ssfm_route.hpp"' in sources["ssfm_kernels.hpp"]
    assert "ssfm_route.hpp" in _read(CSRC, "Makefile")


def test_the_host_file_keeps_its_limits():
    """No member function of PlanT is longer than 120 lines (they begin and end at the struct's indentation)."""
    lines = _read(CSRC, "ssfm_host.hip").split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("template <typename T> struct PlanT"))
    end = next(i for i in range(start, len(lines)) if lines[i] == "};")
    i, longest = start + 1, (0, "")
    while i < end:
        if re.match(r"^    \S.*\)\s*(const\s*)?(override\s*)?\{\s*(//.*)?$", lines[i]) and not lines[i].strip().startswith(("struct", "//")):
            j = i + 1
            while j < end and not lines[j].startswith("    }"):
                j += 1
            longest = max(longest, (j - i + 1, lines[i].strip()))
            i = j
        i += 1
    assert 0 < longest[0] <= 120, longest


def test_python_and_c_name_the_same_engines_and_sizes():
    from opticomlib_amd import _lib
    hdr = _read(CSRC, "ssfm_route.hpp")
    assert _lib.DIRECT_LOG2_MAX == int(re.search(r"constexpr int kLog2MaxDirect = (\d+);", hdr).group(1))
    api = _read(ROOT, "include", "ssfm_amd.h")
    enum = [(m.group(1), int(m.group(2))) for m in re.finditer(r"^\s*SSFM_ENGINE_(\w+) = (\d+)", api, re.M)]
    assert [v for _, v in enum] == list(range(len(_lib.ENGINES))), enum
    names = {"NONE": "none", "ADAPT_3": "adaptive_3_launches", "ADAPT_FUSED": "adaptive_fused", "SMALL_ADAPT": "small_adaptive", "MEDIUM_ADAPT": "medium_adaptive",
             "SPLIT_ADAPT": "split_adaptive"}
    for (c_name, value) in enum:
        py = _lib.ENGINES[value]
        assert py == names.get(c_name, py) and (c_name in names or py.replace("adaptive", "adapt") == c_name.lower()), (c_name, value, py)
