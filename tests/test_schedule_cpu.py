"""ssfm::Schedule (opticomlib_amd/csrc/ssfm_schedule.hpp) -- what the fixed-step entry points know about a run's step sizes: the first unusable step, the
distinct sizes in order of first appearance, the table index of every step -- against a brute-force restatement, in a host program of its own under
AddressSanitizer / UBSan (tests/schedule_host.cpp).  No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")


def test_schedule_against_brute_force(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    route = open(os.path.join(CSRC, "ssfm_route.hpp")).read()
    kmax = int(re.search(r"constexpr int kMaxTables = (\d+)[,;]", route).group(1))
    exe = str(tmp_path / "schedule_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DK_MAX_TABLES={kmax}",
                    f"-I{CSRC}", "-o", exe, os.path.join(ROOT, "tests", "schedule_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout[-2000:] + out.stderr[-4000:]


def test_the_plan_uses_the_schedule_it_tests():
    """The host file includes the header the program above checks, and checks no step size by itself any more; the header is plain C++."""
    host = open(os.path.join(CSRC, "ssfm_host.hip")).read()
    assert '#include "ssfm_schedule.hpp"' in host and "Schedule<T> sch(" in host and "upload_schedule(sch)" in host
    assert "isfinite" not in host                                       # (the one rule for a usable step is Schedule's)
    hdr = open(os.path.join(CSRC, "ssfm_schedule.hpp")).read()
    assert "#include <hip" not in hdr and "__global__" not in hdr and "__device__" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ssfm_schedule.hpp" in mk and "ssfm_owned.hpp" in mk
