"""The capture rings and the adaptive chunks (opticomlib_amd/csrc/ssfm_capture.hpp): how a z-resolved capture lays out its ring of device blocks, which slot a
snapshot takes and what its writer waits for, how an adaptive run is cut into chunks -- against a restatement typed from the host files as they stood before
the header existed, in a model of the ring under random scheduling that rejects four mutants, and in a model of the adaptive loop, in a host program of its
own under AddressSanitizer / UBSan (tests/capture_host.cpp).  And: the host files ask the header and decide none of it themselves.  No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticomlib_amd", "csrc")
CONSTANTS = ("kCapBlockBytes", "kCapBlockSnaps", "kCapBlocksMax", "kCapRingBytes", "kAcapHalfSlots", "kAcapHalfBytes", "kAdaptChunkMax", "kLineChunkMax")
# what CapRun and AdaptCap held loose before they held a CapRing, a ScalLog and a CapCursor
LOOSE = ("per_block", "nsnap", "nflush", "nblocks", "step_doubles", "per_row", "next_in_list", "half_slots", "chunk_no")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_rings_and_chunks_against_the_parents_arithmetic_and_in_their_models(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "capture_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
                    "-o", exe, os.path.join(ROOT, "tests", "capture_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.match(r"ok: \d+ ", out.stdout), out.stdout[-4000:] + out.stderr[-4000:]
    print(out.stdout)
    counts = [int(x) for x in re.findall(r"\d+", out.stdout)]
    # (seen: 333 million cells, 332 million of them the restatement's; 196350 runs of the ring's model, 6000 of the adaptive loop's)
    assert counts[0] > 300000000 and counts[2] > 150000 and counts[3] >= 6000, out.stdout


def test_the_host_files_ask_the_header_and_decide_none_of_it_themselves():
    sources = {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))}
    host, hdr = sources["ssfm_host.hip"], sources["ssfm_capture.hpp"]
    for f in ("ssfm_host.hip", "chirpz.hip", "manakov.hip"):
        assert '#include "ssfm_capture.hpp"' in sources[f], f
    # one definition of each constant under csrc/, and it is the header's
    for name in CONSTANTS:
        where = [f for f, text in sources.items() if re.search(r"constexpr (size_t|int64_t|int) %s = " % name, text)]
        assert where == ["ssfm_capture.hpp"], (name, where)
    # the three estimates ("queue three quarters of what remains") are one, and the block and ring sizes are spelled nowhere else
    for f, text in sources.items():
        if f.endswith(".hip"):
            assert "0.75 *" not in text, f
    for f in ("chirpz.hip", "manakov.hip"):
        assert "ssfm::chunk_estimate(length - (now.z - now.h), now.h, ssfm::kLineChunkMax, false)" in sources[f], f
    for spelled in ("size_t(8) << 20", "size_t(1) << 30", "size_t(512) << 20", "size_t(8) << 30"):
        assert spelled not in host, spelled
    # CapRun and AdaptCap hold the header's structs and no loose copy of their fields; the plan calls what it used to compute
    start = host.index("template <typename T> struct PlanT")
    plan = host[start:host.index("\n};", start)]
    assert re.search(r"^        CapRing ring;", plan, re.M) and re.search(r"^        ScalLog log\b", plan, re.M) and re.search(r"^        CapCursor cur;", plan, re.M)
    for name in LOOSE:
        assert not re.search(r"^\s+(?:bool|int|size_t|int64_t)\s[^;()]*\b%s\b[^;()]*;" % name, plan, re.M), name
    for call in ("CapRing::make(", "scal_log<T>(", ".captures(s)", ".slot_of(", ".flush_of(", "snap_block(", "snap_whole(", "acap_list_valid(", "acap_half_slots(", "acap_ring_bytes(",
                 "cur.wants(", "cur.room(", "cur.cut(", "cur.half_offset(", "cur.sent(", "cur.reset()", "caps_taken(", "chunk_next(", "chunk_estimate("):
        assert call in plan, call
    for word in ("#include <hip", "__global__", "__device__", "getenv", "std::thread", "std::atomic", "new ", "malloc", "std::vector"):
        assert word not in hdr, word
    assert re.search(r"^HDR\s*:=.*\bssfm_capture\.hpp\b", _read(CSRC, "Makefile"), re.M)


def test_no_new_plan_function_is_long_and_the_capture_entry_point_is_short():
    """propagate_fixed_capture was 77 lines before the header took its arithmetic; the function that makes its resources is new."""
    host = _read(CSRC, "ssfm_host.hip").split("\n")

    def length(name):
        first = next(i for i, line in enumerate(host) if re.match(r"    int %s\(" % name, line))
        return next(i for i in range(first, len(host)) if host[i] == "    }") - first + 1
    assert length("propagate_fixed_capture") < 50
    assert length("capture_resources") <= 60
