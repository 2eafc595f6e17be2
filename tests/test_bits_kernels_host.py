"""The streaming kernels of csrc/bits.hip, run on the host: their text between the two marks is compiled with tests/bits_host_emulation.cpp, which runs
every lane of every workgroup in turn under AddressSanitizer on exactly sized buffers and compares each result with the plain loop -- every
source and destination offset modulo 16, and results above the grid cap, where the grid-stride loops go round a second time.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_tile_and_stride_kernels_lane_by_lane(tmp_path):
    src = open(os.path.join(ROOT, "opticomlib_amd", "csrc", "bits.hip")).read()
    begin, end = src.index("// [host-emulated: begin]"), src.index("// [host-emulated: end]")
    body = src[begin:end]
    assert "k_bits_map" in body and "k_bits_tile" in body and "k_bits_stride" in body
    (tmp_path / "bits_kernels.inc").write_text(body)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the emulation"
    exe = str(tmp_path / "emulation")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{tmp_path}", "-o", exe,
                    os.path.join(ROOT, "tests", "bits_host_emulation.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout[-2000:] + out.stderr[-4000:]
