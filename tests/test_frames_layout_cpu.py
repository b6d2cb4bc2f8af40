"""The layout arithmetic of the resident frame store (fluidnet_amd/csrc/tfl_frames.hpp: plane and slot offsets, the plane ->
output tensor map, the per-thread vector / tail split of k_frames_gather) in a stand-alone program under AddressSanitizer and
UBSan: tests/frames_layout_host.cpp, compiled here for the host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frames_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frames_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "frames_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "frames layout OK" in out.stdout, out.stdout + out.stderr
