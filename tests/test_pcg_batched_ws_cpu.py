"""The workspace table of solveLinearSystemPCGBatched (pcg_batched_ws, fluidnet_amd/csrc/tfl_pcg_ws.hpp) in a stand-alone program
under AddressSanitizer and UBSan: tests/pcg_batched_ws_host.cpp walks it for B = 1, 3, 16 at odd 2-D and 3-D sizes -- every region
disjoint and inside the total, the stride 8-byte aligned, the existing pcg_ws offsets and totals unchanged; compiled here for the
host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcg_batched_ws_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pcg_batched_ws_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pcg_batched_ws_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pcg batched workspace OK" in out.stdout, out.stdout + out.stderr
