"""The level geometry and index maps of the multigrid preconditioner (fluidnet_amd/csrc/tfl_pcg_mg.hpp) and the block it appends
to the PCG workspace (tfl_pcg_ws.hpp) in a stand-alone program under AddressSanitizer and UBSan: tests/pcg_mg_ws_host.cpp walks
mg_levels and the appended block -- every region disjoint and inside the total, the old offsets and totals unchanged, every child
inside its parent's extent and every parent's children inside the fine extent, odd sizes included; compiled here for the host and
run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcg_mg_ws_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pcg_mg_ws_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pcg_mg_ws_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pcg mg workspace OK" in out.stdout, out.stdout + out.stderr
