"""The workspace table of the un-cut native step (fluidnet_amd/csrc/tfl_step_ws.hpp) in a stand-alone program under
AddressSanitizer and UBSan: tests/step_ws_host.cpp holds every region's offset and length to the expression tfl_simulate_step
used to write out, the total to the size tfl_simulate_workspace_floats used to restate, and the regions that are live at the
same time to being pairwise disjoint; compiled here for the host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_ws_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_ws_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "step_ws_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "step workspace OK" in out.stdout, out.stdout + out.stderr
