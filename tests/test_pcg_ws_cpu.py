"""The workspace tables of solveLinearSystemPCG and normalizePressureMean (fluidnet_amd/csrc/tfl_pcg_ws.hpp) in a stand-alone
program under AddressSanitizer and UBSan: tests/pcg_ws_host.cpp holds every region's offset and length to the expression
pcg_solve / normalize_pressure_mean used to write out, the totals to the sizes pcg_workspace_floats / npm_workspace_floats used
to restate, all regions to being pairwise disjoint and inside the total for every run-time alignment pad, the alignment of the
fp64 regions and of the wavefront block, the span of the per-solve memset and the guard pairs of the hand-off arrays; compiled
here for the host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcg_ws_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pcg_ws_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pcg_ws_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pcg workspace OK" in out.stdout, out.stdout + out.stderr
