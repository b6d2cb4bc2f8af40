"""The index maps of the device-side weight refresh and of the optimiser step's flat parameter space
(fluidnet_amd/csrc/tfl_refresh.hpp) in a stand-alone program under AddressSanitizer and UBSan: tests/refresh_layout_host.cpp
walks them on the host as the kernels do and holds every weight form to the host packers byte for byte; compiled here for the
host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refresh_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "refresh_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "refresh_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refresh layout OK" in out.stdout, out.stdout + out.stderr
