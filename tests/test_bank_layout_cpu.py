"""The host arithmetic of the banked models' training pass (fluidnet_amd/csrc/tfl_train.hpp: the extended tape / workspace
layouts, the weight-gradient plan and chunk walk at tap spacing 1 / 2 / 4, the index maps of the join's and the pyramid pool's
backward) in a stand-alone program under AddressSanitizer and UBSan: tests/bank_layout_host.cpp, compiled here for the host and
run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bank_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bank_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bank_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bank layout OK" in out.stdout, out.stdout + out.stderr
