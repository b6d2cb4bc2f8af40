"""The host arithmetic of the training side (fluidnet_amd/csrc/tfl_train.hpp: weight re-layouts, tape / workspace layouts, the
weight-gradient kernel's chunk walk and its map back to the cudnn layout) in a stand-alone program under AddressSanitizer and
UBSan: tests/train_layout_host.cpp, compiled here for the host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "train_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "train layout OK" in out.stdout, out.stdout + out.stderr
