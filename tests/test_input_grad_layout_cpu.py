"""The host arithmetic of tfl_model_backward_input (fluidnet_amd/csrc/tfl_input_grad.hpp: the net input's channel map, the workspace
layout, the partial-sum slots; the two new weight forms of tfl_train.hpp and their device-refresh maps of tfl_refresh.hpp) in a
stand-alone program under AddressSanitizer and UBSan: tests/input_grad_layout_host.cpp, compiled here for the host and run as its
own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_input_grad_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "input_grad_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "input_grad_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "input grad layout OK" in out.stdout, out.stdout + out.stderr
