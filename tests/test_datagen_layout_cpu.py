"""The scatter map of the frame store (fluidnet_amd/csrc/tfl_frames.hpp: device tensors into slots, as k_frames_scatter walks it)
and the primitive / hash / curl arithmetic of the scene kernels (fluidnet_amd/csrc/tfl_datagen.hpp) in a stand-alone program under
AddressSanitizer and UBSan: tests/datagen_layout_host.cpp, compiled here for the host and run as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_datagen_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "datagen_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "datagen_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "datagen layout OK" in out.stdout, out.stdout + out.stderr
