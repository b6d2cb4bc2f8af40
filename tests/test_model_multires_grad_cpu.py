"""CPU checks of tests/model_multires_grad_ref.py, the yardstick of the training pass of linear models with pooling / upsampling
layers: the layer-by-layer formulas equal fp64 autograd, the inputs are well enough conditioned that
PyTorch-CPU's own fp32 autograd meets the project's bar on them, every mutant of the formulas misses the bar by two orders of
magnitude, and the host arithmetic of the layouts and index maps is clean under AddressSanitizer / UBSan (a stand-alone program)."""
import os
import subprocess

import pytest
import torch

import model_input_grad_ref as IR
import model_multires_grad_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", M.NAMES)
def test_manual_formulas_equal_fp64_autograd(name):
    for mode in M.GRAD_MODES:
        want, want_in, l1 = M.grads(name, mode)
        got, got_in = M.manual_grads(name, mode)
        assert M.worst(name, mode, got, want, l1) <= 1e-12, mode
        assert IR.worst(got_in, want_in) <= 1e-12, mode


@pytest.mark.parametrize("name", M.NAMES)
def test_pytorch_fp32_meets_the_bar_on_these_inputs(name):
    """a condition on the inputs, not on the code under test"""
    for mode in M.GRAD_MODES:
        want, want_in, l1 = M.grads(name, mode)
        fp32, fp32_in, _ = M.grads(name, mode, torch.float32)
        rel = M.rel_l2_per_tensor(name, mode, fp32, want, l1)
        print("fp32 witness %s %s: params %.3e, inputs %.3e" % (name, mode, max(max(r) for r in rel), IR.worst(fp32_in, want_in)))
        for l, (ew, eb) in enumerate(rel):
            assert ew <= M.BAR and eb <= M.BAR, (mode, l, ew, eb)
        assert IR.worst(fp32_in, want_in) <= M.BAR, mode


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_misses_the_bar_by_two_orders(mutant):
    hit = 0
    for name in M.NAMES:
        if not M.mutant_applies(mutant, name):
            continue
        hit += 1
        want, want_in, l1 = M.grads(name, "both")
        got, got_in = M.manual_grads(name, "both", mutant=mutant)
        miss = max(M.worst(name, "both", got, want, l1), IR.worst(got_in, want_in))
        print("mutant %s on %s: %.3e" % (mutant, name, miss))
        assert miss >= 100 * M.BAR, (name, miss)
    assert hit >= 2


def test_multires_layout_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "multires_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "multires_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "multires layout OK" in out.stdout, out.stdout + out.stderr
