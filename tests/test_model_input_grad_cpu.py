"""The yardstick of tfl_model_backward_input, validated on the CPU before any GPU run trusts it (tests/model_input_grad_ref.py):

 * the six pieces the kernels implement (manual_input_grads) equal float64 autograd of the restatement with pDiv and UDiv as
   leaves, to 1e-12, on every case and gradient mode (model_grad_ref's 18 and the two of model_input_grad_ref.EXTRA);
 * PyTorch-CPU fp32 autograd of the same graph lies within the 1e-5 bar of float64 -- the gradient is well posed in fp32
   (measured: worst 4.13e-6, norm-l2-pdiv / u-only / gradPDiv; every other tensor at or below 6e-7);
 * each of six ways to get the pieces wrong exceeds the bar on at least one case and mode where the mistake changes anything;
 * two chained passes, net(net(x)), in fp32 pass the bar for every parameter tensor and both leaf inputs.
"""
import pytest
import torch

import model_grad_ref as R
import model_input_grad_ref as I


@pytest.mark.parametrize("mode", R.GRAD_MODES)
@pytest.mark.parametrize("name", I.NAMES)
def test_the_six_pieces_equal_autograd(name, mode):
    want = I.input_grads(name, mode)
    got = I.manual_input_grads(name, mode)
    e = [I.rel_l2(g, w) for g, w in zip(got, want)]
    assert max(e) <= 1e-12, e


@pytest.mark.parametrize("mode", R.GRAD_MODES)
@pytest.mark.parametrize("name", I.NAMES)
def test_torch_fp32_autograd_passes_the_bar(name, mode):
    want = I.input_grads(name, mode)
    e = [I.rel_l2(g, w) for g, w in zip(I.input_grads(name, mode, torch.float32), want)]
    print("%s %s: PyTorch-CPU fp32 vs fp64, gradPDiv %.2e gradUDiv %.2e" % (name, mode, e[0], e[1]))
    assert max(e) <= I.BAR, e
    if name == "udiv-without-pdiv":          # neither the pDiv channel, nor the skip, nor a pDiv normaliser: exactly zero
        assert not want[0].any()


@pytest.mark.parametrize("mutant", I.MUTANTS)
def test_mutants_exceed_the_bar(mutant):
    caught = applied = 0
    for name in I.NAMES:
        for mode in R.GRAD_MODES:
            if not I.mutant_applies(mutant, name, mode):
                continue
            applied += 1
            e = I.worst(I.manual_input_grads(name, mode, mutant=mutant), I.input_grads(name, mode))
            print("%s on %s %s: worst rel-L2 %.2e" % (mutant, name, mode, e))
            caught += e > I.BAR
    assert applied > 0 and caught > 0, (mutant, applied, caught)


@pytest.mark.parametrize("name", I.CHAIN_CASES)
def test_two_chained_passes_in_fp32_pass_the_bar(name):
    want, want_in = I.chain_param_grads(name, 2)
    got, got_in = I.chain_param_grads(name, 2, torch.float32)
    e = R.worst(got, want)
    ei = I.worst(got_in, want_in)
    print("%s: two passes, PyTorch-CPU fp32 vs fp64, parameters %.2e inputs %.2e" % (name, e, ei))
    assert e <= I.BAR and ei <= I.BAR
