"""The yardstick of tfl_model_backward, validated on the CPU before any GPU run trusts it (tests/model_grad_ref.py):

 * its forward equals the numpy / C restatement of lib/model.lua (oracle/simulate_np.model_forward) on every test model;
 * PyTorch-CPU fp32 autograd of the same graph lies within the 1e-5 bar of its fp64 gradients on every test input, for every
   parameter tensor -- the reference alone passes the bar the GPU is held to;
 * the layer-by-layer formulas the kernels implement (manual_grads) equal autograd, and each of four ways to get them wrong
   exceeds the bar on every input where the mistake changes anything at all -- and on at least half of the cases;
 * the closed loop's learning rate and step count halve the fp64 loss.
"""
import numpy as np
import pytest
import torch

import model_grad_ref as R
import scenes
from oracle import simulate_np as S


def _model(name):
    _, kind, is3D, opts, _ = R.case(name)
    return R.make_model(kind, is3D, opts)


@pytest.mark.parametrize("name", R.NAMES)
def test_restated_forward_is_the_oracles(oracle, name):
    m = _model(name)
    pDiv, UDiv, flags, _, _ = R.make_inputs(name)
    with torch.no_grad():
        p, U, _ = R.forward(m.layers, pDiv, UDiv, flags, m.opts)
    p0, U0 = S.model_forward(oracle, m.layers, pDiv.copy(), UDiv.copy(), flags.copy(), opts=m.opts)
    ep, eu = scenes.rel_l2(p.numpy(), p0), scenes.rel_l2(U.numpy(), U0)
    print("%s: forward vs oracle rel-L2 p %.2e U %.2e" % (name, ep, eu))
    assert ep <= 1e-6 and eu <= 1e-6


@pytest.mark.parametrize("mode", R.GRAD_MODES)
@pytest.mark.parametrize("name", R.NAMES)
def test_torch_fp32_autograd_passes_the_bar(name, mode):
    want, fp32, zero_l1 = R.expected(name, mode)
    rel = R.rel_l2_per_tensor(fp32, want, zero_l1)
    print("%s %s: PyTorch-CPU fp32 vs fp64, worst %.2e" % (name, mode, max(max(r) for r in rel)))
    for l, (ew, eb) in enumerate(rel):
        assert ew <= R.BAR and eb <= R.BAR, (l, ew, eb)
    for l, (gw, gb) in enumerate(want):          # no tensor of the yardstick is zero, but the one that must be
        assert np.linalg.norm(gw) > 0 and (np.linalg.norm(gb) > 0 or (zero_l1 is not None and l + 1 == len(want)))


@pytest.mark.parametrize("name", R.NAMES)
def test_layer_formulas_equal_autograd(name):
    m = _model(name)
    pDiv, UDiv, flags, gP, gU = R.make_inputs(name)
    got = R.manual_grads(m.layers, pDiv, UDiv, flags, gP, gU, m.opts)
    assert R.worst(got, R.expected(name)[0]) <= 1e-12


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_exceed_the_bar(mutant):
    caught = 0
    for name in R.NAMES:
        m = _model(name)
        pDiv, UDiv, flags, gP, gU = R.make_inputs(name)
        if not R.mutant_applies(mutant, m.layers, m.opts, flags.shape[-1]):
            continue
        e = R.worst(R.manual_grads(m.layers, pDiv, UDiv, flags, gP, gU, m.opts, mutant=mutant), R.expected(name)[0])
        print("%s on %s: worst rel-L2 %.2e" % (mutant, name, e))
        assert e > R.BAR, (mutant, name, e)
        caught += 1
    assert caught >= len(R.NAMES) // 2


def test_loop_settings_halve_the_fp64_loss(oracle):
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    m = R.loop_model()
    U_bc = UDiv.copy()
    oracle.setWallBcsForward(U_bc, flags)
    div = np.zeros_like(flags)
    oracle.velocityDivergenceForward(U_bc, flags, div)
    pT = np.zeros_like(flags)
    oracle.solveLinearSystemJacobi(pT, flags, div, False, 0, L["jacobi_iters"])
    UT = U_bc.copy()
    oracle.velocityUpdateForward(UT, flags, pT)
    oracle.setWallBcsForward(UT, flags)
    losses, _ = R.train_loop(m.layers, m.opts, pDiv, U_bc, flags, pT, UT, L["lambdas"], L["lr"], L["steps"])
    print("fp64 loop: loss %.4e -> %.4e over %d steps" % (losses[0], losses[-1], L["steps"]))
    assert losses[-1] <= 0.5 * losses[0]
