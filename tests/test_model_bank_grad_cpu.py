"""The yardstick of the banked models' backward pass (tests/model_bank_grad_ref.py), checked on the CPU before the GPU tests rely
on it: its forward is model_graph_ref's on the oracle's ops, its module-by-module formulas equal autograd in fp64, PyTorch-CPU's
own fp32 autograd passes the bar on every case (so the inputs leave the bar reachable for fp32 arithmetic), and every mutant of
the formulas fails the bar where it applies."""
import numpy as np
import pytest
import torch

import model_bank_grad_ref as K
import model_grad_ref as R
import scenes


def _mode(name, mode):
    pDiv, UDiv, flags, gP, gU = K.make_inputs(name)
    return pDiv, UDiv, flags, (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


@pytest.mark.parametrize("name", K.NAMES)
def test_restated_forward_is_the_graph_reference(name, oracle):
    import model_graph_ref as G
    m = K.make_model(name)
    pDiv, UDiv, flags, _, _ = K.make_inputs(name)
    with torch.no_grad():
        p, U, _, _, _ = K.forward(m, m.layers, pDiv, UDiv, flags, torch.float64)
    p0, U0 = G.model_forward(oracle, m, np.array(pDiv), np.array(UDiv), np.array(flags), conv_dtype="float64")
    # (the oracle's ops and graph_stack's result are fp32 arrays: agreement to fp32 rounding of an fp64 conv stack)
    assert scenes.rel_l2(p.numpy(), np.asarray(p0, np.float64)) <= 1e-6
    assert scenes.rel_l2(U.numpy(), np.asarray(U0, np.float64)) <= 1e-6


@pytest.mark.parametrize("name", K.NAMES)
def test_manual_formulas_equal_autograd_in_fp64(name):
    m = K.make_model(name)
    for mode in K.GRAD_MODES:
        pDiv, UDiv, flags, gP, gU = _mode(name, mode)
        want, l1, _ = K.grads(m, m.layers, pDiv, UDiv, flags, gP, gU)
        got, g_x = K.manual_grads(m, m.layers, pDiv, UDiv, flags, gP, gU)
        zero_l1 = l1 if mode == "u-only" else None
        assert max(max(r) for r in K.rel_l2_per_tensor(got, want, zero_l1)) <= 1e-12, mode
        assert scenes.rel_l2(g_x, K.x_grad(m, m.layers, pDiv, UDiv, flags, gP, gU)) <= 1e-12, mode


@pytest.mark.parametrize("name", K.NAMES)
def test_pytorch_fp32_passes_the_bar(name):
    for mode in K.GRAD_MODES:
        want, fp32, zero_l1, in64, in32 = K.expected(name, mode)
        rel = K.rel_l2_per_tensor(fp32, want, zero_l1)
        assert max(max(r) for r in rel) <= K.BAR, (mode, rel)
        assert max(scenes.rel_l2(a, b) for a, b in zip(in32, in64)) <= K.BAR, mode


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_fails_the_bar_where_it_applies(mutant):
    names = [n for n in K.NAMES if K.mutant_applies(mutant, n)]
    assert names
    caught = 0
    for name in names:
        m = K.make_model(name)
        pDiv, UDiv, flags, gP, gU = K.make_inputs(name)
        want, _, _ = K.grads(m, m.layers, pDiv, UDiv, flags, gP, gU)
        got, g_x = K.manual_grads(m, m.layers, pDiv, UDiv, flags, gP, gU, mutant=mutant)
        err = max(max(max(r) for r in K.rel_l2_per_tensor(got, want)),
                  scenes.rel_l2(g_x, K.x_grad(m, m.layers, pDiv, UDiv, flags, gP, gU)))
        assert err > K.BAR, (name, err)          # every case it applies to, not just one
        caught += 1
    assert caught == len(names)


def test_loop_settings_halve_the_fp64_loss_on_the_banked_model(oracle):
    """model_grad_ref.LOOP's rate and step count on the two-bank mres / add model, Jacobi targets as in test_model_grad_cpu"""
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    m = K.loop_model()
    U_bc = UDiv.copy()
    oracle.setWallBcsForward(U_bc, flags)
    div = np.zeros_like(flags)
    oracle.velocityDivergenceForward(U_bc, flags, div)
    pT = np.zeros_like(flags)
    oracle.solveLinearSystemJacobi(pT, flags, div, False, 0, L["jacobi_iters"])
    UT = U_bc.copy()
    oracle.velocityUpdateForward(UT, flags, pT)
    oracle.setWallBcsForward(UT, flags)
    losses, _ = K.train_loop(m, m.layers, pDiv, U_bc, flags, pT, UT, L["lambdas"], L["lr"], L["steps"])
    print("fp64 loop, banked: loss %.4e -> %.4e over %d steps" % (losses[0], losses[-1], L["steps"]))
    assert losses[-1] <= 0.5 * losses[0]
