"""GPU checks of the training pass of banked projection nets ('mres' and 'dilate' banks joined by 'concat' or 'add': DESIGN.md
3.18) -- tfl_model_forward_train / tfl_model_backward / tfl_model_backward_input on graph models, through
fluidnet_amd.ProjectionNet -- against the fp64 restatement of tests/model_bank_grad_ref.py, which
tests/test_model_bank_grad_cpu.py validates first.

Figures measured on an MI355X (worst per-tensor rel-L2 against fp64 and the witness ratio = our error over PyTorch-CPU-fp32's):
see profiles/model_bank_backward.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import model_bank_grad_ref as K
import model_grad_ref as R
import model_input_grad_ref as I
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _net(name, input_grad=False, seed=3):
    from fluidnet_amd import ProjectionNet
    return ProjectionNet(K.make_model(name, seed=seed), device=DEV, input_grad=input_grad).train()


def _inputs(name):
    return [_up(a) for a in K.make_inputs(name)]


def _host(gw, gb):
    return [(w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)) for w, b in zip(gw, gb)]


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _mode(mode, gP, gU):
    return (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


@pytest.mark.parametrize("name", K.NAMES)
def test_parameter_gradients_against_fp64(name):
    """every parameter tensor within 1e-5 rel-L2 of the fp64 gradients, for gradP + gradU, gradP alone and gradU alone"""
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, _, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in K.GRAD_MODES:
        want, fp32, zero_l1, _, _ = K.expected(name, mode)
        a, b = _mode(mode, gP, gU)
        gw, gb = net.backward(flags, a, b, tape)
        rel = K.rel_l2_per_tensor(_host(gw, gb), want, zero_l1)
        ours = max(max(r) for r in rel)
        theirs = max(max(r) for r in K.rel_l2_per_tensor(fp32, want, zero_l1))
        print("bank grad witness %s %s: ours %.3e, PyTorch fp32 %.3e, ratio %.2f" % (name, mode, ours, theirs, ours / max(theirs, 1e-300)))
        for l, (ew, eb) in enumerate(rel):
            assert ew <= K.BAR and eb <= K.BAR, (mode, l, ew, eb)


@pytest.mark.parametrize("name", K.NAMES)
def test_input_gradients_against_fp64(name):
    """gradPDiv and gradUDiv each within 1e-5 plain rel-L2 of fp64 in the three gradient modes; the parameter gradients that come
    with them are tfl_model_backward's bits, and leaving them out changes neither input gradient"""
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in K.GRAD_MODES:
        _, _, _, want, fp32 = K.expected(name, mode)
        a, b = _mode(mode, gP, gU)
        gw, gb, gp, gu = net.backward_input(flags, pDiv, UDiv, U, a, b, tape)
        ours = [I.rel_l2(_np(gp), want[0]), I.rel_l2(_np(gu), want[1])]
        theirs = [I.rel_l2(fp32[0], want[0]), I.rel_l2(fp32[1], want[1])]
        print("bank input-grad witness %s %s: gradPDiv ours %.3e PyTorch fp32 %.3e, gradUDiv ours %.3e PyTorch fp32 %.3e, ratio %.2f"
              % (name, mode, ours[0], theirs[0], ours[1], theirs[1], max(ours) / max(max(theirs), 1e-300)))
        assert ours[0] <= K.BAR and ours[1] <= K.BAR, (mode, ours)
        ref = net.backward(flags, a, b, tape)
        for x, y in zip(ref[0] + ref[1], gw + gb):
            assert torch.equal(x, y)
        _, _, gp2, gu2 = net.backward_input(flags, pDiv, UDiv, U, a, b, tape, params=False)
        assert torch.equal(gp2, gp) and torch.equal(gu2, gu)


@pytest.mark.parametrize("name", K.NAMES)
def test_forward_train_is_the_inference_forward_bit_for_bit(name):
    net = _net(name)
    pDiv, UDiv, flags, _, _ = _inputs(name)
    p, U, _ = net.forward_train(pDiv, UDiv, flags)
    p0, U0 = K.make_model(name).forward([pDiv, UDiv, flags])
    assert torch.equal(p, p0) and torch.equal(U, U0)


@pytest.mark.parametrize("name", ["mres3-concat-3d", "mres3-add-split2-join4-2d", "dilate3-add-3d", "skip-dilate2-add-3d"])
def test_backward_is_deterministic_and_accumulates_exactly(name):
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    a = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    b = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    # unrelated work on the stream in between: a matrix product and a forward of another model through the shared scratch
    x = torch.randn(512, 512, device=DEV)
    (x @ x).sum()
    _net("dilate2-concat-2d").forward_train(*_inputs("dilate2-concat-2d")[:3])
    c = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    flat = lambda r: r[0] + r[1] + [r[2], r[3]]
    for other in (b, c):
        for fresh, again in zip(flat(a), flat(other)):
            assert torch.equal(fresh, again)
    # accumulate = 1 onto random buffers: old + fresh, one fp32 add per element
    rng = torch.Generator(device=DEV).manual_seed(5)
    old = [torch.randn(t.shape, device=DEV, generator=rng) for t in a[0] + a[1]]
    acc = [t.clone() for t in old]
    n = len(a[0])
    net.backward(flags, gP, gU, tape, out=(acc[:n], acc[n:]), accumulate=True)
    for o, fresh, got in zip(old, a[0] + a[1], acc):
        assert torch.equal(got, o + fresh)


@pytest.mark.parametrize("name", ["mres2-concat-2d", "dilate3-concat-3d", "skip-dilate2-add-3d", "udiv-mres2-concat-2d"])
def test_device_refresh_rebuilds_the_data_gradient_weights(name):
    """after tfl_model_set_weights_device with new values, forward_train + backward (parameter and input gradients) are those
    of a model created fresh from the new values, bit for bit"""
    net = _net(name, seed=3)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    net.forward_train(pDiv, UDiv, flags)               # (the native model exists, holding the seed-3 weights)
    fresh = K.make_model(name, seed=11)
    with torch.no_grad():
        for (w, b), pw, pb in zip(fresh.layers, net.weights, net.biases):
            pw.copy_(_up(w))
            pb.copy_(_up(b))
    p, U, tape = net.forward_train(pDiv, UDiv, flags)  # (the version counters moved: pushed on the device)
    got = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    other = _net(name, seed=11)
    p0, U0, tape0 = other.forward_train(pDiv, UDiv, flags)
    want = other.backward_input(flags, pDiv, UDiv, U0, gP, gU, tape0)
    assert torch.equal(p, p0) and torch.equal(U, U0)
    for x, y in zip(got[0] + got[1] + [got[2], got[3]], want[0] + want[1] + [want[2], want[3]]):
        assert torch.equal(x, y)


def test_the_loop_closes_on_a_banked_model():
    """ProjectionNet + FluidCriterion + torch.optim.SGD on model_grad_ref.LOOP's scene with a two-bank mres / add model: the loss
    falls, the parameters after the first step are the restatement's to the 1e-5 bar (what the linear loop test asks), and the
    loss after the 20 steps is the fp64 restatement's to 1e-3: per step the update carries the bar's 1e-5 relative error, 20
    steps of a descent that contracts errors add at most 20 of them, 2e-4, and the loss is a smooth function of the parameters
    with a relative sensitivity of order one here; 1e-3 leaves a factor five."""
    from fluidnet_amd import FluidCriterion, ProjectionNet, calcPUTargets
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    model = K.loop_model()
    start = [(w.copy(), b.copy()) for w, b in model.layers]
    batch = dict(pDiv=_up(pDiv), UDiv=_up(UDiv), flags=_up(flags), pTarget=_up(pDiv), UTarget=_up(UDiv))
    calcPUTargets(None, dict(trainTargetSource="jacobi", maxIter=L["jacobi_iters"]), batch)
    net = ProjectionNet(model, device=DEV).train()
    crit = FluidCriterion(*L["lambdas"])
    opt = torch.optim.SGD(net.parameters(), lr=L["lr"])
    losses, first = [], None
    for step in range(L["steps"] + 1):
        opt.zero_grad()
        p, U = net(batch["pDiv"], batch["UDiv"], batch["flags"])
        loss = crit((p, U), (batch["pTarget"], batch["UTarget"], batch["flags"]))
        losses.append(float(loss.detach()))
        if step == L["steps"]:
            break
        loss.backward()
        opt.step()
        if step == 0:
            first = _host([w.detach() for w in net.weights], [b.detach() for b in net.biases])
    ref_losses, hist = K.train_loop(model, start, pDiv, batch["UDiv"].cpu().numpy(), flags, batch["pTarget"].cpu().numpy(),
                                    batch["UTarget"].cpu().numpy(), L["lambdas"], L["lr"], L["steps"])
    print("GPU loop, banked: loss %.6e -> %.6e over %d steps; fp64 %.6e -> %.6e" % (losses[0], losses[-1], L["steps"], ref_losses[0], ref_losses[-1]))
    assert losses[-1] < losses[0]
    for l, ((gw, gb), (ww, wb)) in enumerate(zip(first, hist[0])):
        assert scenes.rel_l2(gw, ww) <= R.BAR and scenes.rel_l2(gb, wb) <= R.BAR, l
    assert abs(losses[-1] - ref_losses[-1]) <= 1e-3 * ref_losses[-1]


def _raw(net, flags):
    from fluidnet_amd import tfluids
    lib, ctx, h, work = net.net._prep(flags)
    return tfluids, lib, ctx, h, work


def test_untrainable_graph_models_are_still_refused_and_nothing_is_written():
    """batch norm, a max-pooled graph, a banked `tog` and the single-bank `tog`: refused by name before anything is written, the
    three size queries answer -1"""
    from fluidnet_amd import FluidNetModel, ProjectionNet, TfluidsError
    models = ((FluidNetModel.from_mconf(dict(addBatchNorm=True), False, seed=3), "graph models"),
              (FluidNetModel.from_mconf(dict(banksNum=2, banksType="dilate", addBatchNorm=True), False, seed=3), "graph models"),
              (FluidNetModel.from_mconf(dict(modelType="tog", poolType="max"), False, seed=3), "graph models"),
              (FluidNetModel.from_mconf(dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5), False, seed=3), "graph models"),
              (FluidNetModel.tog(False, seed=3), "pooling or ConvolutionUpsample"))
    for model, why in models:
        net = ProjectionNet(model, device=DEV).train()
        sc = scenes.make_scene((1, 16, 32), seed=2, B=1)
        f2, U2, p2 = _up(sc["flags"]), _up(sc["U"]), _up(sc["p"])
        tfl, lib, ctx, h, work = _raw(net, f2)
        assert lib.tfl_model_tape_floats(h, 1, 1, 16, 32) == -1
        assert lib.tfl_model_backward_workspace_floats(h, 1, 1, 16, 32) == -1
        assert lib.tfl_model_backward_input_workspace_floats(h, 1, 1, 16, 32) == -1
        pO, UO = torch.full_like(p2, 7.0), torch.full_like(U2, 7.0)
        tape = torch.full((1 << 16,), 7.0, device=DEV)
        rc = lib.tfl_model_forward_train(ctx, h, tfl._tt(p2), tfl._tt(U2), tfl._tt(f2), tfl._tt(pO), tfl._tt(UO),
                                         ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(tape.data_ptr()), tape.numel())
        err = lib.tfl_last_error(ctx).decode()
        assert rc != 0 and why in err and "no training pass" in err
        gw = [torch.full_like(w, 7.0) for w in net.weights]
        gb = [torch.full_like(b, 7.0) for b in net.biases]
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        rc = lib.tfl_model_backward(ctx, h, tfl._tt(f2), tfl._tt(p2), tfl._tt(U2), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                    ctypes.c_void_p(tape.data_ptr()), tape.numel(), arr(gw), arr(gb), 0)
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
        gp, gu = torch.full_like(p2, 7.0), torch.full_like(U2, 7.0)
        rc = lib.tfl_model_backward_input(ctx, h, tfl._tt(f2), tfl._tt(p2), tfl._tt(U2), tfl._tt(U2), tfl._tt(p2), tfl._tt(U2),
                                          ctypes.c_void_p(tape.data_ptr()), tape.numel(), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                          arr(gw), arr(gb), 0, tfl._tt(gp), tfl._tt(gu))
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
        torch.cuda.synchronize()
        for t in [pO, UO, tape, gp, gu] + gw + gb:
            assert bool((t == 7.0).all())
        with pytest.raises(TfluidsError, match=why):
            net(p2, U2, f2)


def test_short_tape_and_short_workspace_are_refused_exactly():
    """the size queries are exact: one float less of either is refused before anything is written"""
    name = "mres3-concat-3d"
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    B, _, Z, Y, X = flags.shape
    tfl, lib, ctx, h, work = _raw(net, flags)
    nt = lib.tfl_model_tape_floats(h, B, Z, Y, X)
    nw = lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X)
    assert nt > 0 and nw > 0
    _, _, good = net.forward_train(pDiv, UDiv, flags)
    pO, UO = torch.full_like(pDiv, 7.0), torch.full_like(UDiv, 7.0)
    tape = torch.full((nt,), 7.0, device=DEV)
    rc = lib.tfl_model_forward_train(ctx, h, tfl._tt(pDiv), tfl._tt(UDiv), tfl._tt(flags), tfl._tt(pO), tfl._tt(UO),
                                     ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(tape.data_ptr()), nt - 1)
    assert rc != 0 and "tape too small" in lib.tfl_last_error(ctx).decode()
    gw = [torch.full_like(w, 7.0) for w in net.weights]
    gb = [torch.full_like(b, 7.0) for b in net.biases]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ws = torch.full((nw,), 7.0, device=DEV)
    for tn, wn, why in ((nt - 1, nw, "tape too small"), (nt, nw - 1, "workspace too small")):
        rc = lib.tfl_model_backward(ctx, h, tfl._tt(flags), tfl._tt(gP), tfl._tt(gU), ctypes.c_void_p(good.data_ptr()), tn,
                                    ctypes.c_void_p(ws.data_ptr()), wn, arr(gw), arr(gb), 0)
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
    torch.cuda.synchronize()
    for t in [pO, UO, tape, ws] + gw + gb:
        assert bool((t == 7.0).all())
    # with exactly the sizes asked for, the pass runs and gives the bits of the call through ProjectionNet
    rc = lib.tfl_model_backward(ctx, h, tfl._tt(flags), tfl._tt(gP), tfl._tt(gU), ctypes.c_void_p(good.data_ptr()), nt,
                                ctypes.c_void_p(ws.data_ptr()), nw, arr(gw), arr(gb), 0)
    assert rc == 0, lib.tfl_last_error(ctx).decode()
    want = net.backward(flags, gP, gU, good)
    for x, y in zip(want[0] + want[1], gw + gb):
        assert torch.equal(x, y)
