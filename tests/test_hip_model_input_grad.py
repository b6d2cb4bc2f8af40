"""GPU checks of the projection ConvNet's input gradients (tfl_model_backward_input, ProjectionNet(input_grad=True)) against the
float64 restatement of tests/model_input_grad_ref.py, which tests/test_model_input_grad_cpu.py validates first.

Figures measured on an MI355X (worst rel-L2 against float64 per gradient mode over all 18 cases, and the witness ratio = our
error over PyTorch-CPU-fp32's): see profiles/model_input_grad.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import model_grad_ref as R
import model_input_grad_ref as I
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _net(name, input_grad=False):
    from fluidnet_amd import ProjectionNet
    kind, is3D, opts = I.spec(name)
    return ProjectionNet(R.make_model(kind, is3D, opts), device=DEV, input_grad=input_grad).train()


def _inputs(name):
    return [_up(a) for a in I.make_inputs(name)]


def _mode(mode, gP, gU):
    return (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", I.NAMES)
def test_input_gradients_against_fp64(name, monkeypatch):
    """gradPDiv and gradUDiv each within 1e-5 plain rel-L2 of float64, for gradP + gradU, gradP alone and gradU alone: the 18 cases
    of model_grad_ref, and two where the backward recomputes the divergence (model_input_grad_ref.EXTRA)"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in R.GRAD_MODES:
        want = I.input_grads(name, mode)
        fp32 = I.input_grads(name, mode, torch.float32)
        a, b = _mode(mode, gP, gU)
        _, _, gp, gu = net.backward_input(flags, pDiv, UDiv, U, a, b, tape)
        ours = [I.rel_l2(_np(gp), want[0]), I.rel_l2(_np(gu), want[1])]
        theirs = [I.rel_l2(fp32[0], want[0]), I.rel_l2(fp32[1], want[1])]
        print("input-grad witness %s %s: gradPDiv ours %.3e PyTorch fp32 %.3e, gradUDiv ours %.3e PyTorch fp32 %.3e, ratio %.2f"
              % (name, mode, ours[0], theirs[0], ours[1], theirs[1], max(ours) / max(max(theirs), 1e-300)))
        assert ours[0] <= R.BAR and ours[1] <= R.BAR, (mode, ours)
        if name == "udiv-without-pdiv":      # neither the pDiv channel, nor the skip, nor a pDiv normaliser
            assert not bool(gp.view(torch.int32).any())
        # the parameter gradients may be left out, and either input gradient: what is built does not change
        _, _, gp2, none = net.backward_input(flags, pDiv, UDiv, U, a, b, tape, want=(True, False), params=False)
        _, _, none2, gu2 = net.backward_input(flags, pDiv, UDiv, U, a, b, tape, want=(False, True), params=False)
        assert none is None and none2 is None and torch.equal(gp2, gp) and torch.equal(gu2, gu)


@pytest.mark.parametrize("name", ["default3d-b", "default2d-c", "k5-skip3d", "sigmoid"])
def test_parameter_gradients_are_tfl_model_backwards_bits_and_calls_repeat(name, monkeypatch):
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    ref = net.backward(flags, gP, gU, tape)
    a = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    b = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    # unrelated work on the stream in between: a matrix product and a forward of another model through the shared scratch
    x = torch.randn(512, 512, device=DEV)
    (x @ x).sum()
    _net("default2d-a").forward_train(*_inputs("default2d-a")[:3])
    c = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    for fresh, want in zip(a[0] + a[1], ref[0] + ref[1]):
        assert torch.equal(fresh, want)
    for other in (b, c):
        for fresh, again in zip(a[0] + a[1] + [a[2], a[3]], other[0] + other[1] + [other[2], other[3]]):
            assert torch.equal(fresh, again)
    # accumulate = 1 onto random buffers: the same bits as tfl_model_backward's accumulate
    rng = torch.Generator(device=DEV).manual_seed(5)
    old = [torch.randn(t.shape, device=DEV, generator=rng) for t in ref[0] + ref[1]]
    n = len(ref[0])
    acc0, acc1 = [t.clone() for t in old], [t.clone() for t in old]
    net.backward(flags, gP, gU, tape, out=(acc0[:n], acc0[n:]), accumulate=True)
    _, _, gp, gu = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape, out=(acc1[:n], acc1[n:]), accumulate=True)
    for o, x0, x1 in zip(old, acc0, acc1):
        assert torch.equal(x0, x1) and not torch.equal(x1, o)
    assert torch.equal(gp, a[2]) and torch.equal(gu, a[3])


def _fresh_from(net):
    """a new ProjectionNet built from the parameter values `net` holds now"""
    from fluidnet_amd import FluidNetModel, ProjectionNet
    layers = [(w.detach().cpu().numpy().copy(), b.detach().cpu().numpy().copy()) for w, b in zip(net.weights, net.biases)]
    return ProjectionNet(FluidNetModel(layers, net.net.is3D, opts=net.net.opts), device=DEV, input_grad=True).train()


@pytest.mark.parametrize("stepper", ["fused-adam", "torch-sgd"])
@pytest.mark.parametrize("name", ["k5-skip2d", "udiv-with-pdiv"])
def test_input_gradients_after_an_optimiser_step_are_a_fresh_models(name, stepper, monkeypatch):
    """both new weight forms (the first layer's data-gradient form, the skip channel's) are rows of the device refresh: after a
    step that pushes on the device, the input gradients are bit for bit those of a net created from the new values"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    import fluidnet_amd.optim
    net = _net(name, input_grad=True)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    before = [w.detach().clone() for w in net.weights]
    p, U = net(pDiv, UDiv, flags)
    ((p * gP).sum() + (U * gU).sum()).backward()
    opt = fluidnet_amd.optim.Adam(net, learningRate=0.05) if stepper == "fused-adam" else torch.optim.SGD(net.parameters(), lr=1e-4)
    opt.step()
    _, U1, tape = net.forward_train(pDiv, UDiv, flags)       # (torch.optim moved the version counters: pushed on the device here)
    assert all(not torch.equal(w, w0) for w, w0 in zip(net.weights, before))
    got = net.backward_input(flags, pDiv, UDiv, U1, gP, gU, tape)
    fresh = _fresh_from(net)
    _, U2, tape2 = fresh.forward_train(pDiv, UDiv, flags)
    want = fresh.backward_input(flags, pDiv, UDiv, U2, gP, gU, tape2)
    assert torch.equal(U1, U2)
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    for a, b in zip(got[0] + got[1], want[0] + want[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", I.CHAIN_CASES)
def test_two_chained_passes_under_autograd(name, monkeypatch):
    """net(net(x)) with the loss on the second outputs: every parameter's .grad and both leaf inputs' within the bar of float64"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name, input_grad=True)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    pDiv.requires_grad_(True)
    UDiv.requires_grad_(True)
    p1, U1 = net(pDiv, UDiv, flags)
    p2, U2 = net(p1, U1, flags)
    ((p2 * gP).sum() + (U2 * gU).sum()).backward()
    want, want_in = I.chain_param_grads(name, 2)
    fp32, fp32_in = I.chain_param_grads(name, 2, torch.float32)
    got = [(_np(w.grad), _np(b.grad)) for w, b in zip(net.weights, net.biases)]
    rel = R.rel_l2_per_tensor(got, want)
    ein = [I.rel_l2(_np(pDiv.grad), want_in[0]), I.rel_l2(_np(UDiv.grad), want_in[1])]
    print("chain witness %s: parameters ours %.3e PyTorch fp32 %.3e, inputs ours %.3e PyTorch fp32 %.3e"
          % (name, max(max(r) for r in rel), R.worst(fp32, want), max(ein), I.worst(fp32_in, want_in)))
    for l, (ew, eb) in enumerate(rel):
        assert ew <= R.BAR and eb <= R.BAR, (l, ew, eb)
    assert max(ein) <= R.BAR, ein


def test_an_in_place_edit_of_a_saved_input_is_caught_by_autograd():
    net = _net("default2d-a", input_grad=True)
    pDiv, UDiv, flags, gP, gU = _inputs("default2d-a")
    UDiv.requires_grad_(True)
    p, U = net(pDiv, UDiv, flags)
    loss = (p * gP).sum() + (U * gU).sum()
    with torch.no_grad():
        UDiv.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def _raw(net, flags):
    from fluidnet_amd import tfluids
    lib, ctx, h, work = net.net._prep(flags)
    return tfluids, lib, ctx, h, work


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def test_refusals_name_the_reason_and_write_nothing():
    from fluidnet_amd import FluidNetModel, ProjectionNet, TfluidsError
    name = "default2d-a"
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    B, _, Z, Y, X = flags.shape
    # the default construction still says no, and so does flags with input_grad=True
    with pytest.raises(TfluidsError, match="input gradients are not built"):
        _net(name)(pDiv, UDiv.clone().requires_grad_(True), flags)
    with pytest.raises(TfluidsError, match="never for flags"):
        _net(name, input_grad=True)(pDiv, UDiv, flags.clone().requires_grad_(True))
    # models without a training pass: refused before anything is written
    for model, why in ((FluidNetModel.from_mconf(dict(addBatchNorm=True), False, seed=3), "graph models"),
                       (FluidNetModel.tog(False, seed=3), "pooling or ConvolutionUpsample")):
        net = ProjectionNet(model, device=DEV, input_grad=True).train()
        sc = scenes.make_scene((1, 16, 32), seed=2, B=1)
        f2, U2, p2 = _up(sc["flags"]), _up(sc["U"]), _up(sc["p"])
        tfl, lib, ctx, h, work = _raw(net, f2)
        assert lib.tfl_model_backward_input_workspace_floats(h, 1, 1, 16, 32) == -1
        tape = torch.full((1 << 16,), 7.0, device=DEV)
        ws = torch.full((1 << 16,), 7.0, device=DEV)
        gw = [torch.full_like(w, 7.0) for w in net.weights]
        gb = [torch.full_like(b, 7.0) for b in net.biases]
        gp, gu = torch.full_like(p2, 7.0), torch.full_like(U2, 7.0)
        rc = lib.tfl_model_backward_input(ctx, h, tfl._tt(f2), tfl._tt(p2), tfl._tt(U2), tfl._tt(U2), tfl._tt(p2), tfl._tt(U2),
                                          ctypes.c_void_p(tape.data_ptr()), tape.numel(), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                          _arr(gw), _arr(gb), 0, tfl._tt(gp), tfl._tt(gu))
        assert rc == -3 and why in lib.tfl_last_error(ctx).decode()          # TFL_EUNSUPPORTED
        torch.cuda.synchronize()
        for t in [tape, ws, gp, gu] + gw + gb:
            assert bool((t == 7.0).all())
    # a short tape / a short workspace
    net = _net(name)
    tfl, lib, ctx, h, work = _raw(net, flags)
    nt = lib.tfl_model_tape_floats(h, B, Z, Y, X)
    nw = lib.tfl_model_backward_input_workspace_floats(h, B, Z, Y, X)
    assert nt > 0 and nw > lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X)
    _, U, good = net.forward_train(pDiv, UDiv, flags)
    gw = [torch.full_like(w, 7.0) for w in net.weights]
    gb = [torch.full_like(b, 7.0) for b in net.biases]
    gp, gu = torch.full_like(pDiv, 7.0), torch.full_like(UDiv, 7.0)
    ws = torch.full((nw,), 7.0, device=DEV)
    for tn, wn, why in ((nt - 1, nw, "tape too small"), (nt, nw - 1, "workspace too small")):
        rc = lib.tfl_model_backward_input(ctx, h, tfl._tt(flags), tfl._tt(pDiv), tfl._tt(UDiv), tfl._tt(U), tfl._tt(gP), tfl._tt(gU),
                                          ctypes.c_void_p(good.data_ptr()), tn, ctypes.c_void_p(ws.data_ptr()), wn,
                                          _arr(gw), _arr(gb), 0, tfl._tt(gp), tfl._tt(gu))
        assert rc == -1 and why in lib.tfl_last_error(ctx).decode()          # TFL_EINVAL
    torch.cuda.synchronize()
    for t in [ws, gp, gu] + gw + gb:
        assert bool((t == 7.0).all())


def test_forward_train_and_backward_input_replay_from_a_graph(monkeypatch):
    """one capture of forward_train + backward_input replays to the eager bits: no host read, no synchronisation in either"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    name = "default2d-a"
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    eager = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, Ug, tape_g = net.forward_train(pDiv, UDiv, flags)
        got = net.backward_input(flags, pDiv, UDiv, Ug, gP, gU, tape_g)
    for t in got[0] + got[1] + [got[2], got[3]]:
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Ug, U)
    for a, b in zip(got[0] + got[1] + [got[2], got[3]], eager[0] + eager[1] + [eager[2], eager[3]]):
        assert torch.equal(a, b)
