"""GPU checks of the training side of the projection ConvNet (tfl_model_set_weights, tfl_model_forward_train,
tfl_model_backward, fluidnet_amd.ProjectionNet) against the fp64 restatement of tests/model_grad_ref.py, which
tests/test_model_grad_cpu.py validates first.

Figures measured on an MI355X (worst per-tensor rel-L2 against fp64 over all 18 cases and the three gradient modes, and the
witness ratio = our error over PyTorch-CPU-fp32's): see profiles/model_backward.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import model_grad_ref as R
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _net(name, train=True):
    from fluidnet_amd import ProjectionNet
    _, kind, is3D, opts, _ = R.case(name)
    net = ProjectionNet(R.make_model(kind, is3D, opts), device=DEV)
    return net.train(train)


def _inputs(name):
    return [_up(a) for a in R.make_inputs(name)]


def _host(gw, gb):
    return [(w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)) for w, b in zip(gw, gb)]


@pytest.mark.parametrize("name", R.NAMES)
def test_parameter_gradients_against_fp64(name, monkeypatch):
    """every parameter tensor within 1e-5 rel-L2 of the fp64 gradients, for gradP + gradU, gradP alone and gradU alone"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, _, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in R.GRAD_MODES:
        want, fp32, zero_l1 = R.expected(name, mode)
        gw, gb = net.backward(flags, None if mode == "u-only" else gP, None if mode == "p-only" else gU, tape)
        rel = R.rel_l2_per_tensor(_host(gw, gb), want, zero_l1)
        ours = max(max(r) for r in rel)
        theirs = max(max(r) for r in R.rel_l2_per_tensor(fp32, want, zero_l1))
        print("grad witness %s %s: ours %.3e, PyTorch fp32 %.3e, ratio %.2f" % (name, mode, ours, theirs, ours / max(theirs, 1e-300)))
        for l, (ew, eb) in enumerate(rel):
            assert ew <= R.BAR and eb <= R.BAR, (mode, l, ew, eb)


@pytest.mark.parametrize("name", R.NAMES)
def test_forward_train_is_the_direct_forward_bit_for_bit(name, monkeypatch):
    """whatever inference path the model is on (the default topologies: their MFMA kernels), forward_train's outputs are those
    of tfl_model_forward of the same model created under TFL_CONV_PATH=direct"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name)
    pDiv, UDiv, flags, _, _ = _inputs(name)
    p, U, _ = net.forward_train(pDiv, UDiv, flags)          # (the native model is created here: the switch is read at creation)
    monkeypatch.setenv("TFL_CONV_PATH", "direct")
    _, kind, is3D, opts, _ = R.case(name)
    p0, U0 = R.make_model(kind, is3D, opts).forward([pDiv, UDiv, flags])
    assert torch.equal(p, p0) and torch.equal(U, U0)


@pytest.mark.parametrize("name", ["default3d-b", "default2d-c", "k5-skip3d", "sigmoid"])
def test_backward_is_deterministic_and_accumulates_exactly(name, monkeypatch):
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, _, tape = net.forward_train(pDiv, UDiv, flags)
    a = net.backward(flags, gP, gU, tape)
    b = net.backward(flags, gP, gU, tape)
    # unrelated work on the stream in between: a matrix product and a forward of another model through the shared scratch
    x = torch.randn(512, 512, device=DEV)
    (x @ x).sum()
    _net("default2d-a").forward_train(*_inputs("default2d-a")[:3])
    c = net.backward(flags, gP, gU, tape)
    for other in (b, c):
        for fresh, again in zip(a[0] + a[1], other[0] + other[1]):
            assert torch.equal(fresh, again)
    # accumulate = 1 onto random buffers: old + fresh, one fp32 add per element
    rng = torch.Generator(device=DEV).manual_seed(5)
    old = [torch.randn(t.shape, device=DEV, generator=rng) for t in a[0] + a[1]]
    acc = [t.clone() for t in old]
    n = len(a[0])
    net.backward(flags, gP, gU, tape, out=(acc[:n], acc[n:]), accumulate=True)
    for o, fresh, got in zip(old, a[0] + a[1], acc):
        assert torch.equal(got, o + fresh)


@pytest.mark.parametrize("is3D,dims", [(True, (16, 24, 32)), (False, (1, 64, 96))])
def test_set_weights_equals_a_fresh_model_on_the_inference_path(is3D, dims, monkeypatch):
    """3-D default (conv_mfma16) and 2-D default (conv2d_mfma): new parameters pushed into an existing native model give the
    bits of a model created from them"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    from fluidnet_amd import ProjectionNet
    sc = scenes.make_scene(dims, seed=21, B=1, vel_cells=1.0)
    pDiv, UDiv, flags = _up(sc["p"]), _up(sc["U"]), _up(sc["flags"])
    net = ProjectionNet(R.make_model("default", is3D, seed=3), device=DEV).eval()
    before = net(pDiv, UDiv, flags)
    fresh = R.make_model("default", is3D, seed=11)
    with torch.no_grad():
        for (w, b), pw, pb in zip(fresh.layers, net.weights, net.biases):
            pw.copy_(_up(w))
            pb.copy_(_up(b))
    after = net(pDiv, UDiv, flags)                       # (the version counters moved: pushed by itself)
    want = fresh.forward([pDiv, UDiv, flags])
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert not torch.equal(before[0], after[0])


def test_simulate_takes_the_module_where_it_takes_a_model(monkeypatch):
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    import bench
    from fluidnet_amd import FluidNetModel, ProjectionNet
    from fluidnet_amd.simulate import simulate
    dev = torch.device(DEV)
    a, mconf = bench.build_scene(24, 24, None, dev)
    b, _ = bench.build_scene(24, 24, None, dev)
    net = ProjectionNet(FluidNetModel.default_3d(seed=1), device=DEV).eval()
    plain = FluidNetModel.default_3d(seed=1)
    for _ in range(2):
        simulate(None, mconf, a, net)
        simulate(None, mconf, b, plain)
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(a[k], b[k]), k


def test_backward_after_a_push_is_refused():
    """a backward whose forward ran on weights the native model no longer holds raises instead of mixing the two sets"""
    from fluidnet_amd import TfluidsError
    net = _net("default2d-a")
    pDiv, UDiv, flags, gP, gU = _inputs("default2d-a")
    p, U = net(pDiv, UDiv, flags)
    loss = (p * gP).sum() + (U * gU).sum()
    with torch.no_grad():
        net.weights[0].mul_(1.5)
    net(pDiv, UDiv, flags)                   # (the version moved: this forward pushes)
    with pytest.raises(TfluidsError, match="pushed to the native model"):
        loss.backward()
    p, U = net(pDiv, UDiv, flags)
    ((p * gP).sum() + (U * gU).sum()).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in net.parameters())


def _raw(net, flags):
    from fluidnet_amd import tfluids
    lib, ctx, h, work = net.net._prep(flags)
    return tfluids, lib, ctx, h, work


def test_refusals_name_the_reason_and_write_nothing():
    from fluidnet_amd import FluidNetModel, ProjectionNet, TfluidsError
    name = "default2d-a"
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    B, _, Z, Y, X = flags.shape
    # models without a training pass: refused before anything is written
    for model, why in ((FluidNetModel.from_mconf(dict(addBatchNorm=True), False, seed=3), "graph models"),
                       (FluidNetModel.tog(False, seed=3), "pooling or ConvolutionUpsample")):
        net = ProjectionNet(model, device=DEV).train()
        sc = scenes.make_scene((1, 16, 32), seed=2, B=1)
        f2, U2, p2 = _up(sc["flags"]), _up(sc["U"]), _up(sc["p"])
        tfl, lib, ctx, h, work = _raw(net, f2)
        assert lib.tfl_model_tape_floats(h, 1, 1, 16, 32) == -1 and lib.tfl_model_backward_workspace_floats(h, 1, 1, 16, 32) == -1
        pO, UO = torch.full_like(p2, 7.0), torch.full_like(U2, 7.0)
        tape = torch.full((1 << 16,), 7.0, device=DEV)
        rc = lib.tfl_model_forward_train(ctx, h, tfl._tt(p2), tfl._tt(U2), tfl._tt(f2), tfl._tt(pO), tfl._tt(UO),
                                         ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(tape.data_ptr()), tape.numel())
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
        gw = [torch.full_like(w, 7.0) for w in net.weights]
        gb = [torch.full_like(b, 7.0) for b in net.biases]
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        rc = lib.tfl_model_backward(ctx, h, tfl._tt(f2), tfl._tt(p2), tfl._tt(U2), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                    ctypes.c_void_p(tape.data_ptr()), tape.numel(), arr(gw), arr(gb), 0)
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
        torch.cuda.synchronize()
        for t in [pO, UO, tape] + gw + gb:
            assert bool((t == 7.0).all())
        with pytest.raises(TfluidsError, match=why):
            net(p2, U2, f2)
    # a short tape / a short workspace
    net = _net(name)
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
    for tp, tn, wn, why in ((good, nt - 1, nw, "tape too small"), (good, nt, nw - 1, "workspace too small")):
        rc = lib.tfl_model_backward(ctx, h, tfl._tt(flags), tfl._tt(gP), tfl._tt(gU), ctypes.c_void_p(tp.data_ptr()), tn,
                                    ctypes.c_void_p(ws.data_ptr()), wn, arr(gw), arr(gb), 0)
        assert rc != 0 and why in lib.tfl_last_error(ctx).decode()
    torch.cuda.synchronize()
    for t in [pO, UO, tape, ws] + gw + gb:
        assert bool((t == 7.0).all())
    # an input that asks for a gradient
    with pytest.raises(TfluidsError, match="input gradients are not built"):
        net(pDiv, UDiv.clone().requires_grad_(True), flags)


def test_the_loop_closes():
    """ProjectionNet + FluidCriterion + torch.optim.SGD on the 2-D 32 x 32, B = 2 scene with Jacobi targets (calcPUTargets), at
    the learning rate and step count the CPU test holds to halve the fp64 loss: the loss falls, and after the first step the
    parameters are the restatement's to the 1e-5 bar"""
    from fluidnet_amd import FluidCriterion, ProjectionNet, calcPUTargets
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    model = R.loop_model()
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
            first = [(w.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64))
                     for w, b in zip(net.weights, net.biases)]
    print("GPU loop: loss %.4e -> %.4e over %d steps" % (losses[0], losses[-1], L["steps"]))
    assert losses[-1] < losses[0]
    _, hist = R.train_loop(start, model.opts, pDiv, batch["UDiv"].cpu().numpy(), flags, batch["pTarget"].cpu().numpy(),
                           batch["UTarget"].cpu().numpy(), L["lambdas"], L["lr"], 1)
    for l, ((gw, gb), (ww, wb)) in enumerate(zip(first, hist[0])):
        assert scenes.rel_l2(gw, ww) <= R.BAR and scenes.rel_l2(gb, wb) <= R.BAR, l
