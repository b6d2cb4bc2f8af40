"""GPU checks of the device-side weight refresh (tfl_model_set_weights_device) and of the fused optimiser step (tfl_optim_*,
fluidnet_amd.optim): the refresh against a model created from the same values, bit for bit, on every conv path and model
kind; the step against the fp64 restatement of tests/optim_ref.py (validated by tests/test_optim_ref_cpu.py); determinism;
capture and replay; and the closed training loop.

The bound on an updated parameter tensor (optim_ref.within): |x - x64| <= 1e-5 |delta64| + 2^-24 |x64|. The witness figure
printed beside ours is the fp32 numpy restatement's error over the same bound.
"""
import numpy as np
import pytest
import torch

import model_grad_ref as R
import optim_ref as O
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS3, DIMS2 = (16, 24, 32), (1, 64, 96)


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


# ---- 1. refresh equals a fresh model --------------------------------------------------------------------------------------
def _graph_model():
    from fluidnet_amd import FluidNetModel
    mc = dict(banksNum=2, banksType="mres", banksAggregateMethod="concat", banksSplitStage=2, banksJoinStage=4,
              addBatchNorm=True, batchNormAffine=True)
    return FluidNetModel.from_mconf(mc, True, seed=5)


def _tog(is3D):
    from fluidnet_amd import FluidNetModel
    return FluidNetModel.tog(is3D, seed=2)


# (name, model factory, TFL_CONV_PATH or None, trains)
REFRESH = [
    ("default3d-mfma16", lambda: R.make_model("default", True), None, True),
    ("default3d-mfma", lambda: R.make_model("default", True), "mfma", True),
    ("default3d-winograd", lambda: R.make_model("default", True), "winograd", True),
    ("default3d-direct", lambda: R.make_model("default", True), "direct", True),
    ("default2d-mfma", lambda: R.make_model("default", False), None, True),
    ("default2d-direct", lambda: R.make_model("default", False), "direct", True),
    ("yang2d", lambda: R.make_model("yang", False), None, True),
    ("yang3d", lambda: R.make_model("yang", True), None, True),
    ("k5-skip3d", lambda: R.make_model("k5-skip", True), None, True),
    ("tog2d", lambda: _tog(False), None, False),
    ("tog3d", lambda: _tog(True), None, False),
    ("graph-concat-bn", _graph_model, None, False),
]
VARIANTS = ("random", "scaled37", "wide-span", "all-zero")


def _w1(layers, variant):
    """the new parameter values: random; W0 times 37 (every layer's fp16 exponent moves); random with layers 1 and 3 spanning
    2^-24 .. 1 of their maximum (both halves of the fp16 split pass through subnormals); random with those layers all zero"""
    rng = np.random.RandomState(11)
    if variant == "scaled37":
        return [(w * np.float32(37.0), b * np.float32(37.0)) for w, b in layers]
    out = [((rng.randn(*w.shape) * max(float(w.std()), 1e-3)).astype(np.float32), (rng.randn(*b.shape) * 0.01).astype(np.float32))
           for w, b in layers]
    if variant in ("wide-span", "all-zero"):
        for l in (1, 3):
            if l < len(out) - 1:
                w, b = out[l]
                if variant == "all-zero":
                    out[l] = (np.zeros_like(w), b)
                else:
                    span = np.ldexp(np.float32(1.0), -(np.arange(w.size) % 25)).astype(np.float32).reshape(w.shape)
                    out[l] = ((np.sign(w) * (0.5 + np.abs(np.tanh(w))) * span * np.float32(0.7)).astype(np.float32), b)
    return out


@pytest.fixture(scope="module")
def fields():
    out = {}
    for is3D, dims in ((True, DIMS3), (False, DIMS2)):
        sc = scenes.make_scene(dims, seed=21, B=1, vel_cells=1.0)
        rng = np.random.RandomState(5)
        out[is3D] = (_up(sc["p"]), _up(sc["U"]), _up(sc["flags"]),
                     _up((rng.randn(*sc["p"].shape) + 0.5).astype(np.float32)), _up(rng.randn(*sc["U"].shape).astype(np.float32)))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,make,path,trains", REFRESH, ids=[c[0] for c in REFRESH])
def test_device_refresh_equals_a_fresh_model(name, make, path, trains, variant, fields, monkeypatch):
    """a model created from W0 and refreshed on the device with W1 gives the bits of a model created from W1: the inference
    forward (the packed forms of the model's path) and, where the model trains, forward_train + backward (the data-gradient
    form)"""
    if path is None:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    else:
        monkeypatch.setenv("TFL_CONV_PATH", path)
    from fluidnet_amd import FluidNetModel, ProjectionNet
    m0 = make()
    pDiv, UDiv, flags, gP, gU = fields[m0.is3D]
    net = ProjectionNet(m0, device=DEV).eval()
    before = net(pDiv, UDiv, flags)
    handle = net.net._handles[0]
    new = _w1(m0.layers, variant)
    with torch.no_grad():
        for (w, b), pw, pb in zip(new, net.weights, net.biases):
            pw.copy_(_up(w))
            pb.copy_(_up(b))
    after = net(pDiv, UDiv, flags)                 # (the version counters moved: refreshed on the device by itself)
    assert net.net._handles[0] == handle and net._host_stale, "the refresh must go through the device path, into the same model"
    fresh = ProjectionNet(FluidNetModel(new, m0.is3D, pool=m0.pool, up=m0.up, opts=m0.opts, graph=m0.graph), device=DEV).eval()
    want = fresh(pDiv, UDiv, flags)
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    if variant == "random":
        assert not torch.equal(before[0], after[0])
    if not trains:
        return
    got_t, want_t = [], []
    for n, out in ((net, got_t), (fresh, want_t)):
        p, U, tape = n.forward_train(pDiv, UDiv, flags)
        gw, gb = n.backward(flags, gP, gU, tape)
        out.extend([p, U] + list(gw) + list(gb))
    for a, b in zip(got_t, want_t):
        assert torch.equal(a, b)
    # the host copy follows when something reads it
    for (w, b), (w1, b1) in zip(net.layers, new):
        assert np.array_equal(w, w1) and np.array_equal(b, b1)
    assert not net._host_stale


def test_refresh_on_the_fp16_path_is_refused_while_capturing(fields, monkeypatch):
    """the one exception: on the 3-D default model's split-fp16 path the refresh reads three floats back, so it says no --
    before launching anything -- while the stream captures; the capture stays valid and the weights stay as they were"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    from fluidnet_amd import ProjectionNet, TfluidsError
    pDiv, UDiv, flags, _, _ = fields[True]
    net = ProjectionNet(R.make_model("default", True), device=DEV).eval()
    want = net(pDiv, UDiv, flags)
    t = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.add_(1.0)
        with pytest.raises(TfluidsError, match="capturing"):
            net._push_device()
    got = net(pDiv, UDiv, flags)
    assert torch.equal(got[0], want[0])


# ---- 2. optimiser steps against fp64 -----------------------------------------------------------------------------------------
def _kind_model(kind):
    return R.make_model("yang" if kind == "yang" else "default", False, seed=3)


def _optimizer(net, cfg):
    from fluidnet_amd import optim
    if cfg["method"] == O.ADAM:
        return optim.Adam(net, **{k: cfg[k] for k in ("learningRate", "learningRateDecay", "beta1", "beta2", "epsilon", "weightDecay",
                                                       "gradNormThreshold")})
    return optim.RMSprop(net, **{k: cfg[k] for k in ("learningRate", "alpha", "epsilon", "weightDecay", "initialMean", "gradNormThreshold")})


def _set_grads(net, flat):
    """flat = [gw0, gb0, gw1, gb1, ...] (numpy) into the parameters' .grad, in place where they exist"""
    for l, (w, b) in enumerate(zip(net.weights, net.biases)):
        for p, g in ((w, flat[2 * l]), (b, flat[2 * l + 1])):
            if p.grad is None:
                p.grad = _up(g)
            else:
                p.grad.copy_(_up(g))


def _flat(net, grad=False):
    return [(t.grad if grad else t).detach().cpu().numpy() for wb in zip(net.weights, net.biases) for t in wb]


@pytest.mark.parametrize("kind,method,clip", O.CASES)
def test_steps_against_the_fp64_restatement(kind, method, clip):
    from fluidnet_amd import ProjectionNet
    cfg = O.config(method, clip)
    want = O.trajectory(kind, cfg, np.float64)
    witness = O.trajectory(kind, cfg, np.float32)
    net = ProjectionNet(_kind_model(kind), device=DEV).train()
    opt = _optimizer(net, cfg)
    got = []
    for s in range(O.STEPS):
        _set_grads(net, O.gradients(kind, s))
        opt.step()
        m, v = opt.state()
        got.append((_flat(net), _flat(net, grad=True), [t.cpu().numpy() for t in m], [t.cpu().numpy() for t in v] if v is not None else None))
    assert opt.steps == O.STEPS
    start = O.parameters(kind)
    wx, ws = O.check(got, want, start, method == O.ADAM)
    fx, fs = O.check(witness, want, start, method == O.ADAM)
    print("%s %s clip=%s: worst error/bound ours %.3f (fp32 restatement %.3f); worst rel-L2 of m, v, g' ours %.2e (%.2e)"
          % (kind, method, clip, wx, fx, ws, fs))
    assert wx <= 1.0 and ws <= O.BAR


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------
def _run_steps(kind, cfg, noise=False):
    from fluidnet_amd import ProjectionNet
    net = ProjectionNet(_kind_model(kind), device=DEV).train()
    opt = _optimizer(net, cfg)
    for s in range(2):
        _set_grads(net, O.gradients(kind, s))
        if noise:      # unrelated work on the stream in front of the step
            a = torch.randn(256, 256, device=DEV)
            (a @ a).sum().item()
            torch.empty(1 << 20, device=DEV).fill_(3.0)
        opt.step()
    m, v = opt.state()
    return [t.detach().clone() for t in net.parameters()] + [t.grad.clone() for t in net.parameters()] + m + (v or [])


@pytest.mark.parametrize("method", [O.ADAM, O.RMSPROP])
def test_same_bits_every_time(method):
    cfg = O.config(method, True)
    a, b, c = _run_steps("default2d", cfg), _run_steps("default2d", cfg), _run_steps("default2d", cfg, noise=True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---- 4. capture ---------------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_as_eager_steps(fields):
    """2-D default model: 3 eager steps against 1 captured step replayed 3 times -- parameters, state, step counter and
    forward outputs bit-equal. Captured on one stream (torch.cuda.graph, as GraphedSimulate does): a call that synchronised or
    read the host would fail the capture, and a counter advanced by the host would stand still on replay."""
    from fluidnet_amd import ProjectionNet
    pDiv, UDiv, flags, _, _ = fields[False]
    cfg = O.config(O.ADAM, True)
    src = [_up(g) for g in O.gradients("default2d", 0)]       # the step rewrites .grad (clip, decay): each step starts from these

    def load(net):
        for l, (w, b) in enumerate(zip(net.weights, net.biases)):
            w.grad.copy_(src[2 * l])
            b.grad.copy_(src[2 * l + 1])

    nets, opts = [], []
    for _ in range(2):
        net = ProjectionNet(_kind_model("default2d"), device=DEV).train()
        net(pDiv, UDiv, flags)                               # (the native model exists before the first step)
        _set_grads(net, O.gradients("default2d", 0))
        nets.append(net)
        opts.append(_optimizer(net, cfg))
    eager, graphed = nets
    for _ in range(3):
        load(eager)
        opts[0].step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        load(graphed)
        opts[1].step()
    assert opts[1].steps == 0                                # (captured, not run)
    for _ in range(3):
        g.replay()
    assert opts[0].steps == 3 and opts[1].steps == 3
    for a, b in zip(eager.parameters(), graphed.parameters()):
        assert torch.equal(a, b)
    for sa, sb in zip(opts[0].state(), opts[1].state()):
        for a, b in zip(sa, sb):
            assert torch.equal(a, b)
    with torch.no_grad():
        ea, gr = eager.eval()(pDiv, UDiv, flags), graphed.eval()(pDiv, UDiv, flags)
    assert torch.equal(ea[0], gr[0]) and torch.equal(ea[1], gr[1])
    assert eager._pushes == 3 and graphed._pushes == 1       # no second push: the step refreshed the native model itself


# ---- 5. the closed loop ---------------------------------------------------------------------------------------------------------
def test_the_loop_closes_with_the_fused_adam():
    """R.LOOP's scene with fluidnet_amd.optim.Adam as default_conf.lua configures it (optimState, gradNormThreshold = 1): the
    loss falls over its step count, and after the first step the parameters meet the bound against the fp64 restatement
    (gradient from the fp64 model, step from optim_ref)"""
    from fluidnet_amd import FluidCriterion, ProjectionNet, calcPUTargets, optim
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    model = R.loop_model()
    start = [(w.copy(), b.copy()) for w, b in model.layers]
    batch = dict(pDiv=_up(pDiv), UDiv=_up(UDiv), flags=_up(flags), pTarget=_up(pDiv), UTarget=_up(UDiv))
    calcPUTargets(None, dict(trainTargetSource="jacobi", maxIter=L["jacobi_iters"]), batch)
    net = ProjectionNet(model, device=DEV).train()
    crit = FluidCriterion(*L["lambdas"])
    mconf = dict(optimizationMethod="adam", gradNormThreshold=1,
                 optimState=dict(bestPerf=float("inf"), learningRate=0.0025, weightDecay=0, momentum=0.9, dampening=0,
                                 learningRateDecay=0, nesterov=False, epsilon=0.0001, beta1=0.9, beta2=0.999))
    opt = optim.from_mconf(net, mconf)
    losses, first = [], None
    for step in range(L["steps"] + 1):
        p, U = net(batch["pDiv"], batch["UDiv"], batch["flags"])
        loss = crit((p, U), (batch["pTarget"], batch["UTarget"], batch["flags"]))
        losses.append(float(loss.detach()))
        if step == L["steps"]:
            break
        loss.backward()
        opt.step()
        if step == 0:
            first = _flat(net)
        opt.zero_grad()
    print("GPU loop, fused Adam: loss %.4e -> %.4e over %d steps" % (losses[0], losses[-1], L["steps"]))
    assert losses[-1] < losses[0] and opt.steps == L["steps"]
    # the first step in fp64
    cur = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in start]
    pT, UT = batch["pTarget"].cpu().numpy(), batch["UTarget"].cpu().numpy()
    p, U, params = R.forward(cur, pDiv, batch["UDiv"].cpu().numpy(), flags, model.opts, torch.float64)
    loss = R.criterion_loss(p, U, pT, UT, flags, L["lambdas"])
    flat = [t for wb in params for t in wb]
    g64 = [t.numpy() for t in torch.autograd.grad(loss, flat)]
    cfg = dict(method=O.ADAM, gradNormThreshold=1.0, alpha=0.0, initialMean=0.0, **{k: float(mconf["optimState"][k]) for k in (
        "learningRate", "learningRateDecay", "beta1", "beta2", "epsilon", "weightDecay")})
    x0 = [t for wb in cur for t in wb]
    x64, _ = O.step(x0, g64, O.new_state(x0, cfg), cfg)
    worst = 0.0
    for a, b, p0 in zip(first, x64, x0):
        err, bound = O.within(a, b, p0)
        worst = max(worst, err / bound)
    print("first step: worst error/bound %.3f, gradient norm %.3f" % (worst, np.sqrt(sum((a ** 2).sum() for a in g64))))
    assert worst <= 1.0


# ---- 6. a native model on another device --------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU in the process")
def test_a_fused_step_reaches_the_native_model_on_another_device(fields):
    """the fused step refreshes the native model on the parameters' device; one on another device is dropped, as after a push,
    and re-created from the brought-up-to-date host copy: its forward equals the first device's, bit for bit"""
    from fluidnet_amd import ProjectionNet
    pDiv, UDiv, flags, _, _ = fields[False]
    other = [t.to("cuda:1") for t in (pDiv, UDiv, flags)]
    net = ProjectionNet(_kind_model("default2d"), device=DEV).eval()
    net(pDiv, UDiv, flags)
    old = net(*other)
    opt = _optimizer(net, O.config(O.ADAM, True))
    _set_grads(net, O.gradients("default2d", 0))
    opt.step()
    here, there = net(pDiv, UDiv, flags), net(*other)
    assert torch.equal(here[0].cpu(), there[0].cpu()) and torch.equal(here[1].cpu(), there[1].cpu())
    assert not torch.equal(old[0].cpu(), there[0].cpu())
