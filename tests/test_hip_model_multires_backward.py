"""GPU checks of the training pass of linear models with pooling / upsampling layers -- `tog` and custom layer tables, switched on
by tfl_model_enable_multires_training / ProjectionNet(multires=True) -- against the fp64 restatement of
tests/model_multires_grad_ref.py, which tests/test_model_multires_grad_cpu.py validates first.

Figures measured on an MI355X (worst per-tensor rel-L2 against fp64 and the witness ratio = our error over PyTorch-CPU-fp32's):
see profiles/model_multires_backward.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import model_input_grad_ref as IR
import model_multires_grad_ref as M
import optim_ref as O
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _net(name, input_grad=False):
    from fluidnet_amd import ProjectionNet
    _, kind, is3D, _ = M.case(name)
    return ProjectionNet(M.make_model(kind, is3D), device=DEV, input_grad=input_grad, multires=True).train()


def _inputs(name):
    return [_up(a) for a in M.make_inputs(name)]


def _host(gw, gb):
    return [(w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)) for w, b in zip(gw, gb)]


def _mode(mode, gP, gU):
    return (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


@pytest.mark.parametrize("name", M.NAMES)
def test_parameter_gradients_against_fp64(name):
    """every parameter tensor within 1e-5 rel-L2 of the fp64 gradients, for gradP + gradU, gradP alone and gradU alone"""
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, _, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in M.GRAD_MODES:
        want, _, l1 = M.grads(name, mode)
        fp32, _, _ = M.grads(name, mode, torch.float32)
        gw, gb = net.backward(flags, *_mode(mode, gP, gU), tape)
        rel = M.rel_l2_per_tensor(name, mode, _host(gw, gb), want, l1)
        ours = max(max(r) for r in rel)
        theirs = M.worst(name, mode, fp32, want, l1)
        print("grad witness %s %s: ours %.3e, PyTorch fp32 %.3e, ratio %.2f" % (name, mode, ours, theirs, ours / max(theirs, 1e-300)))
        for l, (ew, eb) in enumerate(rel):
            assert ew <= M.BAR and eb <= M.BAR, (mode, l, ew, eb)


@pytest.mark.parametrize("name", M.NAMES)
def test_input_gradients_against_fp64(name):
    """gradPDiv and gradUDiv within the bar; the parameter gradients that come with them are tfl_model_backward's bits"""
    net = _net(name, input_grad=True)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, U, tape = net.forward_train(pDiv, UDiv, flags)
    for mode in M.GRAD_MODES:
        _, want, _ = M.grads(name, mode)
        _, fp32, _ = M.grads(name, mode, torch.float32)
        a, b = _mode(mode, gP, gU)
        gw, gb, gp, gu = net.backward_input(flags, pDiv, UDiv, U, a, b, tape)
        got = (gp.cpu().numpy(), gu.cpu().numpy())
        ours = [IR.rel_l2(g, w) for g, w in zip(got, want)]
        theirs = [IR.rel_l2(g, w) for g, w in zip(fp32, want)]
        print("input-grad witness %s %s: ours %.3e / %.3e, PyTorch fp32 %.3e / %.3e" % (name, mode, ours[0], ours[1], theirs[0], theirs[1]))
        assert ours[0] <= M.BAR and ours[1] <= M.BAR, (mode, ours)
        pw, pb = net.backward(flags, a, b, tape)
        assert all(torch.equal(x, y) for x, y in zip(gw + gb, pw + pb))
        only = net.backward_input(flags, pDiv, UDiv, U, a, b, tape, params=False)
        assert torch.equal(only[2], gp) and torch.equal(only[3], gu)


@pytest.mark.parametrize("name", M.NAMES)
def test_forward_train_is_the_inference_forward_bit_for_bit(name):
    net = _net(name)
    pDiv, UDiv, flags, _, _ = _inputs(name)
    p, U, _ = net.forward_train(pDiv, UDiv, flags)
    _, kind, is3D, _ = M.case(name)
    p0, U0 = M.make_model(kind, is3D).forward([pDiv, UDiv, flags])
    assert torch.equal(p, p0) and torch.equal(U, U0) and float(p.abs().max()) > 0


@pytest.mark.parametrize("name", ["tog3d-b", "tog2d-c", "custom2d-sigmoid", "custom3d-relu6"])
def test_backward_is_deterministic_and_accumulates_exactly(name):
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    _, _, tape = net.forward_train(pDiv, UDiv, flags)
    a = net.backward(flags, gP, gU, tape)
    b = net.backward(flags, gP, gU, tape)
    # unrelated work on the stream in between: a matrix product and a forward of another model through the shared scratch
    x = torch.randn(512, 512, device=DEV)
    (x @ x).sum()
    _net("tog2d-a").forward_train(*_inputs("tog2d-a")[:3])
    c = net.backward(flags, gP, gU, tape)
    for other in (b, c):
        for fresh, again in zip(a[0] + a[1], other[0] + other[1]):
            assert torch.equal(fresh, again)
    rng = torch.Generator(device=DEV).manual_seed(5)
    old = [torch.randn(t.shape, device=DEV, generator=rng) for t in a[0] + a[1]]
    acc = [t.clone() for t in old]
    n = len(a[0])
    net.backward(flags, gP, gU, tape, out=(acc[:n], acc[n:]), accumulate=True)
    for o, fresh, got in zip(old, a[0] + a[1], acc):
        assert torch.equal(got, o + fresh)


@pytest.mark.parametrize("name", ["tog3d-a", "tog2d-a", "custom2d-relu6", "custom3d-sigmoid"])
def test_refresh_equals_a_fresh_model(name):
    """new parameters copied into net.weights / net.biases: the next inference forward is a fresh model's, bit for bit, and so
    are forward_train and the backward (the data-gradient weights of every sub-position were rebuilt on the device)"""
    from fluidnet_amd import FluidNetModel, ProjectionNet
    net = _net(name, input_grad=True)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    net.forward_train(pDiv, UDiv, flags)               # (the native model exists, holding the old weights)
    rng = np.random.RandomState(21)
    new = [((w * rng.uniform(0.5, 1.5, w.shape)).astype(np.float32), (b + rng.randn(*b.shape) * 0.02).astype(np.float32))
           for w, b in net.net.layers]
    with torch.no_grad():
        for (w, b), pw, pb in zip(new, net.weights, net.biases):
            pw.copy_(_up(w))
            pb.copy_(_up(b))
    fresh = lambda: FluidNetModel(new, net.is3D, pool=net.net.pool, up=net.net.up, opts=net.net.opts)
    net.eval()
    p, U = net(pDiv, UDiv, flags)                      # (the version counters moved: pushed by itself)
    p0, U0 = fresh().forward([pDiv, UDiv, flags])
    assert torch.equal(p, p0) and torch.equal(U, U0)
    net.train()
    p, U, tape = net.forward_train(pDiv, UDiv, flags)
    got = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape)
    other = ProjectionNet(fresh(), device=DEV, input_grad=True, multires=True).train()
    p1, U1, tape1 = other.forward_train(pDiv, UDiv, flags)
    want = other.backward_input(flags, pDiv, UDiv, U1, gP, gU, tape1)
    assert torch.equal(p, p1) and torch.equal(U, U1)
    for x, y in zip(got[0] + got[1] + [got[2], got[3]], want[0] + want[1] + [want[2], want[3]]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("is3D", [False, True])
def test_one_fused_adam_step_against_the_fp64_restatement(is3D):
    """optim.Adam on the `tog` parameters: tests/test_hip_optim.py's check and bounds (optim_ref.check)"""
    from fluidnet_amd import FluidNetModel, ProjectionNet, optim
    cfg = O.config(O.ADAM, True)
    model = FluidNetModel.tog(is3D, seed=3)
    start = [np.array(t, np.float32) for wb in model.layers for t in wb]
    rng = np.random.RandomState(77)
    grads = [(rng.randn(*p.shape) * 0.05).astype(np.float32) for p in start]
    net = ProjectionNet(model, device=DEV, multires=True).train()
    opt = optim.Adam(net, **{k: cfg[k] for k in ("learningRate", "learningRateDecay", "beta1", "beta2", "epsilon", "weightDecay", "gradNormThreshold")})
    for l, (w, b) in enumerate(zip(net.weights, net.biases)):
        w.grad, b.grad = _up(grads[2 * l]), _up(grads[2 * l + 1])
    opt.step()
    m, v = opt.state()
    flat = lambda grad: [(t.grad if grad else t).detach().cpu().numpy() for wb in zip(net.weights, net.biases) for t in wb]
    got = [(flat(False), flat(True), [t.cpu().numpy() for t in m], [t.cpu().numpy() for t in v])]
    want = []
    for dtype in (np.float64, np.float32):
        st = O.new_state(start, cfg, dtype)
        x, g = O.step(start, grads, st, cfg, dtype)
        want.append([(x, g, st["m"], st["v"])])
    wx, ws = O.check(got, want[0], start, True)
    fx, fs = O.check(want[1], want[0], start, True)
    print("tog %dD adam: worst error/bound ours %.3f (fp32 restatement %.3f); worst rel-L2 of m, v, g' ours %.2e (%.2e)" % (3 if is3D else 2, wx, fx, ws, fs))
    assert wx <= 1.0 and ws <= O.BAR
    # ... and the step refreshed the native model: the next forward is a fresh model's from the stepped parameters
    sc = scenes.make_scene((8, 8, 16) if is3D else (1, 16, 32), seed=2, B=1)
    pDiv, UDiv, flags = _up(sc["p"]), _up(sc["U"]), _up(sc["flags"])
    net.eval()
    p, U = net(pDiv, UDiv, flags)
    layers = [(w.detach().cpu().numpy(), b.detach().cpu().numpy()) for w, b in zip(net.weights, net.biases)]
    p0, U0 = FluidNetModel(layers, is3D, pool=model.pool, up=model.up).forward([pDiv, UDiv, flags])
    assert torch.equal(p, p0) and torch.equal(U, U0)


def test_three_closure_iterations_follow_the_fp64_series():
    """run_epoch.Closure (forward_train, fused criterion, backward, fused clipped Adam) on the 2-D `tog`, B = 2, 1 x 16 x 32: the
    loss behind three steps is the fp64 series' to 1e-3 (the figure of test_hip_model_bank_backward.py's loop: per step the update
    carries the bar's 1e-5, three steps add at most three of them, and the loss is a smooth function of the parameters) and
    below the first"""
    from fluidnet_amd import FluidCriterion, ProjectionNet, optim
    from fluidnet_amd.run_epoch import Closure
    L = M.LOOP
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0, gravityScale=0,
                 vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource="manta", maxIter=12,
                 lossPLambda=L["lambdas"][0], lossULambda=L["lambdas"][1], lossDivLambda=L["lambdas"][2], longTermDivLambda=0,
                 longTermDivNumSteps=None, longTermDivProbability=0, timeScaleSigma=1, optimizationMethod="adam",
                 gradNormThreshold=L["clip"], optimState=dict(L["adam"], bestPerf=float("inf")))
    net = ProjectionNet(M.loop_model(), device=DEV, multires=True).train()
    crit = FluidCriterion(*L["lambdas"])
    closure = Closure(net, crit, optim.from_mconf(net, mconf), None, mconf)
    batch = {k: _up(v) for k, v in M.loop_batch().items()}
    plan = dict(buoyancyScale=0, gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], dt=0.1, numFutureSteps=0)
    losses = []
    for step in range(L["steps"] + 1):
        closure(batch, plan, training=step < L["steps"])
        losses.append(float(closure.loss[3]))
    closure.check()
    want = M.loop_series()
    print("closure on tog 2-D: loss %s; fp64 %s" % (" ".join("%.6e" % v for v in losses), " ".join("%.6e" % v for v in want)))
    assert abs(losses[-1] - want[-1]) <= 1e-3 * want[-1]
    assert losses[-1] < losses[0]


def _raw(net, flags):
    from fluidnet_amd import tfluids
    lib, ctx, h, work = net.net._prep(flags)
    return tfluids, lib, ctx, h, work


def test_the_enable_call_refuses_graph_models_by_name_and_writes_nothing():
    """a banked `tog`, a max-pool `tog` and a batch-norm model: the call names the reason, the size queries stay -1, the three
    entries still refuse and buffers pre-filled with 7.0 stay 7.0; ProjectionNet(multires=True) raises the library's refusal"""
    from fluidnet_amd import FluidNetModel, ProjectionNet, TfluidsError
    makers = (lambda: FluidNetModel.from_mconf(dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5), False, seed=3),
              lambda: FluidNetModel.from_mconf(dict(modelType="tog", poolType="max"), False, seed=3),
              lambda: FluidNetModel.from_mconf(dict(addBatchNorm=True), False, seed=3))
    sc = scenes.make_scene((1, 16, 32), seed=2, B=1)
    f2, U2, p2 = _up(sc["flags"]), _up(sc["U"]), _up(sc["p"])
    for make in makers:
        net = ProjectionNet(make(), device=DEV).train()
        tfl, lib, ctx, h, work = _raw(net, f2)
        rc = lib.tfl_model_enable_multires_training(ctx, h)
        err = lib.tfl_last_error(ctx).decode()
        assert rc != 0 and "model_enable_multires_training" in err and "graph models" in err, err
        assert lib.tfl_model_tape_floats(h, 1, 1, 16, 32) == -1
        assert lib.tfl_model_backward_workspace_floats(h, 1, 1, 16, 32) == -1
        assert lib.tfl_model_backward_input_workspace_floats(h, 1, 1, 16, 32) == -1
        pO, UO = torch.full_like(p2, 7.0), torch.full_like(U2, 7.0)
        tape = torch.full((1 << 16,), 7.0, device=DEV)
        rc = lib.tfl_model_forward_train(ctx, h, tfl._tt(p2), tfl._tt(U2), tfl._tt(f2), tfl._tt(pO), tfl._tt(UO),
                                         ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(tape.data_ptr()), tape.numel())
        assert rc != 0 and "no training pass" in lib.tfl_last_error(ctx).decode()
        gw = [torch.full_like(w, 7.0) for w in net.weights]
        gb = [torch.full_like(b, 7.0) for b in net.biases]
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        rc = lib.tfl_model_backward(ctx, h, tfl._tt(f2), tfl._tt(p2), tfl._tt(U2), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                    ctypes.c_void_p(tape.data_ptr()), tape.numel(), arr(gw), arr(gb), 0)
        assert rc != 0 and "no training pass" in lib.tfl_last_error(ctx).decode()
        torch.cuda.synchronize()
        for t in [pO, UO, tape] + gw + gb:
            assert bool((t == 7.0).all())
        with pytest.raises(TfluidsError, match="graph models"):
            ProjectionNet(make(), device=DEV, multires=True).train()(p2, U2, f2)
    # a model that trains anyway: the option changes nothing
    import model_grad_ref as R
    a = ProjectionNet(R.make_model("default", False), device=DEV, multires=True).train()
    b = ProjectionNet(R.make_model("default", False), device=DEV).train()
    ta, tb = a.forward_train(p2, U2, f2), b.forward_train(p2, U2, f2)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    # ... and without the option the single-bank `tog` is refused as it always was
    plain = ProjectionNet(FluidNetModel.tog(False, seed=3), device=DEV).train()
    with pytest.raises(TfluidsError, match="pooling or ConvolutionUpsample"):
        plain(p2, U2, f2)
    # a grid the coarsest level does not divide, on an enabled model: refused before anything is written
    sc = scenes.make_scene((1, 9, 32), seed=2, B=1)
    net = ProjectionNet(FluidNetModel.tog(False, seed=3), device=DEV, multires=True).train()
    with pytest.raises(TfluidsError, match="not divisible"):
        net.forward_train(_up(sc["p"]), _up(sc["U"]), _up(sc["flags"]))


def test_short_tape_and_short_workspace_are_refused_exactly():
    """the size queries are exact on an enabled model: one float less of either is refused before anything is written"""
    name = "tog3d-a"
    net = _net(name)
    pDiv, UDiv, flags, gP, gU = _inputs(name)
    B, _, Z, Y, X = flags.shape
    tfl, lib, ctx, h, work = _raw(net, flags)
    nt = lib.tfl_model_tape_floats(h, B, Z, Y, X)
    nw = lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X)
    assert nt > 0 and nw > 0 and lib.tfl_model_backward_input_workspace_floats(h, B, Z, Y, X) > nw
    _, _, good = net.forward_train(pDiv, UDiv, flags)
    assert good.numel() == nt
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
    # the exact sizes are enough
    rc = lib.tfl_model_backward(ctx, h, tfl._tt(flags), tfl._tt(gP), tfl._tt(gU), ctypes.c_void_p(good.data_ptr()), nt,
                                ctypes.c_void_p(ws.data_ptr()), nw, arr(gw), arr(gb), 0)
    assert rc == 0
    want = net.backward(flags, gP, gU, good)
    assert all(torch.equal(x, y) for x, y in zip(gw + gb, want[0] + want[1]))


def test_fit_trains_tog_on_a_generated_set_and_resumes_to_the_same_bits(tmp_path):
    """fit() with modelType = 'tog' on a generated 2-D set (2 runs, 32 x 32, pcgPrecond = 'mg'): it opts in by itself, runs two
    epochs, and one epoch + resume + one epoch ends with the bits of the uninterrupted run"""
    import datagen_ref as G
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    from fluidnet_amd.train_loop import fit
    dims = (1, 32, 32)
    g = dict(G.gen_gconf(False, dims), pcgPrecond="mg")
    store = FrameStore(DEV, False, *dims, 12, 12)

    def mconf():
        return dict(modelType="tog", dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0,
                    gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource="manta",
                    maxIter=12, lossPLambda=0, lossULambda=1.0, lossDivLambda=1.0, longTermDivLambda=0, longTermDivNumSteps=None,
                    longTermDivProbability=0.5, timeScaleSigma=1, trainBuoyancyProb=0, trainBuoyancyScale=2.0, trainGravityProb=0,
                    trainGravityScale=1.0, trainVorticityConfinementProb=0, trainVorticityConfinementAmp=0.8,
                    optimizationMethod="adam", gradNormThreshold=1, epoch=0,
                    optimState=dict(bestPerf=float("inf"), learningRate=0.0025, weightDecay=0, learningRateDecay=0, epsilon=0.0001,
                                    beta1=0.9, beta2=0.999))

    def state(res):
        m, v = res["optimiser"].state()
        return [p.detach().clone() for p in res["net"].parameters()] + m + v

    try:
        tr = datagen.generate(g, "tr", G.GEN_RUNS, G.GEN_SEED, store=store, device=DEV)["data"]
        a, b = str(tmp_path / "straight" / "model"), str(tmp_path / "resumed" / "model")
        conf = lambda out, epochs: dict(modelDirname=out, maxEpochs=epochs, batchSize=4, seed=5, evaluateDuringTraining=False)
        straight = fit(conf(a, 2), mconf(), tr)
        assert straight["epochs"] == 2 and straight["net"].multires
        lines = open(a + "_log.txt").read().splitlines()
        assert len(lines) == 2 and all(np.isfinite(float(x)) for line in lines for x in line.split("\t"))
        first = fit(conf(b, 1), mconf(), tr)
        assert first["epochs"] == 1
        del first
        resumed = fit(conf(b, 2), None, tr, resume=b + "_lastEpoch.npz")
        assert resumed["epochs"] == 1 and resumed["mconf"]["epoch"] == 2 and resumed["net"].multires
        sa, sb = state(straight), state(resumed)
        assert resumed["optimiser"].steps == straight["optimiser"].steps == 6
        assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
        assert open(a + "_log.txt").read() == open(b + "_log.txt").read()
    finally:
        store.close()
