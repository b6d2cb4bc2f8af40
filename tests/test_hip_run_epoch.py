"""GPU checks of fluidnet_amd.run_epoch (the training closure of torch/lib/run_epoch.lua:133-330 as one call), of
simulate.dataAugmentation, and of the device pieces behind them: tfl_closure_fold and tfl_optim_step_guarded.

The yardstick of the closure is hand_iteration() below: the same batch sequenced call by call with the public pieces, written
from the Lua line numbers. Both sides run the same kernels on the same inputs, so every comparison is torch.equal; five
deliberate mistakes in the hand sequence (MUTANTS) show that the comparison sees them.
Grids: 2-D 1 x 16 x 32 and 3-D 8 x 8 x 32, B = 2, the seeded `default` nets of tests/model_grad_ref.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import model_grad_ref as R
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = {False: (1, 16, 32), True: (8, 8, 32)}
B = 2
MUTANTS = ("second-backward-overwrites", "lambdas-left-on-with-manta", "dt-not-scaled", "outputDiv-on-every-step",
           "rollout-before-the-first-pass")


def _up(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _mconf(source, lambdas=(1.0, 1.0, 1.0), **over):
    m = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0, gravityScale=0,
             vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource=source, maxIter=12,
             lossPLambda=lambdas[0], lossULambda=lambdas[1], lossDivLambda=lambdas[2],
             longTermDivLambda=1, longTermDivNumSteps=[4, 16], longTermDivProbability=0.9, timeScaleSigma=1,
             trainBuoyancyProb=0.5, trainBuoyancyScale=2.0, trainGravityProb=0.5, trainGravityScale=1.0,
             trainVorticityConfinementProb=0.5, trainVorticityConfinementAmp=0.8,
             optimizationMethod="adam", gradNormThreshold=1,
             optimState=dict(bestPerf=float("inf"), learningRate=0.0025, weightDecay=0, momentum=0.9, dampening=0,
                             learningRateDecay=0, nesterov=False, epsilon=0.0001, beta1=0.9, beta2=0.999))
    m.update(over)
    return m


def _plan(n, dt=0.1, buoy=0, grav=0, vort=0, gravity=(0.0, 1.0, 0.0)):
    return dict(buoyancyScale=buoy, gravityScale=grav, vorticityConfinementAmp=vort, gravity=list(gravity), dt=dt, numFutureSteps=n)


AUGMENTED = dict(buoy=2.0, grav=1.0, vort=0.8, gravity=(-1.0, 0.0, 0.0))


def _scene(is3D, seed=31):
    sc = scenes.make_scene(DIMS[is3D], seed=seed, B=B, vel_cells=0.6)
    sc["U"][1] *= 0.4
    return sc


def _batch(is3D, seed=31):
    """a mini-batch as data_binary.lua delivers it; the (manta) targets are a damped copy of the inputs"""
    sc = _scene(is3D, seed)
    return dict(pDiv=_up(sc["p"]), UDiv=_up(sc["U"]), flags=_up(sc["flags"]), densityDiv=_up(sc["density"]),
                pTarget=_up(sc["p"] * np.float32(0.5)), UTarget=_up(sc["U"] * np.float32(0.9)))


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


def _setup(is3D, mconf, errLimit=None, model=None):
    from fluidnet_amd import FluidCriterion, ProjectionNet, optim
    from fluidnet_amd.run_epoch import Closure
    net = ProjectionNet(model if model is not None else R.make_model("default", is3D), device=DEV).train()
    crit = FluidCriterion(mconf["lossPLambda"], mconf["lossULambda"], mconf["lossDivLambda"])
    opt = optim.from_mconf(net, mconf)
    kw = {} if errLimit is None else dict(errLimit=errLimit)
    return net, crit, opt, Closure(net, crit, opt, None, mconf, **kw)


def _grads(net):
    for p in net.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    return [p.grad for p in net.weights], [p.grad for p in net.biases]


def hand_iteration(net, crit, opt, mconf, batch, plan, sums, mutant=None):
    """one mini-batch of run_epoch.lua with existing public calls only; sums: float64 [5] on the device (p, u, div, total,
    long-term total). mutant: one of MUTANTS, a mistake made on purpose."""
    from fluidnet_amd import calcPUTargets, dataAugmentation, tfluids
    from fluidnet_amd.simulate import simulate_native
    m = dict(mconf)
    for k in ("buoyancyScale", "gravityScale", "vorticityConfinementAmp", "gravity"):      # :133-158
        m[k] = plan[k]
    manta = m["trainTargetSource"] == "manta"
    is3D = batch["UDiv"].size(1) == 3
    flags = batch["flags"]
    long_term = m["longTermDivNumSteps"] is not None and m["longTermDivLambda"] > 0      # :240
    n = plan["numFutureSteps"]

    def rollout():
        if mutant != "dt-not-scaled":
            m["dt"] = plan["dt"]                                                          # :243-250
        net.eval()                                                                        # :252
        state = dict(batch, density=batch["densityDiv"])                                  # simulate.lua:29
        for i in range(1, n + 1):                                                         # :262-265
            simulate_native(None, m, state, net, outputDiv=(i == n or mutant == "outputDiv-on-every-step"))
        net.train()                                                                       # :266

    def forward_criterion_backward(accumulate):
        p, U, tape = net.forward_train(batch["pDiv"], batch["UDiv"], flags)               # :207 / :269
        p.requires_grad_(True)
        U.requires_grad_(True)
        err = crit((p, U), (batch["pTarget"], batch["UTarget"], flags))                   # :209 / :286
        err.backward()                                                                    # :233 / :292
        net.backward(flags, p.grad, U.grad, tape, out=_grads(net), accumulate=accumulate)  # :234 / :293
        return err.detach()

    if not manta and (m["lossPLambda"] > 0 or m["lossULambda"] > 0):                      # :160-170
        dataAugmentation(None, m, batch)
        calcPUTargets(None, m, batch, net)
    if m["lossPLambda"] > 0:                                                              # :172-179
        tfluids.normalizePressureMean(batch["pTarget"], flags, is3D)
    if mutant == "rollout-before-the-first-pass" and long_term:
        rollout()
    _grads(net)
    opt.zero_grad()                                                                       # :203
    err = forward_criterion_backward(True)      # (Torch7's backward always accumulates)
    sums[3] += err                                                                        # :224-229
    sums[0] += crit.pLoss
    sums[1] += crit.uLoss
    sums[2] += crit.divLoss
    if long_term:
        if mutant != "rollout-before-the-first-pass":
            rollout()
        if manta:                                                                         # :273-284
            if mutant != "lambdas-left-on-with-manta":
                crit.pLambda = crit.uLambda = 0
        else:
            calcPUTargets(None, m, batch, net)
            tfluids.normalizePressureMean(batch["pTarget"], flags, is3D)
        crit.divLambda = m["longTermDivLambda"]                                           # :285
        err2 = forward_criterion_backward(mutant != "second-backward-overwrites")         # :286-293
        sums[4] += err2                                                                   # :287
        sums[3] += err2                                                                   # :291
        crit.pLambda, crit.uLambda, crit.divLambda = m["lossPLambda"], m["lossULambda"], m["lossDivLambda"]      # :296-298
    opt.step()                                                                            # :304-320 (the clip is the step's own)


def _state(net, opt, batch, sums):
    m, v = opt.state()
    out = [("param%d" % i, p.detach()) for i, p in enumerate(net.parameters())]
    out += [("m%d" % i, t) for i, t in enumerate(m)] + [("v%d" % i, t) for i, t in enumerate(v)]
    out += [(k, batch[k]) for k in ("pDiv", "UDiv", "densityDiv", "pTarget", "UTarget")]
    return out + [("sums", sums)]


def _differences(a, b):
    return [k for (k, x), (_, y) in zip(a, b) if not torch.equal(x, y)]


# (name, is3D, target source, lossDivLambda of the main pass, the three plans)
CASES = [
    ("2d-manta-n1", False, "manta", 1.0, [_plan(1, 0.05), _plan(1, 0.13), _plan(1)]),
    ("2d-jacobi-n4-augmented", False, "jacobi", 1.0, [_plan(4, 0.07, **AUGMENTED), _plan(1, 0.1), _plan(4, 0.03, vort=0.8)]),
    ("3d-manta-n4", True, "manta", 0.0, [_plan(4, 0.06), _plan(1, 0.1), _plan(4, 0.12)]),
    ("3d-jacobi-n1-augmented", True, "jacobi", 1.0, [_plan(1, 0.08, **AUGMENTED), _plan(4, 0.05, buoy=2.0, gravity=(0.0, 0.0, 1.0)), _plan(1, 0.1)]),
]


# ---- 1. the closure equals its parts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,is3D,source,lamD,plans", CASES, ids=[c[0] for c in CASES])
def test_the_closure_equals_the_hand_sequence(name, is3D, source, lamD, plans):
    mconf = _mconf(source, (1.0, 1.0, lamD))
    net_a, _, opt_a, closure = _setup(is3D, mconf)
    net_b, crit_b, opt_b, _ = _setup(is3D, mconf)
    sums_b = torch.zeros(5, dtype=torch.float64, device=DEV)
    for it, plan in enumerate(plans):
        fresh = _batch(is3D, seed=31 + it)
        ba, bb = _clone(fresh), _clone(fresh)
        closure(ba, plan)
        hand_iteration(net_b, crit_b, opt_b, mconf, bb, plan, sums_b)
        diff = _differences(_state(net_a, opt_a, ba, closure.sums), _state(net_b, opt_b, bb, sums_b))
        assert not diff, (name, it, diff)
        assert not torch.equal(ba["UDiv"], fresh["UDiv"])                    # (the rollout really moved the batch)
        assert float(closure.sums[4]) > 0 and int(closure.guard.item()) == 0
    assert opt_a.steps == len(plans) == opt_b.steps


# ---- 2. mutants are caught -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_mutated_hand_sequence_differs(mutant):
    """2-D, manta targets with all three lambdas on, four future steps at a scaled dt: each mistake changes what an iteration
    leaves behind"""
    mconf = _mconf("manta")
    plan = _plan(4, 0.04)
    net_a, _, opt_a, closure = _setup(False, mconf)
    net_b, crit_b, opt_b, _ = _setup(False, mconf)
    sums_b = torch.zeros(5, dtype=torch.float64, device=DEV)
    ba = _batch(False)
    bb = _clone(ba)
    closure(ba, plan)
    hand_iteration(net_b, crit_b, opt_b, mconf, bb, plan, sums_b, mutant=mutant)
    diff = _differences(_state(net_a, opt_a, ba, closure.sums), _state(net_b, opt_b, bb, sums_b))
    print(mutant, "->", diff)
    assert diff
    assert any(k.startswith("param") for k in diff) and any(k.startswith("m") for k in diff)


# ---- 3. state restore ----------------------------------------------------------------------------------------------------------
def test_lambdas_mconf_and_mode_are_restored():
    mconf = _mconf("manta")
    before = copy.deepcopy(mconf)
    net, crit, opt, closure = _setup(False, mconf)
    crit.pLambda, crit.uLambda, crit.divLambda = 0.5, 0.25, 2.0      # (the caller's own: not mconf's)
    net.eval()
    closure(_batch(False), _plan(1, 0.05, **AUGMENTED))
    assert (crit.pLambda, crit.uLambda, crit.divLambda) == (0.5, 0.25, 2.0)
    assert mconf == before and net.training is False
    from fluidnet_amd import TfluidsError
    bad = _batch(False)
    del bad["UTarget"]
    with pytest.raises(TfluidsError, match="UTarget"):
        closure(bad, _plan(1, 0.05, **AUGMENTED))
    assert (crit.pLambda, crit.uLambda, crit.divLambda) == (0.5, 0.25, 2.0)
    assert mconf == before and net.training is False
    net.train()
    with pytest.raises(TfluidsError, match="UTarget"):
        closure(bad, _plan(1), training=False)
    assert net.training is True and opt.steps == 1


# ---- 4. training = False -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
def test_evaluation_mode_scores_and_changes_nothing(is3D):
    mconf = _mconf("jacobi")
    net, crit, opt, closure = _setup(is3D, mconf)
    closure(_batch(is3D, seed=40), _plan(1))      # one real step first: the moments and the counter are not trivially zero
    params = [p.detach().clone() for p in net.parameters()]
    m0, v0 = opt.state()
    plan = _plan(4, 0.06, **AUGMENTED)
    fresh = _batch(is3D)
    be, bt = _clone(fresh), _clone(fresh)
    closure(be, plan, training=False)
    got = (closure.loss.clone(), closure.loss_long_term.clone())
    m1, v1 = opt.state()
    assert all(torch.equal(a, b.detach()) for a, b in zip(params, net.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(m0 + v0, m1 + v1)) and opt.steps == 1
    closure(bt, plan, training=True)
    assert torch.equal(got[0], closure.loss) and torch.equal(got[1], closure.loss_long_term)
    assert float(got[0][3]) > 0 and float(got[1][3]) > 0 and opt.steps == 2
    for k in be:
        assert torch.equal(be[k], bt[k]), k


# ---- 5. dataAugmentation -------------------------------------------------------------------------------------------------------
FORCES = [("buoyancy", dict(buoyancyScale=2.0)), ("gravity", dict(gravityScale=1.5)), ("vorticity", dict(vorticityConfinementAmp=0.8)),
          ("all", dict(buoyancyScale=2.0, gravityScale=1.5, vorticityConfinementAmp=0.8))]


@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
@pytest.mark.parametrize("name,force", FORCES, ids=[f[0] for f in FORCES])
def test_data_augmentation_equals_the_operators(name, force, is3D):
    """simulate.lua:374-414 by hand: addBuoyancy with mconf.gravity as it is, addGravity with gravity * (-getDx / 4 *
    gravityScale) as a float tensor holds it, vorticityConfinement with getDx * amp"""
    from fluidnet_amd import dataAugmentation, tfluids
    mconf = dict(_mconf("jacobi"), gravity=[0.0, -1.0, 0.0], dt=0.07, **force)
    before = copy.deepcopy(mconf)
    got = _batch(is3D)
    U, flags, dens = got["UDiv"].clone(), got["flags"], got["densityDiv"]
    dataAugmentation(None, mconf, got)
    if "buoyancyScale" in force:
        tfluids.addBuoyancy(U, flags, dens, [0.0, -1.0, 0.0], 0.07)
    if "gravityScale" in force:
        s = np.float32((-tfluids.getDx(flags) / 4) * 1.5)
        tfluids.addGravity(U, flags, [float(np.float32(v) * s) for v in (0.0, -1.0, 0.0)], 0.07)
    if "vorticityConfinementAmp" in force:
        tfluids.vorticityConfinement(U, flags, tfluids.getDx(flags) * 0.8)
    assert torch.equal(got["UDiv"], U) and not torch.equal(U, _batch(is3D)["UDiv"])
    assert not torch.equal(U[0], U[1]) and mconf == before
    # the density may come as batch.density (:386)
    alt = _batch(is3D)
    alt["density"] = alt.pop("densityDiv")
    dataAugmentation(None, mconf, alt)
    assert torch.equal(alt["UDiv"], U)


# ---- 6. fold and guard ---------------------------------------------------------------------------------------------------------
def test_the_sums_are_the_running_fp64_sum_of_the_losses():
    mconf = _mconf("jacobi")
    net, crit, opt, closure = _setup(False, mconf)
    s = np.zeros(5, np.float64)
    for it, plan in enumerate([_plan(1, 0.05), _plan(4, 0.03, vort=0.8), _plan(1)]):
        closure(_batch(False, seed=50 + it), plan)
        l, ll = closure.loss.cpu().numpy(), closure.loss_long_term.cpu().numpy()
        s[0] = s[0] + l[0]
        s[1] = s[1] + l[1]
        s[2] = s[2] + l[2]
        s[3] = s[3] + l[3]
        s[3] = s[3] + ll[3]
        s[4] = s[4] + ll[3]
        assert l[3] == (l[0] + l[1]) + l[2] and all(x > 0 for x in l) and ll[3] > 0
        assert np.array_equal(closure.sums.cpu().numpy(), s), (it, closure.sums.cpu().numpy(), s)
    assert int(closure.guard.item()) == 0
    closure.check()
    closure.reset()
    assert not closure.sums.any() and not closure.guard.any()


def _snapshot(net, opt, probe):
    net.eval()
    with torch.no_grad():
        p, U = net(*probe)
    net.train()
    m, v = opt.state()
    return [t.detach().clone() for t in net.parameters()] + m + (v or []) + [p.clone(), U.clone()], opt.steps


@pytest.mark.parametrize("how", ["nan-in-UDiv", "small-errLimit"])
def test_a_set_guard_stops_the_step(how):
    """one NaN in UDiv makes the loss NaN by ordinary arithmetic; errLimit = 1e-12 is below any loss: either way the guard is
    set, and the guarded step leaves parameters, moments, the counter and the native model's weights (a forward) as they were.
    (The NaN batch runs without the long-term pass: the NaN meets the net and the criterion only, never a back-trace.)"""
    from fluidnet_amd import TfluidsError
    mconf = _mconf("manta", longTermDivNumSteps=None if how == "nan-in-UDiv" else [4, 16])
    net, crit, opt, closure = _setup(False, mconf, errLimit=1e-12 if how == "small-errLimit" else None)
    probe = [_batch(False, seed=60)[k] for k in ("pDiv", "UDiv", "flags")]
    if how == "nan-in-UDiv":
        closure(_batch(False, seed=61), _plan(1))       # a clean step first
        assert int(closure.guard.item()) == 0 and opt.steps == 1
    before, steps = _snapshot(net, opt, probe)
    bad = _batch(False, seed=62)
    if how == "nan-in-UDiv":
        bad["UDiv"][1, 0, 0, 7, 13] = float("nan")
    closure(bad, _plan(1, 0.05))
    assert int(closure.guard.item()) == 1
    after, steps_after = _snapshot(net, opt, probe)
    assert steps_after == steps and all(torch.equal(a, b) for a, b in zip(before, after))
    closure(_batch(False, seed=63), _plan(1))           # sticky: a clean batch afterwards is not stepped either
    after, steps_after = _snapshot(net, opt, probe)
    assert steps_after == steps and all(torch.equal(a, b) for a, b in zip(before, after))
    with pytest.raises(TfluidsError, match=r"criterion error is NaN or > 1e-12" if how == "small-errLimit" else r"criterion error is NaN or > 1e9"):
        closure.check(5)
    assert closure.first_bad == 5


def test_the_fold_by_itself():
    """tfl_closure_fold on hand-made losses: the two passes' slots, the order of the adds, NaN and the limit, stickiness"""
    from fluidnet_amd import tfluids
    like = torch.zeros(1, device=DEV)
    lib, ctx = tfluids._context(like)
    sums = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64, device=DEV)
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fold(loss, longTerm, limit=1e9):
        l = torch.tensor(loss, dtype=torch.float64, device=DEV)
        tfluids._call(lib, ctx, lib.tfl_closure_fold(ctx, ctypes.c_void_p(l.data_ptr()), ctypes.c_void_p(sums.data_ptr()),
                                                     ctypes.c_void_p(guard.data_ptr()), longTerm, limit))
        return sums.cpu().tolist(), int(guard.item())

    assert fold([0.1, 0.2, 0.3, 0.7], 0) == ([1.0 + 0.1, 2.0 + 0.2, 3.0 + 0.3, 4.0 + 0.7, 5.0], 0)
    assert fold([9.0, 9.0, 9.0, 1e9], 1) == ([1.0 + 0.1, 2.0 + 0.2, 3.0 + 0.3, (4.0 + 0.7) + 1e9, 5.0 + 1e9], 0)      # not ABOVE the limit
    assert fold([0.0, 0.0, 0.0, 0.5], 1, limit=0.25)[1] == 1
    assert fold([0.0, 0.0, 0.0, 0.0], 0)[1] == 1                                                                        # sticky
    guard.zero_()
    got, g = fold([0.0, 0.0, 0.0, float("nan")], 0)
    assert g == 1 and np.isnan(got[3]) and got[0] == 1.0 + 0.1
    guard.zero_()
    assert fold([0.0, 0.0, 0.0, float("inf")], 1)[1] == 1
    assert lib.tfl_closure_fold(ctx, None, ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(guard.data_ptr()), 0, 1e9) != 0


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_null_and_zero_guards_are_the_plain_step(method):
    """tfl_optim_step (the old entry), tfl_optim_step_guarded with NULL and with a zero guard word: the same bits after two
    steps; with a set word nothing moves -- the clipped gradients are not written either"""
    from fluidnet_amd import tfluids
    from fluidnet_amd.train import _ptr_array
    mconf = _mconf("manta", optimizationMethod=method)
    if method == "rmsprop":
        mconf["optimState"] = dict(learningRate=0.001, alpha=0.9, epsilon=1e-6, weightDecay=0.01)
    runs = []
    for how in ("old-entry", "null", "zero", "set"):
        net, crit, opt, _ = _setup(False, mconf)
        probe = [_batch(False, seed=60)[k] for k in ("pDiv", "UDiv", "flags")]
        net(*probe)                                             # (the native model exists before the first step)
        start, _ = _snapshot(net, opt, probe)
        gw, gb = _grads(net)
        grng = np.random.RandomState(9)
        src = [_up((grng.randn(*g.shape) * 0.7).astype(np.float32)) for g in gw + gb]      # norm > 1: the clip rewrites .grad
        guard = torch.full((1,), 1 if how == "set" else 0, dtype=torch.int32, device=DEV)
        for _ in range(2):
            for g, s in zip(gw + gb, src):
                g.copy_(s)
            if how == "old-entry":
                lib, ctx = tfluids._context(net.weights[0])
                tfluids._call(lib, ctx, lib.tfl_optim_step(ctx, opt._opt, _ptr_array(list(net.weights)), _ptr_array(list(net.biases)),
                                                           _ptr_array(gw), _ptr_array(gb)))
                net._stepped_on_device()
            else:
                opt.step(guard=None if how == "null" else guard)
        snap, steps = _snapshot(net, opt, probe)
        runs.append((how, snap + [g.clone() for g in gw + gb], steps, start, src))
    (_, old, steps_old, start, src), null, zero, stuck = runs[0], runs[1], runs[2], runs[3]
    assert steps_old == 2 and not torch.equal(old[0], start[0]) and not torch.equal(old[-1], src[-1])
    for how, snap, steps, _, _ in (null, zero):
        assert steps == 2 and all(torch.equal(a, b) for a, b in zip(old, snap)), how
    _, snap, steps, start, src = stuck
    n = len(start)
    assert steps == 0 and all(torch.equal(a, b) for a, b in zip(start, snap[:n]))
    assert all(torch.equal(a, b) for a, b in zip(src, snap[n:]))


def test_run_epoch_means_and_the_batch_it_names():
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.run_epoch import RandomStateRng, run_epoch
    mconf = _mconf("manta", longTermDivNumSteps=[1, 2], longTermDivProbability=0.5)
    before = copy.deepcopy(mconf)
    net, crit, opt, closure = _setup(False, mconf)
    clean = [_batch(False, seed=70 + i) for i in range(2)]
    out = run_epoch(closure, [_clone(b) for b in clean], rng=RandomStateRng(4))
    sums = closure.sums.cpu().numpy()
    assert out == dict(aveLoss=sums[3] / 2, avePLoss=sums[0] / 2, aveULoss=sums[1] / 2, aveDivLoss=sums[2] / 2,
                       aveLongTermDivLoss=sums[4] / 2, nbatches=2)
    assert out["aveLoss"] > out["aveLongTermDivLoss"] > 0 and opt.steps == 2 and mconf == before
    good = [p.detach().clone() for p in net.parameters()]
    # evaluation: same plans (same seed), no step; the means are those of the weights as they now are
    ev = run_epoch(closure, [_clone(b) for b in clean], rng=RandomStateRng(4), training=False)
    assert opt.steps == 2 and ev["nbatches"] == 2 and ev["aveLoss"] > 0
    # a NaN in the third of four batches (no long-term pass: the NaN meets the net and the criterion only): named, and the
    # parameters are those after the two clean batches
    mconf = _mconf("manta", longTermDivNumSteps=None)
    net, _, opt, closure = _setup(False, mconf)
    run_epoch(closure, [_clone(b) for b in clean], rng=RandomStateRng(4))
    good = [p.detach().clone() for p in net.parameters()]
    net2, _, opt2, closure2 = _setup(False, mconf)
    bad = _batch(False, seed=72)
    bad["UDiv"][0, 1, 0, 5, 9] = float("nan")
    with pytest.raises(TfluidsError, match=r"criterion error is NaN or > 1e9 \(first seen at batch 2\)"):
        run_epoch(closure2, [_clone(clean[0]), _clone(clean[1]), bad, _batch(False, seed=73)], rng=RandomStateRng(4))
    assert closure2.first_bad == 2 and opt2.steps == 2
    assert all(torch.equal(a, b.detach()) for a, b in zip(good, net2.parameters()))
    with pytest.raises(TfluidsError, match="No batches"):
        run_epoch(closure2, [])


def test_a_torch_optimiser_takes_the_unfused_path():
    """torch.optim.SGD through the closure: the clip of run_epoch.lua:304-312 in torch ops, the guard read before the step"""
    from fluidnet_amd import FluidCriterion, ProjectionNet, TfluidsError
    from fluidnet_amd.run_epoch import Closure
    mconf = _mconf("manta", gradNormThreshold=1e-3, longTermDivNumSteps=None)
    net = ProjectionNet(R.make_model("default", False), device=DEV).train()
    crit = FluidCriterion(1.0, 1.0, 1.0)
    sgd = torch.optim.SGD(net.parameters(), lr=0.5)
    closure = Closure(net, crit, sgd, None, mconf)
    start = [p.detach().clone() for p in net.parameters()]
    closure(_batch(False), _plan(1, 0.05))
    moved = torch.sqrt(sum(((a - b.detach()).double() ** 2).sum() for a, b in zip(start, net.parameters())))
    assert abs(float(moved) - 0.5 * 1e-3) <= 1e-5 * 0.5 * 1e-3      # the step is lr times a gradient of norm = the threshold
    bad = _batch(False)
    bad["UDiv"][0, 0, 0, 3, 3] = float("nan")
    held = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(TfluidsError, match="criterion error is NaN"):
        closure(bad, _plan(1, 0.05))
    assert all(torch.equal(a, b.detach()) for a, b in zip(held, net.parameters()))


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_as_eager_calls(monkeypatch):
    """2-D net, manta targets, lossPLambda = 0 (normalizePressureMean polls the device and is not capturable): one eager call,
    then one call recorded with torch.cuda.graph and replayed twice, against three eager calls on the same batch tensors. A
    host read or a synchronisation inside the call would fail the capture; a host-advanced counter would stand still."""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    mconf = _mconf("manta", (0.0, 1.0, 1.0))
    plan = _plan(1, 0.05, vort=0.8)
    net_e, _, opt_e, eager = _setup(False, mconf)
    net_g, _, opt_g, graphed = _setup(False, mconf)
    be = _batch(False)
    bg = _clone(be)
    for _ in range(3):
        eager(be, plan)
    graphed(bg, plan)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed(bg, plan)
    assert opt_g.steps == 1                                      # (captured, not run)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert opt_e.steps == 3 == opt_g.steps
    diff = _differences(_state(net_e, opt_e, be, eager.sums), _state(net_g, opt_g, bg, graphed.sums))
    assert not diff, diff
    assert torch.equal(eager.loss, graphed.loss) and torch.equal(eager.loss_long_term, graphed.loss_long_term)
    assert int(graphed.guard.item()) == 0


# ---- 8. it trains --------------------------------------------------------------------------------------------------------------
def _train_series():
    L = R.LOOP
    pDiv, UDiv, flags = R.loop_scene()
    mconf = _mconf("jacobi", L["lambdas"], maxIter=L["jacobi_iters"], longTermDivNumSteps=[2, 2])
    net, crit, opt, closure = _setup(False, mconf, model=R.loop_model())
    fresh = dict(pDiv=_up(pDiv), UDiv=_up(UDiv), flags=_up(flags), densityDiv=_up(np.zeros_like(pDiv)),
                 pTarget=_up(pDiv), UTarget=_up(UDiv))
    series = []
    for _ in range(L["steps"]):
        closure(_clone(fresh), _plan(2))
        series.append((float(closure.loss[3]), float(closure.loss_long_term[3])))
    closure.check()
    return series, opt.steps


def test_it_trains():
    """R.LOOP's scene and model, fluidnet_amd.optim.Adam as default_conf.lua configures it, jacobi targets, two future steps,
    20 iterations on the same mini-batch: the total loss (main + long-term) of the last iteration is below the first's, and a
    second run gives the same series. (No bar on how far it falls; profiles/run_epoch.md keeps a measured series.)"""
    first, steps = _train_series()
    total = [a + b for a, b in first]
    for i, (a, b) in enumerate(first):
        print("iteration %2d: main %.6e  long-term %.6e  total %.6e" % (i, a, b, a + b))
    assert steps == R.LOOP["steps"]
    assert total[-1] < total[0], (total[0], total[-1])
    second, _ = _train_series()
    assert first == second
