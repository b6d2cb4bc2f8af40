"""GPU checks of data-parallel training: tfl_optim_step_reduced / _reduced_guard / _sync_parameters, optim.step(comm=...),
run_epoch.Closure(comm=...), run_epoch() under a comm and dist.run_virtual_closures.

All ranks are VIRTUAL: threads of this process over dist.ThreadComm on one GPU (dist.run_virtual), worlds of 2 and 3. The rule
of the reduced step is its whole definition -- g = float((g_0 + g_1 + ...) in fp64, rank order, / world) -- so the yardstick of
every test but one is a hand form in torch ops and existing public calls, and every comparison is torch.equal. The one other
(test 5) holds the reduced gradients to the fp64 whole-batch gradient of tests/data_parallel_ref.py at model_grad_ref.BAR.
Grids and nets are those of tests/test_hip_run_epoch.py: 2-D 1 x 16 x 32 and 3-D 8 x 8 x 32, B = 2 per rank, the seeded `default`
nets of tests/model_grad_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import data_parallel_ref as D
import model_grad_ref as R
import test_hip_run_epoch as E

pytestmark = pytest.mark.gpu
DEV = E.DEV
MISTAKES = D.MISTAKES


def _world(world, is3D, mconf, seeds=None, errLimits=None, comm_cls=None):
    """one (net, criterion, optimiser, comm, closure) per rank over a fresh hub; equal seeds = equal parameters"""
    from fluidnet_amd import FluidCriterion, ProjectionNet, dist, optim
    from fluidnet_amd.run_epoch import Closure
    hub = dist.ThreadComm.Hub(world)
    ranks = []
    for r in range(world):
        net = ProjectionNet(R.make_model("default", is3D, seed=3 if seeds is None else seeds[r]), device=DEV).train()
        crit = FluidCriterion(mconf["lossPLambda"], mconf["lossULambda"], mconf["lossDivLambda"])
        opt = optim.from_mconf(net, mconf)
        comm = (comm_cls or dist.ThreadComm)(hub, r)
        kw = {} if errLimits is None or errLimits[r] is None else dict(errLimit=errLimits[r])
        ranks.append(dict(net=net, crit=crit, opt=opt, comm=comm, closure=Closure(net, crit, opt, None, mconf, comm=comm, **kw)))
    return hub, ranks


def _single(is3D, mconf):
    net, crit, opt, closure = E._setup(is3D, mconf)
    return dict(net=net, crit=crit, opt=opt, closure=closure)


def _probe(is3D):
    return [E._batch(is3D, seed=60)[k] for k in ("pDiv", "UDiv", "flags")]


def _seeded_grads(net, seed, scale=0.7):
    rng = np.random.RandomState(seed)
    return [E._up((rng.randn(*g.shape) * scale).astype(np.float32)) for g in _flat_grads(net)]


def _flat_grads(net):
    gw, gb = E._grads(net)
    return gw + gb


def _mean_by_the_rule(per_rank):
    """((g0.double() + g1.double() + ...) / world).float(), the ranks added in ThreadComm's order"""
    out = []
    for parts in zip(*per_rank):
        acc = parts[0].double()
        for g in parts[1:]:
            acc = acc + g.double()
        out.append((acc / len(parts)).float())
    return out


def _full(rank, probe):
    """parameters, moments and an eval forward (the native model's weight forms), the gradient arrays, the counter"""
    snap, steps = E._snapshot(rank["net"], rank["opt"], probe)
    return snap + [g.clone() for g in _flat_grads(rank["net"])], steps


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _optim_mconf(method, threshold, wd):
    m = E._mconf("manta", optimizationMethod=method, gradNormThreshold=threshold)
    if method == "rmsprop":
        m["optimState"] = dict(learningRate=0.001, alpha=0.9, epsilon=1e-6, weightDecay=wd)
    else:
        m["optimState"] = dict(m["optimState"], weightDecay=wd)
    return m


# ---- 1. the reduced step against the hand form ---------------------------------------------------------------------------------
# (name, method, gradNormThreshold, weightDecay, world, is3D); gradients of norm >> 1: a threshold of 1 clips, 1e6 does not
STEP_CASES = [
    ("adam-clip-w2-2d", "adam", 1, 0.0, 2, False),
    ("adam-clip-not-triggered-wd-w3-2d", "adam", 1e6, 0.01, 3, False),
    ("adam-no-clip-wd-w3-3d", "adam", 0, 0.01, 3, True),
    ("rmsprop-clip-wd-w3-2d", "rmsprop", 1, 0.01, 3, False),
    ("rmsprop-no-clip-w2-3d", "rmsprop", 0, 0.0, 2, True),
]


@pytest.mark.parametrize("name,method,threshold,wd,world,is3D", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_the_reduced_step_equals_the_guarded_step_on_hand_averaged_gradients(name, method, threshold, wd, world, is3D):
    from fluidnet_amd import dist
    mconf = _optim_mconf(method, threshold, wd)
    hub, ranks = _world(world, is3D, mconf)
    ref = _single(is3D, mconf)
    probe = _probe(is3D)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    for it in range(3):
        src = [_seeded_grads(ranks[r]["net"], 100 * it + r) for r in range(world)]      # different on every rank and step

        def work(r):
            def f():
                for g, s in zip(_flat_grads(ranks[r]["net"]), src[r]):
                    g.copy_(s)
                ranks[r]["opt"].step(guard=zero, comm=ranks[r]["comm"])
            return f
        dist.run_virtual(hub, [work(r) for r in range(world)])
        for g, s in zip(_flat_grads(ref["net"]), _mean_by_the_rule(src)):
            g.copy_(s)
        ref["opt"].step(guard=zero)
        if it in (0, 2):
            want, steps = _full(ref, probe)
            assert steps == it + 1
            for r in range(world):
                got, steps_r = _full(ranks[r], probe)
                assert steps_r == steps and _same(got, want), (name, it, r)
            # the step did something, and the clip did what the case says
            avg = _mean_by_the_rule(src)
            rewritten = not _same(want[-len(avg):], avg)
            assert rewritten == (threshold == 1 or wd > 0), name


# ---- 2. the guard --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [1, 0], ids=["clip", "no-clip"])
def test_one_ranks_guard_holds_every_rank(threshold):
    from fluidnet_amd import dist
    world = 3
    mconf = _optim_mconf("adam", threshold, 0.01)
    hub, ranks = _world(world, False, mconf)
    ref = _single(False, mconf)
    probe = _probe(False)
    guards = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(world)]
    src = [_seeded_grads(ranks[r]["net"], 7 + r) for r in range(world)]

    def work(r):
        def f():
            for g, s in zip(_flat_grads(ranks[r]["net"]), src[r]):
                g.copy_(s)
            ranks[r]["opt"].step(guard=guards[r], comm=ranks[r]["comm"])
            return ranks[r]["opt"].reduced_guard()
        return f

    assert all(int(ranks[r]["opt"].reduced_guard().item()) == 0 for r in range(world))      # before the first step
    before = [_full(ranks[r], probe) for r in range(world)]
    guards[1].fill_(1)
    reduced = dist.run_virtual(hub, [work(r) for r in range(world)])
    for r in range(world):
        got, steps = _full(ranks[r], probe)
        n = len(src[r])
        assert steps == 0 and _same(got[:-n], before[r][0][:-n]), r      # parameters, moments, weight forms, counter
        assert _same(got[-n:], src[r]), r                                # the gradient arrays keep the local gradients
        assert reduced[r].dtype == torch.int32 and reduced[r].is_cuda and int(reduced[r].item()) != 0, r
    guards[1].zero_()
    reduced = dist.run_virtual(hub, [work(r) for r in range(world)])
    for g, s in zip(_flat_grads(ref["net"]), _mean_by_the_rule(src)):
        g.copy_(s)
    ref["opt"].step()
    want, _ = _full(ref, probe)
    for r in range(world):
        got, steps = _full(ranks[r], probe)
        assert steps == 1 and _same(got, want) and int(reduced[r].item()) == 0, r


# ---- 3. entry equivalence ------------------------------------------------------------------------------------------------------
def _counting_comm():
    from fluidnet_amd import dist

    class Counting(dist.ThreadComm):
        calls = 0
        doubles = None

        def allreduce(self, stats):
            self.calls += 1
            self.doubles = stats.numel()
            super().allreduce(stats)
    return Counting


@pytest.mark.parametrize("threshold", [1, 0], ids=["clip", "no-clip"])
def test_entries_are_equivalent_and_launch_counts_are_bounded(threshold):
    from fluidnet_amd import tfluids
    from fluidnet_amd.train import _ptr_array
    mconf = _optim_mconf("adam", threshold, 0.0)
    probe = _probe(False)
    runs, launches = {}, {}
    for how in ("guarded", "null-comm", "hub-of-one"):
        hub, (rank,) = _world(1, False, mconf, comm_cls=_counting_comm())
        net, opt, comm = rank["net"], rank["opt"], rank["comm"]
        net(*probe)
        guard = torch.zeros(1, dtype=torch.int32, device=DEV)
        src = _seeded_grads(net, 9)
        for it in range(2):
            for g, s in zip(_flat_grads(net), src):
                g.copy_(s)
            with tfluids.profile(net.weights[0]) as prof:
                if how == "guarded":
                    opt.step(guard=guard)
                elif how == "hub-of-one":
                    opt.step(guard=guard, comm=comm)
                else:
                    lib, ctx = tfluids._context(net.weights[0])
                    gw, gb = E._grads(net)
                    tfluids._call(lib, ctx, lib.tfl_optim_step_reduced(
                        ctx, opt._opt, _ptr_array(list(net.weights)), _ptr_array(list(net.biases)), _ptr_array(gw), _ptr_array(gb),
                        ctypes.c_void_p(guard.data_ptr()), None, 1, None, 0))
                    net._stepped_on_device()
            launches[how] = {k: v["calls"] for k, v in prof.kernels.items()}
        runs[how] = _full(rank, probe)
        assert comm.calls == (2 if how == "hub-of-one" else 0), how                     # exactly one all-reduce per step
        if how == "hub-of-one":
            lib, ctx = tfluids._context(net.weights[0])
            assert comm.doubles == int(lib.tfl_optim_get_state(ctx, opt._opt, None, None)) + 1      # P + 1
    print(launches)
    assert runs["guarded"][1] == 2
    for how in ("null-comm", "hub-of-one"):
        assert runs[how][1] == 2 and _same(runs[how][0], runs["guarded"][0]), how
    assert launches["null-comm"] == launches["guarded"]                                  # the guarded entry: the same launches
    extra = sum(launches["hub-of-one"].values()) - sum(launches["guarded"].values())
    assert 1 <= extra <= 2, launches
    new = {k for k in launches["hub-of-one"] if launches["hub-of-one"][k] != launches["guarded"].get(k, 0)}
    assert new <= {"k_optim_pack", "k_optim_unpack", "k_optim_unpack_norm", "k_optim_norm"}, new


# ---- 4. the closure ------------------------------------------------------------------------------------------------------------
def _passes(net, crit, mconf, batch, plan, sums, early=None):
    """both passes of one rank's mini-batch with the public calls, manta targets (run_epoch.lua:160-302 as
    tests/test_hip_run_epoch.py hand_iteration sequences it), into net's .grad; early: a list that receives a copy of the
    gradients as they stand BEFORE the long-term pass. Returns the local guard as the fold forms it."""
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    m = dict(mconf)
    for k in ("buoyancyScale", "gravityScale", "vorticityConfinementAmp", "gravity"):
        m[k] = plan[k]
    flags = batch["flags"]
    is3D = batch["UDiv"].size(1) == 3
    bad = []

    def forward_criterion_backward(accumulate):
        p, U, tape = net.forward_train(batch["pDiv"], batch["UDiv"], flags)
        p.requires_grad_(True)
        U.requires_grad_(True)
        err = crit((p, U), (batch["pTarget"], batch["UTarget"], flags))
        err.backward()
        net.backward(flags, p.grad, U.grad, tape, out=E._grads(net), accumulate=accumulate)
        return err.detach()

    if m["lossPLambda"] > 0:
        tfluids.normalizePressureMean(batch["pTarget"], flags, is3D)
    for g in _flat_grads(net):
        g.zero_()
    err = forward_criterion_backward(True)
    sums[3] += err
    sums[0] += crit.pLoss
    sums[1] += crit.uLoss
    sums[2] += crit.divLoss
    bad.append(err)
    if early is not None:
        early.extend(g.clone() for g in _flat_grads(net))
    n = plan["numFutureSteps"]
    if m["longTermDivNumSteps"] is not None and m["longTermDivLambda"] > 0 and n > 0:
        m["dt"] = plan["dt"]
        net.eval()
        state = dict(batch, density=batch["densityDiv"])
        for i in range(1, n + 1):
            simulate_native(None, m, state, net, outputDiv=(i == n))
        net.train()
        crit.pLambda = crit.uLambda = 0
        crit.divLambda = m["longTermDivLambda"]
        err2 = forward_criterion_backward(True)
        sums[4] += err2
        sums[3] += err2
        bad.append(err2)
        crit.pLambda, crit.uLambda, crit.divLambda = m["lossPLambda"], m["lossULambda"], m["lossDivLambda"]
    return bad


def hand_world_iteration(ref, mconf, batches, plans, sums, limits, mistake=None):
    """one data-parallel iteration in ONE process, as rank 0 sees it: every rank's two passes into gradient buffers of its own
    (the ranks hold equal parameters, so one net serves them in turn), the mean by the rule, the reduced guard, then ONE guarded
    step. mistake: one of MISTAKES, made on purpose."""
    net, crit, opt = ref["net"], ref["crit"], ref["opt"]
    G, guards = [], []
    for r, (batch, plan) in enumerate(zip(batches, plans)):
        early = []
        errs = _passes(net, crit, mconf, batch, plan, sums[r], early)
        G.append(early if mistake == "reduce-before-the-long-term-pass" else [g.clone() for g in _flat_grads(net)])
        guards.append(int(any(not (float(e) <= limits[r]) for e in errs)))      # NaN or above the limit (tfl_closure_fold)
    avg = _mean_by_the_rule(G)
    if mistake == "sum-instead-of-mean":
        avg = [(g.double() * len(G)).float() for g in avg]
    if mistake == "rank-0-only":
        avg = G[0]
    held = guards[0] if mistake == "guard-left-local" else int(any(guards))
    for g, s in zip(_flat_grads(net), avg):
        g.copy_(s)
    opt.step(guard=torch.full((1,), held, dtype=torch.int32, device=DEV))
    return held


def _closure_state(rank, batch):
    return E._state(rank["net"], rank["opt"], batch, rank["closure"].sums)


# (name, is3D, lossDivLambda of the main pass, per iteration the plans of rank 0 and rank 1)
CLOSURE_CASES = [
    ("2d", False, 1.0, [(E._plan(4, 0.05), E._plan(1, 0.13)), (E._plan(1, 0.1), E._plan(4, 0.07, vort=0.8)), (E._plan(4, 0.03), E._plan(4, 0.06))]),
    ("3d", True, 0.0, [(E._plan(1, 0.06), E._plan(4, 0.1)), (E._plan(4, 0.12), E._plan(1, 0.05)), (E._plan(1, 0.1), E._plan(1, 0.08))]),
]


@pytest.mark.parametrize("name,is3D,lamD,plans", CLOSURE_CASES, ids=[c[0] for c in CLOSURE_CASES])
def test_the_closure_under_a_comm_equals_the_hand_sequence(name, is3D, lamD, plans):
    from fluidnet_amd import dist
    mconf = E._mconf("manta", (1.0, 1.0, lamD))
    hub, ranks = _world(2, is3D, mconf)
    ref = _single(is3D, mconf)
    sums = [torch.zeros(5, dtype=torch.float64, device=DEV) for _ in range(2)]
    for it, pair in enumerate(plans):
        fresh = [E._batch(is3D, seed=31 + 10 * it + r) for r in range(2)]      # different batches per rank
        mine = [E._clone(b) for b in fresh]
        theirs = [E._clone(b) for b in fresh]
        dist.run_virtual(hub, [lambda r=r: ranks[r]["closure"](mine[r], pair[r]) for r in range(2)])
        held = hand_world_iteration(ref, mconf, theirs, pair, sums, limits=[E_LIMIT, E_LIMIT])
        assert held == 0
        a, b = _closure_state(ranks[0], mine[0]), _closure_state(ranks[1], mine[1])
        same_keys = [k for k, _ in a if k.startswith(("param", "m", "v"))]
        assert not [k for k in E._differences(a, b) if k in same_keys], (name, it)            # the ranks are equal
        for r in range(2):
            want = E._state(ref["net"], ref["opt"], theirs[r], sums[r])
            diff = E._differences(_closure_state(ranks[r], mine[r]), want)
            assert not diff, (name, it, r, diff)
            assert not torch.equal(mine[r]["UDiv"], fresh[r]["UDiv"])                         # (the rollout moved the batch)
            assert int(ranks[r]["closure"].guard_all.item()) == 0 and float(ranks[r]["closure"].sums[4]) > 0
        assert not torch.equal(mine[0]["UDiv"], mine[1]["UDiv"])
    assert ranks[0]["opt"].steps == ranks[1]["opt"].steps == ref["opt"].steps == len(plans)


E_LIMIT = 1e9


@pytest.mark.parametrize("mistake", MISTAKES)
def test_a_mistake_in_the_hand_sequence_shows(mistake):
    """2-D, world 2, one iteration with the long-term pass on both ranks. The guard case runs rank 1 with errLimit = 1e-12
    (below any loss): the closure holds both ranks back, the correct hand sequence agrees, and the one that leaves the guard
    local steps rank 0. No clip and a weight decay: a clip to norm 1 and Adam's m / sqrt(v) would both forgive a gradient that
    is merely scaled (the sum in place of the mean)."""
    from fluidnet_amd import dist
    mconf = _optim_mconf("adam", 0, 0.01)
    limits = [E_LIMIT, 1e-12] if mistake == "guard-left-local" else [E_LIMIT, E_LIMIT]
    pair = (E._plan(4, 0.04), E._plan(1, 0.09))
    hub, ranks = _world(2, False, mconf, errLimits=limits)
    fresh = [E._batch(False, seed=31 + r) for r in range(2)]
    mine = [E._clone(b) for b in fresh]
    dist.run_virtual(hub, [lambda r=r: ranks[r]["closure"](mine[r], pair[r]) for r in range(2)])
    got = _closure_state(ranks[0], mine[0])
    for m in (None, mistake):
        ref = _single(False, mconf)
        sums = [torch.zeros(5, dtype=torch.float64, device=DEV) for _ in range(2)]
        theirs = [E._clone(b) for b in fresh]
        held = hand_world_iteration(ref, mconf, theirs, pair, sums, limits, mistake=m)
        diff = E._differences(got, E._state(ref["net"], ref["opt"], theirs[0], sums[0]))
        print(m, "->", diff)
        if m is None:
            assert not diff and held == int(mistake == "guard-left-local")
            assert int(ranks[0]["closure"].guard_all.item()) == int(ranks[1]["closure"].guard_all.item()) == held
            assert int(ranks[0]["closure"].guard.item()) == 0
        else:
            assert any(k.startswith("param") for k in diff) and any(k.startswith("m") for k in diff)


# ---- 5. the fp64 yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
def test_the_reduced_gradients_against_the_fp64_whole_batch_gradient(is3D):
    """world 2, clip off, decay 0: after the step the gradient arrays hold the mean of the ranks' gradients, which is the
    gradient of the criterion's mean over all 4 items; held per tensor to model_grad_ref.BAR against fp64 on the CPU"""
    from fluidnet_amd import dist
    mconf = _optim_mconf("adam", 0, 0.0)
    hub, ranks = _world(2, is3D, mconf)
    parts = [D.rank_inputs(is3D, r) for r in range(2)]
    batches = [{k: E._up(v) for k, v in p.items()} for p in parts]

    def work(r):
        def f():
            net, crit, b = ranks[r]["net"], ranks[r]["crit"], batches[r]
            p, U, tape = net.forward_train(b["pDiv"], b["UDiv"], b["flags"])
            p.requires_grad_(True)
            U.requires_grad_(True)
            crit((p, U), (b["pTarget"], b["UTarget"], b["flags"])).backward()
            net.backward(b["flags"], p.grad, U.grad, tape, out=E._grads(net), accumulate=False)
            ranks[r]["opt"].step(comm=ranks[r]["comm"])
        return f
    dist.run_virtual(hub, [work(r) for r in range(2)])
    model = R.make_model("default", is3D)
    whole = D.whole_batch(parts)
    want = D.loss_grads(model, whole)
    witness = D.loss_grads(model, whole, dtype=torch.float32)
    for r in range(2):
        gw, gb = E._grads(ranks[r]["net"])
        got = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in zip(gw, gb)]
        rels = R.rel_l2_per_tensor(got, want)
        wit = R.rel_l2_per_tensor(witness, want)
        for l, ((a, b), (c, d)) in enumerate(zip(rels, wit)):
            print("rank %d layer %d: gradWeight %.2e (PyTorch fp32 %.2e, ratio %.2f)  gradBias %.2e (PyTorch fp32 %.2e, ratio %.2f)"
                  % (r, l, a, c, a / max(c, 1e-30), b, d, b / max(d, 1e-30)))
        assert max(max(p) for p in rels) <= R.BAR, rels
    assert ranks[0]["opt"].steps == 1


# ---- 6. run_epoch --------------------------------------------------------------------------------------------------------------
def test_run_epoch_under_a_comm():
    from fluidnet_amd import TfluidsError, dist
    from fluidnet_amd.run_epoch import RandomStateRng
    mconf = E._mconf("manta", longTermDivNumSteps=[1, 2], longTermDivProbability=0.5)
    hub, ranks = _world(2, False, mconf)
    closures = [rk["closure"] for rk in ranks]
    per_rank = [[E._batch(False, seed=70 + 2 * r + i) for i in range(2)] for r in range(2)]
    out = dist.run_virtual_closures(closures, per_rank, rngs=[RandomStateRng(4), RandomStateRng(5)])      # different plans
    assert out[0] == out[1] and out[0]["nbatches"] == 4
    s = [c.sums.cpu().numpy() for c in closures]
    total = (0 + s[0]) + s[1]                                  # ThreadComm's order, in fp64
    want = dict(aveLoss=float(total[3] / 4), avePLoss=float(total[0] / 4), aveULoss=float(total[1] / 4),
                aveDivLoss=float(total[2] / 4), aveLongTermDivLoss=float(total[4] / 4), nbatches=4)
    assert out[0] == want and not np.array_equal(s[0], s[1]) and want["aveLongTermDivLoss"] > 0
    assert ranks[0]["opt"].steps == 2 == ranks[1]["opt"].steps
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(ranks[0]["net"].parameters(), ranks[1]["net"].parameters()))
    # `steps`: the first batches only
    hub1, ranks1 = _world(2, False, mconf)
    one = dist.run_virtual_closures([rk["closure"] for rk in ranks1], per_rank, steps=1, rngs=[RandomStateRng(4), RandomStateRng(5)])
    assert one[0]["nbatches"] == 2 and ranks1[0]["opt"].steps == 1

    # a NaN in rank 1's second of three batches, the long-term pass off: every rank names batch 1 and has stepped once
    mconf = E._mconf("manta", longTermDivNumSteps=None)
    clean = [[E._batch(False, seed=s) for s in seeds] for seeds in ((70, 71, 73), (74, 72, 75))]
    rngs = lambda: [RandomStateRng(4), RandomStateRng(5)]
    hub_a, first = _world(2, False, mconf)
    dist.run_virtual_closures([rk["closure"] for rk in first], [[E._clone(b) for b in clean[r]] for r in range(2)], steps=1, rngs=rngs())
    good = [p.detach().clone() for p in first[0]["net"].parameters()]
    hub_b, ranks_b = _world(2, False, mconf)
    bad = [[E._clone(b) for b in clean[r]] for r in range(2)]
    bad[1][1]["UDiv"][0, 1, 0, 5, 9] = float("nan")
    from fluidnet_amd.run_epoch import run_epoch

    def work(r):
        def f():
            try:
                run_epoch(ranks_b[r]["closure"], bad[r], rng=rngs()[r])
            except TfluidsError as e:
                return str(e)
            return None
        return f
    said = dist.run_virtual(hub_b, [work(r) for r in range(2)])
    for r in range(2):
        assert said[r] is not None and "criterion error is NaN or > 1e9 (first seen at batch 1)" in said[r], said
        assert ranks_b[r]["closure"].first_bad == 1 and ranks_b[r]["opt"].steps == 1
        assert all(torch.equal(a, b.detach()) for a, b in zip(good, ranks_b[r]["net"].parameters())), r
    assert int(ranks_b[0]["closure"].guard.item()) == 0 and int(ranks_b[1]["closure"].guard.item()) == 1
    # run_virtual_closures raises what the ranks raise
    hub_c, ranks_c = _world(2, False, mconf)
    with pytest.raises(TfluidsError, match=r"first seen at batch 1"):
        dist.run_virtual_closures([rk["closure"] for rk in ranks_c], [[E._clone(b) for b in bad[r]] for r in range(2)])


def test_a_torch_optimiser_under_a_comm_is_refused():
    from fluidnet_amd import FluidCriterion, ProjectionNet, TfluidsError, dist
    from fluidnet_amd.run_epoch import Closure
    mconf = E._mconf("manta")
    net = ProjectionNet(R.make_model("default", False), device=DEV).train()
    comm = dist.ThreadComm(dist.ThreadComm.Hub(1), 0)
    with pytest.raises(TfluidsError, match="fused step"):
        Closure(net, FluidCriterion(1.0, 1.0, 1.0), torch.optim.SGD(net.parameters(), lr=0.1), None, mconf, comm=comm)


# ---- 7. sync_parameters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
def test_sync_parameters_gives_every_rank_rank_zeros(is3D):
    from fluidnet_amd import dist
    world = 3
    mconf = E._mconf("manta")
    hub, ranks = _world(world, is3D, mconf, seeds=[3, 4, 5])
    probe = _probe(is3D)
    zero = [p.detach().clone() for p in ranks[0]["net"].parameters()]
    before = [E._snapshot(rk["net"], rk["opt"], probe)[0] for rk in ranks]
    assert not torch.equal(before[0][-1], before[1][-1]) and not torch.equal(before[1][0], before[2][0])
    dist.run_virtual(hub, [rk["closure"].sync_parameters for rk in ranks])
    after = [E._snapshot(rk["net"], rk["opt"], probe)[0] for rk in ranks]
    for r in range(world):
        assert all(torch.equal(a, b.detach()) for a, b in zip(zero, ranks[r]["net"].parameters())), r
        assert _same(after[r], after[0]) and _same(after[r], before[0]), r      # the eval forward included
        assert ranks[r]["net"]._pushed == ranks[r]["net"]._versions()            # the net knows its parameters were pushed


# ---- 8. the native transport, a world of one -----------------------------------------------------------------------------------
def _rccl_comm(like):
    from fluidnet_amd import dist, tfluids
    lib, ctx = tfluids._context(like)
    if not lib.tfl_rccl_available(ctx):
        pytest.skip("no RCCL could be bound: " + lib.tfl_last_error(ctx).decode())
    comm = dist.RcclComm(ctx, dist.RcclComm.unique_id(ctx), 0, 1)
    comm.set_inline(True)      # every nccl* call on the step's own stream, as the slab graph has it
    return comm


def test_rccl_world_of_one_equals_the_guarded_step(monkeypatch):
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    mconf = _optim_mconf("adam", 1, 0.01)
    probe = _probe(False)
    a, b = _single(False, mconf), _single(False, mconf)
    comm = _rccl_comm(a["net"].weights[0])
    try:
        guard = torch.zeros(1, dtype=torch.int32, device=DEV)
        src = _seeded_grads(a["net"], 9)
        for _ in range(2):
            for rank in (a, b):
                for g, s in zip(_flat_grads(rank["net"]), src):
                    g.copy_(s)
            a["opt"].step(guard=guard, comm=comm)
            b["opt"].step(guard=guard)
        got, want = _full(a, probe), _full(b, probe)
        assert got[1] == want[1] == 2 and _same(got[0], want[0])
        assert int(a["opt"].reduced_guard().item()) == 0
    finally:
        torch.cuda.synchronize()
        comm.close()


def test_rccl_world_of_one_captured_and_replayed(monkeypatch):
    """the 2-D net: one eager reduced step, one captured with torch.cuda.graph and replayed twice, against three eager ones"""
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    mconf = _optim_mconf("adam", 1, 0.0)
    probe = _probe(False)
    e, g = _single(False, mconf), _single(False, mconf)
    comm = _rccl_comm(e["net"].weights[0])
    try:
        guard = torch.zeros(1, dtype=torch.int32, device=DEV)
        src = _seeded_grads(e["net"], 9, scale=0.01)      # (the clip does not rewrite them: every step sees the same gradients)
        for rank in (e, g):
            for gr, s in zip(_flat_grads(rank["net"]), src):
                gr.copy_(s)
        for _ in range(3):
            e["opt"].step(guard=guard, comm=comm)
        g["opt"].step(guard=guard, comm=comm)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g["opt"].step(guard=guard, comm=comm)
        assert g["opt"].steps == 1                       # (captured, not run)
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        got, want = _full(g, probe), _full(e, probe)
        assert got[1] == want[1] == 3 and _same(got[0], want[0])
    finally:
        torch.cuda.synchronize()
        comm.close()
