"""The training closure of torch/lib/run_epoch.lua as one call: what the reference does for one mini-batch (:133-330) -- the
random augmentation and time-scale decisions, data augmentation and targets, forward, criterion and backward, the long-term
divergence pass (:240-302: roll the batch forward with the net, score the divergence of the future frame, accumulate its
gradient), the gradient clip and the optimiser step -- sequenced over ProjectionNet, FluidCriterion's kernels, simulate_native
and fluidnet_amd.optim.

    net = ProjectionNet(model).train()
    crit = FluidCriterion(mconf["lossPLambda"], mconf["lossULambda"], mconf["lossDivLambda"])
    closure = Closure(net, crit, optim.from_mconf(net, mconf), conf, mconf)
    stats = run_epoch(closure, batches)                # {"aveLoss": ..., "aveLongTermDivLoss": ...}: one host read

plan_batch() makes the random decisions on the host, in the reference's draw order; Closure.__call__ runs one batch under a
plan; run_epoch() loops the two. The reference reads every loss back to raise on NaN or err > 1e9 (:216-222); here
tfl_closure_fold adds the losses into five sums on the device and sets a sticky guard word instead, and the fused optimiser
step reads that word when it runs (tfl_optim_step_guarded: a set guard leaves parameters, moments and the step counter alone).

What still waits for the device inside a call: tfluids.normalizePressureMean (its component labelling polls a counter), i.e.
every configuration with lossPLambda > 0 or with non-manta targets and the long-term pass on; the PCG target source; and a
torch.optim optimiser (below). Without those a call enqueues launches only and can be captured into a graph.

Data parallel: Closure(..., comm=a transport of fluidnet_amd.dist) on every rank, each with its own net, optimiser and batches.
Both passes of a batch accumulate into the rank's own gradients; the step at the end is the reduced step (optim.step(guard,
comm): one all-reduce of the gradients and the guard), so N ranks with B items each take the step of the mean over N B items.
closure.sync_parameters() first makes the ranks' parameters rank 0's; run_epoch() then returns the means over all ranks' batches.
"""
import ctypes

import numpy as np
import torch

from . import optim as _optim
from . import simulate as _sim
from . import tfluids
from ._lib import TfluidsError
from .train import ProjectionNet

ERR_LIMIT = 1e9          # run_epoch.lua:216
_SUMS = ("aveLoss", "avePLoss", "aveULoss", "aveDivLoss", "aveLongTermDivLoss")      # <- sums5[3], [0], [1], [2], [4]


class RandomStateRng:
    """The default rng of plan_batch over numpy.random.RandomState: uniform() in [0, 1), randint(lo, hi) with BOTH ends
    included (torch.random(lo, hi)), randn() standard normal."""

    def __init__(self, seed=None):
        self._r = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)

    def uniform(self):
        return float(self._r.uniform())

    def randint(self, lo, hi):
        return int(self._r.randint(lo, hi + 1))

    def randn(self):
        return float(self._r.randn())


def _long_term_on(mconf):
    return mconf.get("longTermDivNumSteps") is not None and (mconf.get("longTermDivLambda") or 0) > 0


def plan_batch(mconf, rng=None, training=True):
    """The random decisions of one batch (run_epoch.lua:133-158, 243-258) in the reference's draw order; host code only.
      1. three uniform draws against trainBuoyancyProb, trainGravityProb, trainVorticityConfinementProb: a draw below its
         probability puts the train* value in place of buoyancyScale / gravityScale / vorticityConfinementAmp
      2. if buoyancyScale or gravityScale is then > 0: randint(1, 3), the cardinal axis, and randint(0, 1) * 2 - 1, the sign
      3. if the long-term pass is on (longTermDivNumSteps set, longTermDivLambda > 0) and timeScaleSigma > 0: randn(), and
         dt = dt * (0.2028 + |randn * timeScaleSigma|)
      4. if the long-term pass is on: one uniform draw; above longTermDivProbability it picks longTermDivNumSteps[1], else [0]
    The reference draws the same in training and in evaluation epochs, so `training` changes nothing here. mconf is only read.
    Returns buoyancyScale, gravityScale, vorticityConfinementAmp, gravity (3 floats, or mconf's own where none was drawn), dt
    and numFutureSteps (0: no long-term pass)."""
    rng = RandomStateRng() if rng is None else rng
    plan = dict(buoyancyScale=mconf.get("buoyancyScale") or 0, gravityScale=mconf.get("gravityScale") or 0,
                vorticityConfinementAmp=mconf.get("vorticityConfinementAmp") or 0)
    for key, prob, value in (("buoyancyScale", "trainBuoyancyProb", "trainBuoyancyScale"),
                             ("gravityScale", "trainGravityProb", "trainGravityScale"),
                             ("vorticityConfinementAmp", "trainVorticityConfinementProb", "trainVorticityConfinementAmp")):
        if rng.uniform() < (mconf.get(prob) or 0):
            plan[key] = mconf.get(value) or 0
    gravity = mconf.get("gravity")
    if gravity is not None:
        gravity = [float(v) for v in (gravity.tolist() if hasattr(gravity, "tolist") else gravity)]
    if plan["buoyancyScale"] > 0 or plan["gravityScale"] > 0:
        gravity = [0.0, 0.0, 0.0]
        axis = rng.randint(1, 3)
        gravity[axis - 1] = float(rng.randint(0, 1) * 2 - 1)
    plan["gravity"] = gravity
    plan["dt"] = mconf.get("dt")
    plan["numFutureSteps"] = 0
    if _long_term_on(mconf):
        sigma = mconf.get("timeScaleSigma") or 0
        if sigma > 0:
            plan["dt"] = mconf["dt"] * (0.2028 + abs(rng.randn() * sigma))
        steps = mconf["longTermDivNumSteps"]
        plan["numFutureSteps"] = int(steps[1] if rng.uniform() > (mconf.get("longTermDivProbability") or 0) else steps[0])
    return plan


def _limit_text(limit):
    return ("%g" % limit).replace("e+0", "e").replace("e+", "e")


class Closure:
    """feval of run_epoch.lua:160-316 for one batch, with the optimiser step behind it (:318-324).

    net: a ProjectionNet; criterion: a FluidCriterion (its lambdas as the caller set them score the main pass); optimiser: a
    fluidnet_amd.optim one (the clip is its own fused clip, the step is the guarded step: nothing in the call waits for the
    device) or a torch.optim one over net.parameters() (the closure clips with the formula of :304-312 in torch ops, and READS
    THE GUARD before optimiser.step(): that path synchronises once per call). mconf: the reference's names (trainTargetSource,
    lossPLambda, lossULambda, longTermDivLambda, longTermDivNumSteps, gradNormThreshold, dt, simulate()'s); it is never written.

    __call__(batch, plan, training=True): batch = a dict of device tensors pDiv, UDiv, flags, pTarget, UTarget and optionally
    density / densityDiv and the BC pairs; UDiv, pDiv, the density, pTarget and UTarget are updated in place as the reference
    updates them. In order:
      1. dataAugmentation + calcPUTargets when trainTargetSource is not 'manta' and lossPLambda or lossULambda > 0
      2. normalizePressureMean(pTarget) when lossPLambda > 0
      3. forward (the training forward), criterion, and -- training -- the backward, which OVERWRITES the parameters' .grad
         (zeroGradParameters and the accumulating backward of :203, :233-234 in one)
      4. the long-term pass when plan["numFutureSteps"] > 0: plan["dt"] in force, that many simulate_native steps with the net in
         inference mode, outputDiv on the last; forward on the advanced batch; manta targets: pLambda = uLambda = 0, otherwise
         calcPUTargets + normalizePressureMean; divLambda = longTermDivLambda; criterion, and -- training -- a backward that
         ACCUMULATES
      5. training: the optimiser step
    tfl_closure_fold runs after each criterion call: .sums (float64 [5]: p, u, div, total, long-term total) and .guard (int32
    [1], sticky) live on the device; .loss and .loss_long_term hold the last call's two criterion results (float64 [4] each).
    The criterion's lambdas and net.training are back as they were when the call returns or raises.
    training=False: the same forwards and losses, no backward, no step. (The reference's evaluation epochs still run the
    long-term pass's backward, :292-293, into gradients nobody reads; that stray backward is dropped here.)

    comm: a DistComm, RcclComm or ThreadComm (fluidnet_amd.dist) joining the ranks of a data-parallel world; every rank calls the
    closure together. Step 5 becomes the reduced step: the gradients both passes left in this rank's .grad are averaged over
    the ranks inside it, and .guard_all (int32 [1]) receives the guard it acted on -- set on every rank once any rank's .guard is
    set, from which batch on no rank steps. Needs a fluidnet_amd.optim optimiser: a torch.optim one is refused. The ranks may
    draw different plans (the long-term pass on one and not on another: launches only, nothing collective in it).
    Without a comm, .guard_all is .guard. (training=False under a comm runs nothing collective: .guard_all follows the local
    guard.)"""

    def __init__(self, net, criterion, optimiser, conf, mconf, errLimit=ERR_LIMIT, comm=None):
        if not isinstance(net, ProjectionNet):
            raise TfluidsError("run_epoch.Closure trains a ProjectionNet")
        self.net, self.criterion, self.optimiser, self.conf, self.mconf = net, criterion, optimiser, conf, mconf
        self.fused = isinstance(optimiser, _optim._Fused)
        if self.fused and optimiser.net is not net:
            raise TfluidsError("run_epoch.Closure: the optimiser steps another net")
        if comm is not None and not self.fused:
            raise TfluidsError("run_epoch.Closure: a comm needs a fluidnet_amd.optim optimiser -- the gradient all-reduce lives "
                               "inside its fused step (tfl_optim_step_reduced), and a torch.optim step has no place for it")
        self.comm = comm
        self.errLimit = float(errLimit)
        dev = net.weights[0].device
        self.sums = torch.zeros(5, dtype=torch.float64, device=dev)
        self.guard = torch.zeros(1, dtype=torch.int32, device=dev)
        self.guard_all = self.guard if comm is None else torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(4, dtype=torch.float64, device=dev)
        self.loss_long_term = torch.zeros(4, dtype=torch.float64, device=dev)
        self.first_bad = None      # the batch index at which a poll first saw the guard set (host side: check())

    def reset(self):
        """a new epoch: the sums and the guard back to zero (on the stream, no synchronisation)"""
        self.sums.zero_()
        self.guard.zero_()
        self.guard_all.zero_()
        self.first_bad = None

    def sync_parameters(self):
        """rank 0's parameters to every rank of the comm's world, bit for bit, and the native models refreshed from them
        (optim.sync_parameters: one all-reduce). Collective; call it before the first batch."""
        if self.comm is None:
            raise TfluidsError("run_epoch.Closure.sync_parameters: the closure has no comm")
        self.optimiser.sync_parameters(self.comm)

    def check(self, index=None):
        """reads the guard (synchronises) and raises as run_epoch.lua:216-222 when it is set; index: the batch this poll
        belongs to, named in the message and kept as .first_bad"""
        if self.first_bad is None and int(self.guard_all.item()) != 0:
            self.first_bad = -1 if index is None else int(index)
        self._raise_if_bad()

    def _raise_if_bad(self):
        if self.first_bad is None:
            return
        where = " (first seen at batch %d)" % self.first_bad if self.first_bad >= 0 else ""
        raise TfluidsError("criterion error is NaN or > %s%s" % (_limit_text(self.errLimit), where))

    # -- the pieces ----------------------------------------------------------------------------------------------------
    def _grads(self):
        gw, gb = [], []
        for params, out in ((self.net.weights, gw), (self.net.biases, gb)):
            for p in params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
                out.append(p.grad)
        return gw, gb

    def _score(self, batch, p, U, loss, longTerm, want_grad):
        """criterion forward (+ its gradients to p and U), then the fold"""
        crit, flags = self.criterion, batch["flags"]
        for key in ("pTarget", "UTarget"):
            if batch.get(key) is None:
                raise TfluidsError("run_epoch.Closure: the batch has no %s" % key)
        gP = torch.empty_like(p) if want_grad else None
        gU = torch.empty_like(U) if want_grad else None
        tfluids.fluidCriterion(p, U, batch["pTarget"], batch["UTarget"], flags, crit.weight(flags), float(crit.pLambda),
                               float(crit.uLambda), float(crit.divLambda), bool(crit.sizeAverage), loss, gP, gU)
        crit.pLoss, crit.uLoss, crit.divLoss = loss[0], loss[1], loss[2]
        lib, ctx = tfluids._context(loss)
        tfluids._call(lib, ctx, lib.tfl_closure_fold(ctx, ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(self.sums.data_ptr()),
                                                     ctypes.c_void_p(self.guard.data_ptr()), int(longTerm), self.errLimit))
        return gP, gU

    def _pass(self, batch, loss, longTerm, training, accumulate):
        net, flags = self.net, batch["flags"]
        p, U, tape = net.forward_train(batch["pDiv"], batch["UDiv"], flags)
        gP, gU = self._score(batch, p, U, loss, longTerm, training)
        if training:
            net.backward(flags, gP, gU, tape, out=self._grads(), accumulate=accumulate)

    def _clip_unfused(self):
        """run_epoch.lua:304-312 with torch ops (a torch.optim optimiser): the norm is read back"""
        thr = self.mconf.get("gradNormThreshold")
        if thr is None or not thr > 0:
            return
        grads = [g for pair in zip(*self._grads()) for g in pair]
        norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
        if norm > thr:
            for g in grads:
                g.div_(norm / thr)

    def __call__(self, batch, plan, training=True):
        net, crit = self.net, self.criterion
        m = dict(self.mconf)      # the plan's overrides live in this copy only
        for key in ("buoyancyScale", "gravityScale", "vorticityConfinementAmp", "gravity"):
            m[key] = plan[key]
        manta = m.get("trainTargetSource") == "manta"
        lamP, lamU = m.get("lossPLambda") or 0, m.get("lossULambda") or 0
        is3D = batch["UDiv"].size(1) == 3
        lambdas, was_training = (crit.pLambda, crit.uLambda, crit.divLambda), net.training
        try:
            if not manta and (lamP > 0 or lamU > 0):
                _sim.dataAugmentation(self.conf, m, batch)
                _sim.calcPUTargets(self.conf, m, batch, net)
            if lamP > 0:
                tfluids.normalizePressureMean(batch["pTarget"], batch["flags"], is3D)
            net.train(training)
            self._pass(batch, self.loss, 0, training, accumulate=False)
            if _long_term_on(m) and plan["numFutureSteps"] > 0:
                m["dt"] = plan["dt"]
                net.train(False)
                state = dict(batch)
                if state.get("density") is None:      # simulate.lua:29: batchData.density or batchData.densityDiv
                    state["density"] = batch.get("densityDiv")
                n = int(plan["numFutureSteps"])
                for i in range(1, n + 1):
                    # n steps forward, the last without its pressure projection
                    _sim.simulate_native(self.conf, m, state, net, outputDiv=(i == n))
                net.train(training)
                if manta:
                    crit.pLambda = crit.uLambda = 0      # no pressure or velocity ground truth for the future frame
                else:
                    _sim.calcPUTargets(self.conf, m, batch, net)
                    tfluids.normalizePressureMean(batch["pTarget"], batch["flags"], is3D)
                crit.divLambda = m["longTermDivLambda"]
                self._pass(batch, self.loss_long_term, 1, training, accumulate=True)
        finally:
            crit.pLambda, crit.uLambda, crit.divLambda = lambdas
            net.train(was_training)
        if not training:
            if self.comm is not None:
                self.guard_all.copy_(self.guard)
            return
        if self.comm is not None:
            self.optimiser.step(guard=self.guard, comm=self.comm)
            self.optimiser.reduced_guard(out=self.guard_all)
        elif self.fused:
            self.optimiser.step(guard=self.guard)
        else:
            self.check()
            self._clip_unfused()
            self.optimiser.step()


def run_epoch(closure, batches, rng=None, training=True):
    """plan_batch + closure over an iterable of batches (run_epoch.lua:106-333); returns the epoch means aveLoss, avePLoss,
    aveULoss, aveDivLoss, aveLongTermDivLoss (:345-375) and the batch count `nbatches`. The sums and the guard are read from the
    device ONCE, after the last batch: per batch only an asynchronous copy of the guard word into pinned host memory is
    enqueued, and the final read looks through those copies for the first batch at which the guard was set -- then it raises
    TfluidsError('criterion error is NaN or > 1e9 ...') naming that batch. (From that batch on the guarded step has left the
    parameters alone.)

    With closure.comm (data parallel) every rank calls run_epoch together. The poll copies closure.guard_all, the guard the
    reduced step acted on, so every rank names the same first bad batch. After the last batch the five sums and the batch count
    go through ONE all-reduce: the means are over all ranks' batches and `nbatches` is their total, the same on every rank.
    Every rank must supply EQUALLY MANY batches (each batch is one collective step; a rank that runs out early leaves the others
    waiting in theirs) -- this is not checked. The ranks may draw different plans."""
    rng = RandomStateRng() if rng is None else rng
    closure.reset()
    chunk, polls, n = 1024, [], 0
    for batch in batches:
        plan = plan_batch(closure.mconf, rng, training)
        closure(batch, plan, training)
        if n % chunk == 0:
            polls.append(torch.zeros(chunk, dtype=torch.int32).pin_memory())
        polls[-1][n % chunk:n % chunk + 1].copy_(closure.guard_all, non_blocking=True)
        n += 1
    if n == 0:
        raise TfluidsError("No batches to train / eval on!")
    total = n
    comm = getattr(closure, "comm", None)
    if comm is not None:      # sums and count of every rank: one all-reduce of six doubles, then the one read
        buf = torch.zeros(16, dtype=torch.float32, device=closure.sums.device)
        all6 = buf.view(torch.float64)
        all6[:5].copy_(closure.sums)
        all6[5].fill_(float(n))
        lib, ctx = tfluids._context(buf)      # (the transport's calls are ordered on the context's stream)
        comm.bind(buf)
        comm.error = None
        if comm.struct.allreduce_sum(comm.struct.user, ctypes.c_void_p(buf.data_ptr()), 6) != 0:
            raise comm.error if comm.error is not None else TfluidsError(lib.tfl_last_error(ctx).decode() or "comm callback failed (allreduce_sum)")
        all6 = all6.cpu().numpy()
        sums, total = all6[:5], int(round(float(all6[5])))
    else:
        sums = closure.sums.cpu().numpy()      # the one read: it waits for the stream, so every guard copy has landed too
    for i in range(n):
        if int(polls[i // chunk][i % chunk]) != 0:
            closure.first_bad = i
            break
    closure._raise_if_bad()
    out = {name: float(sums[j] / total) for name, j in zip(_SUMS, (3, 0, 1, 2, 4))}
    out["nbatches"] = total
    return out
