"""The training loop of torch/fluid_net_train.lua:191-247 over a resident data set: fit() runs epochs of run_epoch on a
data.DataBinary, saves the last and the best model and appends to the log; a last-epoch file is a full checkpoint, and
fit(resume=...) continues from it with the bits of the uninterrupted run.

    conf = dict(dataDir=..., dataset=..., ignoreFrames=0, batchSize=16, maxEpochs=10, modelDirname="out/model")
    tr, te = DataBinary(conf, "tr", "cuda:0"), DataBinary(conf, "te", "cuda:0")
    result = fit(conf, mconf, tr, te)

conf (default_conf.lua's names): modelDirname, maxEpochs, batchSize, evaluateDuringTraining (default: whether `te` is given),
lrEpochMults ([{epoch, mult}]), maxSamplesPerEpoch, seed (the loop's one random stream: epoch orders and batch plans).
mconf: the closure's and the optimiser's names (run_epoch.Closure, optim.from_mconf) plus epoch and optimState.bestPerf, both
updated in place. Files, all under the prefix conf["modelDirname"]:
    _lastEpoch.npz   after every epoch: parameters and model description (FluidNetModel.save_npz), mconf, the optimiser's
                     moments, step count and configuration, the epoch, bestPerf and the random stream's state
    .npz             whenever the epoch's test loss is below bestPerf (fluid_net_train.lua:235-239)
    _log.txt         one line per epoch: trLoss trPLoss trULoss trDivLoss trLongTermDivLoss teLoss tePLoss teULoss teDivLoss
                     teLongTermDivLoss (:205-207, :242-245)
Not built: a Torch7 writer (torch.saveModel's format) and optim.sgd.
"""
import json
import os

import numpy as np
import torch

from . import optim as _optim
from ._lib import TfluidsError
from .criterion import FluidCriterion
from .model import FluidNetModel
from .run_epoch import Closure, RandomStateRng, run_epoch
from .train import ProjectionNet

LOG_NAMES = ("trLoss", "trPLoss", "trULoss", "trDivLoss", "trLongTermDivLoss", "teLoss", "tePLoss", "teULoss", "teDivLoss",
             "teLongTermDivLoss")
_PERF = ("aveLoss", "avePLoss", "aveULoss", "aveDivLoss", "aveLongTermDivLoss")


def _jsonable(d):
    return json.loads(json.dumps(d, default=lambda o: o.tolist()))


def save_checkpoint(path, net, optimiser, mconf, rng_state, extra_meta=None):
    """the last-epoch file: save_npz of the net's model with the optimiser's and the loop's state beside it"""
    _ = net.layers      # (brings the host copy up to date with the parameters: one device-to-host copy)
    m, v = optimiser.state()
    kind, keys, pos, has_gauss, cached = rng_state
    meta = dict(mconf=_jsonable(mconf), epoch=int(mconf.get("epoch", 0)),
                bestPerf=float(mconf.get("optimState", {}).get("bestPerf", float("inf"))),
                optim=dict(method=optimiser.method, config=_jsonable(optimiser.config), steps=int(optimiser.steps)),
                rng=dict(kind=kind, pos=int(pos), has_gauss=int(has_gauss), cached_gaussian=float(cached)))
    meta.update(extra_meta or {})
    extra = dict(optim_m=torch.cat([t.reshape(-1) for t in m]).cpu().numpy(), rng_keys=np.asarray(keys, np.uint32))
    if v is not None:
        extra["optim_v"] = torch.cat([t.reshape(-1) for t in v]).cpu().numpy()
    net.net.save_npz(path, meta=meta, extra=extra)


def load_checkpoint(path):
    """(model, meta, arrays) of a last-epoch file: the FluidNetModel, save_checkpoint's meta, and optim_m / optim_v / rng_keys"""
    meta = FluidNetModel.npz_meta(path)
    if not meta or "optim" not in meta or "rng" not in meta:
        raise TfluidsError("%s is not a training checkpoint (no optimiser / random-stream state in it)" % path)
    z = np.load(path)
    arrays = {k: z[k] for k in ("optim_m", "optim_v", "rng_keys") if k in z.files}
    return FluidNetModel.from_npz(path), meta, arrays


def _log_line(trPerf, tePerf):
    return "\t".join("%.8e" % p[k] for p in (trPerf, tePerf) for k in _PERF)


def _module_for(model, device):
    """the ProjectionNet fit() makes by itself: a linear model with pooling / upsampling layers (`tog`) opts in to its training
    pass (ProjectionNet(multires=True)); every other model is wrapped as it always was"""
    g = model.graph      # (a graph of one bank, average pooling and no batch norm is a linear model: tfl_model_create_graph)
    linear = g is None or (g["banksNum"] == 1 and not g["addBatchNorm"] and g["poolType"] == "avg")
    multires = linear and any(v > 1 for v in list(model.pool) + list(model.up))
    return ProjectionNet(model, device=device, multires=multires)


def fit(conf, mconf, tr, te=None, net=None, comm=None, resume=None):
    """Train on `tr` (a data.DataBinary) until mconf["epoch"] reaches conf["maxEpochs"]. Per epoch: the learning-rate
    multipliers of run_epoch.lua:39-48, run_epoch on tr, run_epoch(training=False) on te when evaluateDuringTraining (else tePerf =
    trPerf), bestPerf and the best model, the last-epoch checkpoint, the log line. (bestPerf is updated BEFORE the checkpoint
    is written -- the reference saves first -- so that a resumed run makes the decisions of the uninterrupted one.)
    net: a ProjectionNet (None: a seeded FluidNetModel.from_mconf(mconf, tr.is3D) -- or, resuming, the checkpoint's model).
    comm: a transport of fluidnet_amd.dist; every rank calls fit() with its own net and the same data, seed and conf: the
    ranks take the shards of data.shard_batches, step together (Closure(comm=...)), and rank 0 alone writes files.
    resume: a last-epoch file. Its mconf replaces / updates `mconf`; parameters, moments, step count, epoch, bestPerf and the
    random stream continue where they were, so N epochs straight and K epochs + resume + N - K epochs end with equal bits.
    Returns {net, optimiser, mconf, trPerf, tePerf, epochs (run in this call)}."""
    prefix = conf["modelDirname"]
    rank, world = (0, 1) if comm is None else (int(comm.rank), _optim.comm_world(comm))
    evaluate = bool(conf.get("evaluateDuringTraining", te is not None))
    if evaluate and te is None:
        raise TfluidsError("fit: evaluateDuringTraining needs a test set")
    rs = np.random.RandomState(conf.get("seed"))
    arrays = None
    if resume is not None:
        model, meta, arrays = load_checkpoint(resume)
        if mconf is None:
            mconf = meta["mconf"]
        else:
            mconf.clear()
            mconf.update(meta["mconf"])
        mconf["epoch"] = int(meta["epoch"])
        mconf.setdefault("optimState", {})["bestPerf"] = float(meta["bestPerf"])
        r = meta["rng"]
        rs.set_state((r["kind"], np.asarray(arrays["rng_keys"], np.uint32), int(r["pos"]), int(r["has_gauss"]), float(r["cached_gaussian"])))
        if net is None:
            net = _module_for(model, tr.device)
        else:
            with torch.no_grad():
                for p, (w, b) in zip(zip(net.weights, net.biases), model.layers):
                    p[0].copy_(torch.from_numpy(w))
                    p[1].copy_(torch.from_numpy(b))
    elif mconf is None:
        raise TfluidsError("fit: no mconf and nothing to resume from")
    if net is None:
        net = _module_for(FluidNetModel.from_mconf(mconf, tr.is3D, seed=int(conf.get("modelSeed", 1))), tr.device)
    if net.is3D != tr.is3D:
        raise TfluidsError("Mixing 3D model with 2D data or vice-versa!")
    net.train()
    mconf.setdefault("epoch", 0)
    state = mconf.setdefault("optimState", {})
    state.setdefault("bestPerf", float("inf"))
    crit = FluidCriterion(mconf.get("lossPLambda", 0), mconf.get("lossULambda", 0), mconf.get("lossDivLambda", 0),
                          mconf.get("lossFuncBorderWeight"), mconf.get("lossFuncBorderWidth"))
    opt = _optim.from_mconf(net, mconf)
    if arrays is not None:
        if meta["optim"]["method"] != opt.method:
            raise TfluidsError("fit: the checkpoint's optimiser is not mconf's optimizationMethod")
        opt.load_state(arrays["optim_m"], arrays.get("optim_v"), int(meta["optim"]["steps"]))
    closure = Closure(net, crit, opt, conf, mconf, comm=comm)
    if comm is not None:
        closure.sync_parameters()
    rng = RandomStateRng(rs)
    batchSize, maxSamples = int(conf.get("batchSize", 16)), conf.get("maxSamplesPerEpoch")
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
        if resume is None and os.path.exists(prefix + "_log.txt"):
            os.remove(prefix + "_log.txt")      # (torch.Logger without resumeTraining starts the file again)
    trPerf = tePerf = None
    epochs = 0
    while mconf["epoch"] < int(conf["maxEpochs"]):
        mconf["epoch"] += 1
        for m in conf.get("lrEpochMults", ()):                                                   # run_epoch.lua:39-48
            if mconf["epoch"] == m["epoch"]:
                state["learningRate"] = state.get("learningRate", opt.config["learningRate"]) * m["mult"]
                opt.set_config(learningRate=state["learningRate"])
        trPerf = run_epoch(closure, tr.batches(batchSize, rng, True, maxSamples, rank, world), rng, True)
        if evaluate:
            tePerf = run_epoch(closure, te.batches(batchSize, rng, False, maxSamples, rank, world), rng, False)
        else:
            tePerf = trPerf                                                                      # fluid_net_train.lua:223-227
        best = tePerf["aveLoss"] < state["bestPerf"]
        if best:
            state["bestPerf"] = tePerf["aveLoss"]
        if rank == 0:
            save_checkpoint(prefix + "_lastEpoch.npz", net, opt, mconf, rs.get_state())
            if best:
                net.net.save_npz(prefix + ".npz", meta=dict(mconf=_jsonable(mconf), epoch=int(mconf["epoch"])))
            with open(prefix + "_log.txt", "a") as f:
                f.write(_log_line(trPerf, tePerf) + "\n")
        epochs += 1
    return dict(net=net, optimiser=opt, mconf=mconf, trPerf=trPerf, tePerf=tePerf, epochs=epochs)
