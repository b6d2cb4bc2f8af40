#!/usr/bin/env python
"""examples/train.py -- the reference's training driver (torch/fluid_net_train.lua) on the MI355X path.

Trains a projection ConvNet from a data set in the reference's layout, <dataDir>/<dataset>/{tr,te}/<run>/NNNNNN.bin +
NNNNNN_divergent.bin (manta's scenes/_trainingData.py): both sets are loaded once into resident frame stores
(fluidnet_amd.data.DataBinary), every mini-batch is one gather launch, every training step one fused device call
(fluidnet_amd.run_epoch), and fluidnet_amd.train_loop.fit writes <out>_lastEpoch.npz (a full checkpoint), <out>.npz (the best
model so far; FluidNetModel.from_npz loads it) and <out>_log.txt.

  python examples/train.py --dataDir data/datasets --dataset output_current_model_sphere --out /tmp/fit/model \\
        [--modelType default|yang|tog] [--epochs 10] [--batchSize 16] [--resume /tmp/fit/model_lastEpoch.npz]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidnet_amd.data import DataBinary  # noqa: E402
from fluidnet_amd.train_loop import fit  # noqa: E402


def default_mconf(modelType, longTerm):
    """torch/lib/default_conf.lua:40-130's newModel table, the fields the closure and the optimiser read"""
    return dict(modelType=modelType, dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0,
                gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet",
                trainTargetSource="manta", maxIter=34, lossFunc="fluid", lossPLambda=0, lossULambda=0, lossDivLambda=1,
                lossFuncBorderWeight=1, lossFuncBorderWidth=3,
                longTermDivLambda=0.25 if longTerm else 0, longTermDivNumSteps=[4, 16], longTermDivProbability=0.9,
                timeScaleSigma=1, trainBuoyancyProb=0.3, trainBuoyancyScale=2.0, trainGravityProb=0, trainGravityScale=0,
                trainVorticityConfinementProb=0.3, trainVorticityConfinementAmp=8 / 9.0,
                optimizationMethod="adam", gradNormThreshold=1, epoch=0,
                optimState=dict(bestPerf=float("inf"), learningRate=0.0025, weightDecay=0, learningRateDecay=0, epsilon=0.0001,
                                beta1=0.9, beta2=0.999))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataDir", required=True, help="holds <dataset>/{tr,te}/...; examples/gen_data.py generates such a set")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--out", required=True, help="conf.modelDirname: the prefix of the files written")
    ap.add_argument("--modelType", default="default", choices=("default", "yang", "tog"))
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batchSize", type=int, default=16)
    ap.add_argument("--ignoreFrames", type=int, default=0)
    ap.add_argument("--maxSamplesPerEpoch", type=int, default=None)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--device-bytes", type=int, default=32 << 30, help="HBM a frame store may take; the rest is pinned host memory")
    ap.add_argument("--no-long-term", action="store_true", help="longTermDivLambda = 0: no rollout pass")
    ap.add_argument("--no-eval", action="store_true", help="evaluateDuringTraining = false: no test set is loaded")
    ap.add_argument("--resume", default=None, help="a _lastEpoch.npz to continue from")
    ap.add_argument("--pcgBatched", action="store_true",
                    help="mconf.pcgBatched: where trainTargetSource = 'pcg', calcPUTargets solves all batch items in the same "
                         "launches ('mg'); without --resume only, a resumed run keeps its saved mconf")
    a = ap.parse_args()
    conf = dict(dataDir=a.dataDir, dataset=a.dataset, ignoreFrames=a.ignoreFrames, batchSize=a.batchSize, maxEpochs=a.epochs,
                modelDirname=a.out, evaluateDuringTraining=not a.no_eval, maxSamplesPerEpoch=a.maxSamplesPerEpoch, seed=a.seed,
                lrEpochMults=[])
    tr = DataBinary(conf, "tr", a.device, a.device_bytes)
    te = None if a.no_eval else DataBinary(conf, "te", a.device, a.device_bytes)
    print("==> loaded %d training samples (%s, %d x %d x %d), %d of %d frames in HBM"
          % (tr.nsamples(), "3D" if tr.is3D else "2D", tr.zdim, tr.ydim, tr.xdim, tr.device_frames, tr.capacity))
    mconf = None if a.resume else default_mconf(a.modelType, not a.no_long_term)
    if mconf is not None and a.pcgBatched:
        mconf["pcgBatched"] = True
    out = fit(conf, mconf, tr, te, resume=a.resume)
    print("==> %d epochs run, now at epoch %d: trLoss %.4e teLoss %.4e, bestPerf %.4e"
          % (out["epochs"], out["mconf"]["epoch"], (out["trPerf"] or {}).get("aveLoss", float("nan")),
             (out["tePerf"] or {}).get("aveLoss", float("nan")), out["mconf"]["optimState"]["bestPerf"]))
    print("    files: %s{_lastEpoch.npz,.npz,_log.txt}" % os.path.abspath(a.out))


if __name__ == "__main__":
    main()
