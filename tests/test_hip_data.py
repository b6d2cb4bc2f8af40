"""GPU checks of fluidnet_amd.data.DataBinary against tests/data_ref.py (torch/lib/data_binary.lua in numpy, its divergence the
oracle's) on the same files: the keep / drop decisions of the divergence filter, the sample list, every CreateBatch bit for bit,
the loader's refusals, and run_epoch over ds.batches() with half the frames host-resident against all of them device-resident.
Data sets are written into tmp_path: 2-D 1 x 16 x 16, three runs of 5 frames; 3-D 8 x 8 x 8, two runs of 3."""
import os

import numpy as np
import pytest
import torch

import data_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (is3D, dims, runs = (frames, wall flux, the frame it goes into)): a frame with divergence +0.05 drops its run; a frame whose
# largest divergence is -1 leaves the signed maximum at the noise and its run in
SETS = {
    "2d": (False, (1, 16, 16), [(5, None, -1), (5, (0.05, (0, 7)), 2), (5, (-1.0, (0, 4)), 3)]),
    "3d": (True, (8, 8, 8), [(3, (0.05, (3, 4)), 0), (3, (-1.0, (2, 5)), 1)]),
}
KEPT = {"2d": ["run_000", "run_002"], "3d": ["run_001"]}


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.int32)


@pytest.fixture(scope="module")
def sets(tmp_path_factory, oracle):
    """name -> (conf, DataRef with the oracle's divergence)"""
    def div(U, flags):
        out = np.empty_like(flags)
        oracle.velocityDivergenceForward(np.ascontiguousarray(U), np.ascontiguousarray(flags), out)
        return out
    made = {}
    for name, (is3D, dims, runs) in SETS.items():
        conf = data_ref.write_dataset(str(tmp_path_factory.mktemp(name)), is3D, dims, runs, seed=len(name) + dims[0])
        made[name] = (conf, data_ref.DataRef(conf, "tr", div))
    return made


@pytest.mark.parametrize("name", ["2d", "3d"])
@pytest.mark.parametrize("resident", ["device", "half", "host"])
def test_loader_decisions_and_every_batch_equal_the_restatement(sets, name, resident):
    from fluidnet_amd.data import DataBinary, FrameStore
    conf, ref = sets[name]
    is3D, dims, runs = SETS[name]
    total = sum(r[0] for r in runs)
    rec = FrameStore.record_bytes(is3D, *dims)
    device_bytes = {"device": 32 << 30, "half": rec * (total // 2) + 5, "host": rec - 1}[resident]
    with pytest.warns(UserWarning, match=r"max\(div\) = 0\.05.*above the allowable threshold"):
        ds = DataBinary(conf, "tr", DEV, device_bytes)
    try:
        assert ds.device_frames == {"device": total, "half": total // 2, "host": 0}[resident] and ds.capacity == total
        assert [d[2] for d in ref.decisions] == ["kept" if ("run_%03d" % i) in KEPT[name] else "dropped" for i in range(len(runs))]
        assert [r["dir"] for r in ds.runs] == KEPT[name] == [r["dir"] for r in ref.runs]
        assert ds.runs == ref.runs
        assert np.array_equal(ds.samples, ref.samples) and ds.nsamples() == ref.nsamples()
        assert (ds.is3D, ds.zdim, ds.ydim, ds.xdim) == (is3D,) + dims == (ref.is3D, ref.zdim, ref.ydim, ref.xdim)
        n = ds.nsamples()
        batch = ds.AllocateBatchMemory(4)
        assert sorted(batch) == sorted(data_ref.KEYS)
        empty = torch.empty_like(batch["flags"])
        from fluidnet_amd import tfluids
        tfluids.emptyDomain(empty, is3D)
        assert torch.equal(batch["flags"], empty) and all(float(batch[k].abs().max()) == 0.0 for k in data_ref.KEYS if k != "flags")
        order = list(np.random.RandomState(1).permutation(n))
        for i in range(0, n, 4):                           # every sample once; the last batch is partial
            ids = order[i:i + 4]
            got, want = ds.CreateBatch(batch, ids), ref.create_batch(ids)
            for k in data_ref.KEYS:
                assert got[k].shape == want[k].shape and got[k].data_ptr() == batch[k].data_ptr(), k      # narrowed views
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, ids)
        assert n % 4 != 0 and got["pDiv"].size(0) == n % 4
    finally:
        ds.close()


def test_loader_refusals_name_the_file(tmp_path):
    from fluidnet_amd import TfluidsError, io
    from fluidnet_amd.data import DataBinary
    conf = data_ref.write_dataset(str(tmp_path), False, (1, 16, 16), [(2, None, -1), (2, None, -1)])
    base = os.path.join(conf["dataDir"], conf["dataset"], "tr")
    bad = os.path.join(base, "run_001", "000001_divergent.bin")
    p, U, flags, density, _ = io.loadMantaFile(bad)
    flags2 = flags.copy()
    flags2[0, 0, 0, 5, 5] = 2.0
    io.saveMantaFile(bad, p, U, flags2, density)
    with pytest.raises(TfluidsError, match=r"Flags changed.*run_001.000001_divergent\.bin"):
        DataBinary(conf, "tr", DEV)
    io.saveMantaFile(bad, p, U, flags, density)
    # another grid in the second run
    other = data_ref.solenoidal_frame(np.random.RandomState(0), False, (1, 16, 20))
    data_ref.write_frame(os.path.join(base, "run_001"), 1, other, other)
    with pytest.raises(TfluidsError, match=r"frame dims .* differ .*run_001.000001\.bin"):
        DataBinary(conf, "tr", DEV)
    # a 3-D frame among 2-D ones
    other = data_ref.solenoidal_frame(np.random.RandomState(0), True, (4, 16, 16))
    data_ref.write_frame(os.path.join(base, "run_001"), 1, other, other)
    with pytest.raises(TfluidsError, match=r"inconsistent 3D flags across run files .*run_001.000001\.bin"):
        DataBinary(conf, "tr", DEV)
    with pytest.raises(TfluidsError, match="there is no CPU path"):
        DataBinary(conf, "tr", "cpu")


def _mconf():
    return dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0, gravityScale=0,
                vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource="manta", maxIter=12,
                lossPLambda=1.0, lossULambda=1.0, lossDivLambda=1.0, longTermDivLambda=1, longTermDivNumSteps=[1, 2],
                longTermDivProbability=0.5, timeScaleSigma=1, trainBuoyancyProb=0.5, trainBuoyancyScale=2.0, trainGravityProb=0.5,
                trainGravityScale=1.0, trainVorticityConfinementProb=0.5, trainVorticityConfinementAmp=0.8,
                optimizationMethod="adam", gradNormThreshold=1,
                optimState=dict(learningRate=0.0025, weightDecay=0, learningRateDecay=0, epsilon=0.0001, beta1=0.9, beta2=0.999))


def test_an_epoch_over_host_resident_frames_has_the_bits_of_a_device_resident_one(sets):
    """run_epoch(closure, ds.batches(...)) on the 2-D set, batch size 4 (10 samples: the last batch holds 2): half the frames in
    pinned host memory against all of them in HBM -- the same epoch means and the same parameters, bit for bit"""
    from fluidnet_amd import FluidCriterion, FluidNetModel, ProjectionNet, optim
    from fluidnet_amd.data import DataBinary, FrameStore
    from fluidnet_amd.run_epoch import Closure, RandomStateRng, run_epoch
    conf, _ = sets["2d"]
    rec = FrameStore.record_bytes(False, 1, 16, 16)
    results = []
    for device_bytes in (32 << 30, rec * 7):
        with pytest.warns(UserWarning):
            ds = DataBinary(conf, "tr", DEV, device_bytes)
        try:
            assert ds.device_frames == (15 if device_bytes > rec * 15 else 7)
            mconf = _mconf()
            net = ProjectionNet(FluidNetModel.from_mconf(dict(modelType="default"), False, seed=2), device=DEV).train()
            opt = optim.from_mconf(net, mconf)
            closure = Closure(net, FluidCriterion(1.0, 1.0, 1.0), opt, None, mconf)
            rng = RandomStateRng(7)
            stats = run_epoch(closure, ds.batches(4, rng), rng)
            assert stats["nbatches"] == 3 and np.isfinite(stats["aveLoss"]) and stats["aveLongTermDivLoss"] > 0
            results.append((stats, [p.detach().clone() for p in net.parameters()], opt.steps))
        finally:
            ds.close()
    (sa, pa, ta), (sb, pb, tb) = results
    assert sa == sb and ta == tb == 3
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
