"""GPU checks of the data-set generator (fluidnet_amd/datagen.py, csrc/datagen.hip): the scene and noise kernels
against the numpy restatement of tests/datagen_ref.py bit for bit; generate() into a frame store against the definition's
two-call restatement (copy the state, simulate(outputDiv=True) on the copy, simulate on the state) bit for bit, twice the same,
one run at a time or together, the disk sink loaded by DataBinary equal to the store, no run dropped; and train_loop.fit on a
generated in-memory set lowers its training loss."""
import numpy as np
import pytest
import torch

import datagen_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)).view(np.int32)


@pytest.mark.parametrize("dims", [(1, 9, 33), (5, 7, 19)], ids=["2d", "3d"])
def test_scene_and_noise_kernels_equal_the_restatement_bit_for_bit(oracle, dims):
    from fluidnet_amd import datagen, tfluids
    Z, Y, X = dims
    is3D = Z > 1
    C, Cpsi = (3, 3) if is3D else (2, 1)
    # the rasteriser: spheres and boxes whose surfaces pass through cell centres' neighbourhood at odd fractions
    obstacles = [dict(kind=0, a=[7.3, 3.9, 2.2], b=[1.7, 0, 0], val=0.0), dict(kind=1, a=[20.25, 2.5, 1.0], b=[25.5, 5.75, 3.5], val=0.0),
                 dict(kind=0, a=[14.5, 4.5, 2.5], b=[0.5, 0, 0], val=0.0)]
    blobs = [dict(kind=0, a=[9.1, 4.2, 2.4], b=[3.3, 0, 0], val=0.625), dict(kind=1, a=[12.0, 1.0, 1.0], b=[22.0, 4.0, 3.0], val=0.3),
             dict(kind=0, a=[13.0, 3.0, 2.0], b=[2.0, 0, 0], val=0.9)]
    flags = torch.full((2, 1) + dims, -1.0, device=DEV)
    density = torch.full((2, 1) + dims, -1.0, device=DEV)
    datagen.scene_flags(obstacles, blobs, is3D, flags, density)
    want_f, want_d = R.scene_flags(obstacles, blobs, is3D, dims)
    for b in range(2):
        assert np.array_equal(_bits(flags[b]), _bits(want_f[0])) and np.array_equal(_bits(density[b]), _bits(want_d[0]))
    assert 0 < int((want_f == 2).sum()) - int((R.scene_flags([], [], is3D, dims)[0] == 2).sum()) and len(np.unique(want_d)) == 4
    empty = torch.empty((1, 1) + dims, device=DEV)
    datagen.scene_flags([], [], is3D, empty)
    assert torch.equal(empty, tfluids.emptyDomain(torch.empty_like(empty), is3D))
    # the noise: item b is run + b
    psi = torch.empty((2, Cpsi) + dims, device=DEV)
    datagen.noise_potential(0xfffffffe, 41, psi)
    want_psi = R.noise_field(0xfffffffe, 41, Cpsi, dims, B=2)
    assert np.array_equal(_bits(psi), _bits(want_psi))
    one = torch.empty((1, Cpsi) + dims, device=DEV)
    datagen.noise_potential(0xfffffffe, 42, one)
    assert torch.equal(one[0], psi[1])
    # blur (the existing operator, against the oracle's) and curl
    sm, sm_ref = torch.empty_like(one), np.empty_like(want_psi[1:])
    tfluids.rectangularBlur(one, 2, is3D, sm)
    oracle.rectangularBlur(np.ascontiguousarray(want_psi[1:]), 2, is3D, sm_ref)
    assert np.array_equal(_bits(sm), _bits(sm_ref))
    for amp in (1.0, 0.37):
        U = torch.empty((1, C) + dims, device=DEV)
        datagen.curl_mac(sm, amp, is3D, U)
        assert np.array_equal(_bits(U), _bits(R.curl_mac(sm_ref, amp, is3D))), amp
    # the whole initial velocity of a plan
    plan = datagen.plan_run(datagen.default_gconf(is3D, dims), 3, 0)
    U0, amp = datagen.initial_velocity(plan, DEV)
    want_U0, want_amp = R.initial_velocity(oracle, plan, datagen.noise_seed(plan))
    assert amp == want_amp and np.array_equal(_bits(U0), _bits(want_U0))
    assert abs(float(U0.abs().max()) - plan["speed"]) <= 1e-6 * plan["speed"]


def test_scene_kernels_refuse_by_name():
    from fluidnet_amd import TfluidsError, datagen
    flags = torch.empty(1, 1, 1, 8, 8, device=DEV)
    with pytest.raises(TfluidsError, match="at most 32"):
        datagen.scene_flags([dict(kind=0, a=[4, 4, 0], b=[1, 0, 0], val=0.0)] * 33, [], False, flags)
    with pytest.raises(TfluidsError, match="unknown kind"):
        datagen.scene_flags([dict(kind=2, a=[4, 4, 0], b=[1, 0, 0], val=0.0)], [], False, flags)
    with pytest.raises(TfluidsError, match="channels"):
        datagen.curl_mac(torch.empty(1, 3, 1, 8, 8, device=DEV), 1.0, False, torch.empty(1, 2, 1, 8, 8, device=DEV))
    with pytest.raises(TfluidsError, match="CPU tensor"):
        datagen.noise_potential(1, 2, torch.empty(1, 1, 1, 8, 8))


@pytest.fixture(scope="module", params=R.GEN_CASES, ids=["2d", "3d"])
def generated(request, tmp_path_factory):
    """(is3D, dims, gconf, store, result, out_dir): 2 runs x 6 saved frames into a store (half of it host-mapped) and onto the disk"""
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    is3D, dims = request.param
    g = R.gen_gconf(is3D, dims)
    out = str(tmp_path_factory.mktemp("gen") / "sets" / "mine")
    store = FrameStore(DEV, is3D, *dims, 12, 6)
    res = datagen.generate(g, "tr", R.GEN_RUNS, R.GEN_SEED, out_dir=out, store=store, device=DEV)
    yield is3D, dims, g, store, res, out
    store.close()


def _gather_all(store, is3D, dims, n):
    C = 3 if is3D else 2
    out = {k: torch.empty((n, C if k in ("UDiv", "UTarget") else 1) + tuple(dims), device=DEV) for k in KEYS}
    store.gather(range(n), out)
    return out


def test_generate_equals_the_two_call_restatement_and_drops_no_run(generated):
    from fluidnet_amd import datagen
    from fluidnet_amd.simulate import simulate
    is3D, dims, g, store, res, _ = generated
    assert res["runs"] == [("000000", 6), ("000001", 6)]
    assert [(r["run"], r["attempt"], r["kept"]) for r in res["report"]] == [(0, 0, True), (1, 0, True)], res["report"]
    print("max div(U target) per run:", [r["max_div"] for r in res["report"]])
    got = _gather_all(store, is3D, dims, 12)
    slot = 0
    for run in range(R.GEN_RUNS):
        plan = datagen.plan_run(g, R.GEN_SEED, run)
        batch, mconf = datagen.init_state(plan, DEV), datagen.mconf_of(plan)
        for k in range(g["steps"]):
            if k % g["saveEvery"] == 0:
                cp = {key: (v.clone() if key in ("pDiv", "UDiv", "density") else v) for key, v in batch.items()}
                simulate(None, mconf, cp, None, outputDiv=True)
            simulate(None, mconf, batch, None)
            if k % g["saveEvery"] == 0:
                want = dict(pDiv=cp["pDiv"], UDiv=cp["UDiv"], flags=batch["flags"], densityDiv=cp["density"], pTarget=batch["pDiv"],
                            UTarget=batch["UDiv"], densityTarget=batch["density"])
                for key in KEYS:
                    assert torch.equal(got[key][slot], want[key][0]), (run, k, key)
                slot += 1
        # the run moved and carried smoke: a frame pair is not a pair of equal frames
        assert float((got["UTarget"][slot - 1] - got["UDiv"][slot - 1]).abs().max()) > 0
        assert float(got["densityTarget"][slot - 1].max()) > 0.1
    assert slot == 12


def test_the_same_seed_gives_the_same_bits_one_run_at_a_time_or_together(generated):
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    is3D, dims, g, store, res, _ = generated
    got = _gather_all(store, is3D, dims, 12)
    again = FrameStore(DEV, is3D, *dims, 12, 0)
    single = FrameStore(DEV, is3D, *dims, 6, 6)
    try:
        datagen.generate(g, "tr", R.GEN_RUNS, R.GEN_SEED, store=again, device=DEV)
        twice = _gather_all(again, is3D, dims, 12)
        for key in KEYS:
            assert torch.equal(twice[key], got[key]), key
        datagen.generate(g, "tr", 1, R.GEN_SEED, store=single, device=DEV, first_run=1)
        alone = _gather_all(single, is3D, dims, 6)
        for key in KEYS:
            assert torch.equal(alone[key], got[key][6:]), key
        other = datagen.generate(g, "tr", 1, R.GEN_SEED + 1, store=single, device=DEV)
        assert not torch.equal(_gather_all(single, is3D, dims, 6)["UTarget"], got["UTarget"][:6]) and other["runs"] == [("000000", 6)]
    finally:
        again.close()
        single.close()


def test_the_disk_sink_loaded_by_databinary_equals_the_store(generated):
    import os
    from fluidnet_amd.data import DataBinary
    is3D, dims, g, store, res, out = generated
    conf = dict(dataDir=os.path.dirname(out), dataset=os.path.basename(out), ignoreFrames=0)
    disk = DataBinary(conf, "tr", DEV)
    try:
        mem = res["data"]
        assert disk.nsamples() == mem.nsamples() == 12 and np.array_equal(disk.samples, mem.samples)
        assert [r["dir"] for r in disk.runs] == [r["dir"] for r in mem.runs] == ["000000", "000001"]
        assert (disk.is3D, disk.zdim, disk.ydim, disk.xdim) == (mem.is3D, mem.zdim, mem.ydim, mem.xdim)
        a = disk.CreateBatch(disk.AllocateBatchMemory(12), range(12))
        b = mem.CreateBatch(mem.AllocateBatchMemory(12), range(12))
        for key in KEYS:
            assert torch.equal(a[key], b[key]), key
        ids = [s for batch in mem.batches(5, training=False) for s in range(batch["UDiv"].size(0))]
        assert len(ids) == 12
    finally:
        disk.close()


def test_fit_on_a_generated_in_memory_set_lowers_the_training_loss(tmp_path):
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    from fluidnet_amd.train_loop import fit
    dims = (1, 32, 32)
    g = R.gen_gconf(False, dims)
    store = FrameStore(DEV, False, *dims, 12, 12)
    try:
        tr = datagen.generate(g, "tr", R.GEN_RUNS, R.GEN_SEED, store=store, device=DEV)["data"]
        mconf = dict(modelType="default", dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0,
                     gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource="manta",
                     maxIter=12, lossPLambda=0, lossULambda=1.0, lossDivLambda=1.0, longTermDivLambda=0, longTermDivNumSteps=None,
                     longTermDivProbability=0.5, timeScaleSigma=1, trainBuoyancyProb=0, trainBuoyancyScale=2.0, trainGravityProb=0,
                     trainGravityScale=1.0, trainVorticityConfinementProb=0, trainVorticityConfinementAmp=0.8,
                     optimizationMethod="adam", gradNormThreshold=1, epoch=0,
                     optimState=dict(bestPerf=float("inf"), learningRate=0.0025, weightDecay=0, learningRateDecay=0, epsilon=0.0001,
                                     beta1=0.9, beta2=0.999))
        conf = dict(modelDirname=str(tmp_path / "m" / "model"), maxEpochs=3, batchSize=4, seed=5, evaluateDuringTraining=False)
        res = fit(conf, mconf, tr)
        lines = open(conf["modelDirname"] + "_log.txt").read().splitlines()
        assert res["epochs"] == 3 and len(lines) == 3
        first, last = float(lines[0].split("\t")[0]), float(lines[2].split("\t")[0])      # trLoss of epochs 1 and 3
        print("training loss: epoch 1 %.6e, epoch 3 %.6e" % (first, last))
        assert np.isfinite(first) and np.isfinite(last) and last < first
    finally:
        store.close()


def test_velocity_emitters_run_through_generate_as_a_ubc_pair():
    """emitterSpeed > 0: the emitters carry a UBC pair besides the densityBC pair (re-imposed after the projection, so the target
    is not divergence-free on their surface: divThreshold = None). One 2-D run whose plan holds an emitter, against the two-call
    restatement bit for bit; the emitter's cells hold its velocity and density in every target frame."""
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    from fluidnet_amd.simulate import simulate
    dims = (1, 32, 32)
    g = datagen.default_gconf(False, dims, steps=6, saveEvery=2, emitterSpeed=0.5, divThreshold=None)
    run = next(r for r in range(64) if datagen.plan_run(g, R.GEN_SEED, r)["emitters"])
    plan = datagen.plan_run(g, R.GEN_SEED, run)
    R.check_plan(plan)
    (ubc, umk), (dbc, dmk) = datagen.emitter_pairs(plan)
    assert ubc is not None and dbc is not None and float(np.abs(ubc).max()) > 0.5
    store = FrameStore(DEV, False, *dims, 3, 3)
    try:
        res = datagen.generate(g, "tr", 1, R.GEN_SEED, store=store, device=DEV, first_run=run)
        assert res["runs"] == [("%06d" % run, 3)] and [r["kept"] for r in res["report"]] == [True]
        print("velocity emitters: max div(U target) = %.3e" % res["report"][0]["max_div"])
        got = _gather_all(store, False, dims, 3)
        batch, mconf = datagen.init_state(plan, DEV), datagen.mconf_of(plan)
        assert "UBC" in batch and "densityBC" in batch
        slot = 0
        for k in range(g["steps"]):
            if k % g["saveEvery"] == 0:
                cp = {key: (v.clone() if key in ("pDiv", "UDiv", "density") else v) for key, v in batch.items()}
                simulate(None, mconf, cp, None, outputDiv=True)
            simulate(None, mconf, batch, None)
            if k % g["saveEvery"] == 0:
                want = dict(pDiv=cp["pDiv"], UDiv=cp["UDiv"], flags=batch["flags"], densityDiv=cp["density"], pTarget=batch["pDiv"],
                            UTarget=batch["UDiv"], densityTarget=batch["density"])
                for key in KEYS:
                    assert torch.equal(got[key][slot], want[key][0]), (k, key)
                slot += 1
        inside = torch.from_numpy(umk[0] == 0).to(DEV)
        for f in range(3):
            assert torch.equal(got["UTarget"][f][inside], torch.from_numpy(ubc[0]).to(DEV)[inside])
            assert torch.equal(got["densityTarget"][f][torch.from_numpy(dmk[0] == 0).to(DEV)], torch.from_numpy(dbc[0]).to(DEV)[torch.from_numpy(dmk[0] == 0).to(DEV)])
    finally:
        store.close()
