"""GPU checks of every projection net lib/model.lua's defineModelGraph builds (tfl_model_create_graph): resolution and
dilated banks, their concat / add join, inference-form batch norm and max pooling, against the PyTorch-CPU restatement
in tests/model_graph_ref.py (tolerance and fp64 witness as test_hip_simulate.py's tog test)."""
import numpy as np
import pytest

import model_graph_ref as R
import scenes
from flavours import experiments_flavour

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _check(oracle, model, dims, seed=31):
    import torch
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(dims, seed=seed, vel_cells=0.4, B=2)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    p, U = model.forward([tp, tU, tf])
    p_ref, U_ref = R.model_forward(oracle, model, sc["p"], sc["U"], sc["flags"])
    rp, rU = scenes.rel_l2(p.cpu().numpy(), p_ref), scenes.rel_l2(U.cpu().numpy(), U_ref)
    assert rp <= TOL and rU <= TOL, (rp, rU)
    assert float(np.abs(p_ref).max()) > 0
    p64, _ = R.model_forward(oracle, model, sc["p"], sc["U"], sc["flags"], conv_dtype="float64")
    assert scenes.rel_l2(p.cpu().numpy(), p64) <= 4 * scenes.rel_l2(p_ref, p64) + 1e-7


def _mconf(n, bt, agg, bn, **kw):
    m = dict(banksNum=n, banksType=bt, banksAggregateMethod=agg, banksSplitStage=2, banksJoinStage=4)
    m.update(kw)
    if bn != "off":
        m.update(addBatchNorm=True, batchNormAffine=bn == "affine")
    return m


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("bt", ["mres", "dilate"])
@pytest.mark.parametrize("agg", ["concat", "add"])
@pytest.mark.parametrize("bn", ["off", "affine", "plain"])
def test_banks_3d(oracle, n, bt, agg, bn):
    from fluidnet_amd import FluidNetModel
    _check(oracle, FluidNetModel.from_mconf(_mconf(n, bt, agg, bn), True, seed=n), (16, 24, 32))


@pytest.mark.parametrize("n,bt,agg,bn", [(2, "mres", "concat", "affine"), (3, "dilate", "add", "plain"),
                                         (2, "dilate", "concat", "off"), (3, "mres", "add", "affine")])
def test_banks_2d(oracle, n, bt, agg, bn):
    from fluidnet_amd import FluidNetModel
    _check(oracle, FluidNetModel.from_mconf(_mconf(n, bt, agg, bn), False, seed=7), (1, 64, 96))


@pytest.mark.parametrize("bt", ["mres", "dilate"])
def test_banks_3d_cube(oracle, bt):
    from fluidnet_amd import FluidNetModel
    _check(oracle, FluidNetModel.from_mconf(_mconf(3, bt, "concat", "affine", banksSplitStage=1, banksJoinStage=3), True, seed=2),
           (32, 32, 32))


@pytest.mark.parametrize("is3d,dims", [(True, (32, 32, 32)), (False, (1, 64, 96))])
def test_tog_banks_max_pool(oracle, is3d, dims):
    from fluidnet_amd import FluidNetModel
    mc = dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5, poolType="max", addBatchNorm=True)
    _check(oracle, FluidNetModel.from_mconf(mc, is3d, seed=9), dims)


@pytest.mark.parametrize("is3d,dims", [(True, (16, 24, 32)), (False, (1, 64, 96))])
def test_yang_batch_norm(oracle, is3d, dims):
    from fluidnet_amd import FluidNetModel
    _check(oracle, FluidNetModel.from_mconf(dict(modelType="yang", addBatchNorm=True), is3d, seed=4), dims)


def test_non_default_opts(oracle):
    from fluidnet_amd import FluidNetModel
    mc = _mconf(2, "dilate", "concat", "affine", nonlinType="relu6", normalizeInputChan="pDiv", addPressureSkip=True,
                inputChannels=dict(UDiv=True))
    _check(oracle, FluidNetModel.from_mconf(mc, True, seed=6), (16, 24, 32))


@experiments_flavour
def test_banks_against_the_experiments_flavour(oracle):
    from fluidnet_amd import FluidNetModel
    _check(oracle, FluidNetModel.from_mconf(_mconf(3, "mres", "concat", "affine"), True, seed=3), (16, 24, 32))


@pytest.mark.parametrize("is3d,dims", [(True, (16, 24, 32)), (False, (1, 64, 96))])
def test_trivial_graph_is_the_plain_model(is3d, dims):
    """One bank, no BN, average pooling: tfl_model_create_graph builds what tfl_model_create_opts builds (the 3-D default
    topology on its MFMA path) -- the same bits."""
    import torch
    from fluidnet_amd import FluidNetModel
    dev = torch.device("cuda:0")
    base = FluidNetModel.from_mconf({}, is3d, seed=1)
    g = FluidNetModel(base.layers, is3d, graph=dict(banksNum=1, poolType="avg", addBatchNorm=False))
    sc = scenes.make_scene(dims, seed=5, vel_cells=0.4, B=2)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    a, b = base.forward([tp, tU, tf]), g.forward([tp, tU, tf])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("bt,agg,joins", [("mres", "concat", 1), ("mres", "add", 1), ("dilate", "add", 1), ("dilate", "concat", 0)])
def test_launch_structure(bt, agg, joins):
    """No launch for BN; one join launch per forward (none when every bank writes its own concat slice); banksNum - 1
    pyramid launches for mres."""
    import torch
    from fluidnet_amd import FluidNetModel, tfluids
    dev = torch.device("cuda:0")
    n = 3
    model = FluidNetModel.from_mconf(_mconf(n, bt, agg, "affine"), True, seed=1)
    sc = scenes.make_scene((16, 24, 32), seed=5, vel_cells=0.4, B=1)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    model.forward([tp, tU, tf])
    with tfluids.profile(tU) as prof:
        model.forward([tp, tU, tf])
    k = prof.kernels
    calls = lambda name: k.get(name, {}).get("calls", 0)      # noqa: E731
    assert calls("k_conv_direct_ex") == len(model.layers)     # one per conv module (none has up > 1)
    assert calls("k_bank_join") == joins
    assert calls("k_avg_pool2") == (n - 1 if bt == "mres" else 0)
    assert calls("k_pool2_ex") == 0 and calls("k_conv_direct") == 0
    assert not any("bn" in name.lower() or "batch" in name.lower() for name in k)


def _plume(dims, dev):
    import test_hip_simulate as T
    return T._to_dev(T._plume_batch(dims, 0.15, 1.0, obstacles_seed=7), dev)


def test_native_step_with_banked_bn_model():
    """tfl_simulate_step with a banked + BN model equals the Python simulate() orchestration bit for bit, and a captured
    graph of the step replays the eager steps."""
    import torch
    from fluidnet_amd import FluidNetModel
    from fluidnet_amd.simulate import GraphedSimulate, simulate, simulate_native
    dev = torch.device("cuda:0")
    model = FluidNetModel.from_mconf(_mconf(2, "mres", "concat", "affine"), True, seed=5)
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.5, gravityScale=0,
                 vorticityConfinementAmp=1.0, simMethod="convnet")
    ta, tb, tc = _plume((16, 24, 32), dev), _plume((16, 24, 32), dev), _plume((16, 24, 32), dev)
    gn = GraphedSimulate(None, mconf, tc, model, native=True)       # the one-call native step, captured and replayed
    for _ in range(3):
        simulate(None, mconf, ta, model)
        simulate_native(None, mconf, tb, model)
        gn.step()
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(ta[k], tb[k]), k
        assert torch.equal(ta[k], tc[k]), ("graph", k)
    assert float(ta["UDiv"].abs().max()) > 0.1


def test_slab_step_refuses_graph_models_before_writing():
    import torch
    from fluidnet_amd import FluidNetModel, TfluidsError
    from fluidnet_amd.dist import SlabLayout, SlabSimulation
    dev = torch.device("cuda:0")
    model = FluidNetModel.from_mconf(_mconf(2, "dilate", "add", "affine"), True, seed=5)
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.5, gravityScale=0,
                 vorticityConfinementAmp=0, simMethod="convnet")
    ref = _plume((16, 24, 32), dev)
    lay = SlabLayout(16, 1, 0, 1)
    loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
    sim = SlabSimulation(loc, mconf, model, lay, None, own_context=True)
    before = {k: sim.batch[k].clone() for k in ("pDiv", "UDiv", "density")}
    with pytest.raises(TfluidsError, match="un-sharded"):
        sim.step(eager=True)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(sim.batch[k], v), k


def test_grid_not_divisible_is_refused():
    import torch
    from fluidnet_amd import FluidNetModel, TfluidsError
    dev = torch.device("cuda:0")
    model = FluidNetModel.from_mconf(_mconf(3, "mres", "concat", "off"), True, seed=1)     # pyramid factor 4
    sc = scenes.make_scene((16, 24, 30), seed=5, vel_cells=0.4, B=1)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    with pytest.raises(TfluidsError, match="not divisible"):
        model.forward([tp, tU, tf])


def test_create_refusals():
    import torch
    from fluidnet_amd import FluidNetModel, TfluidsError
    dev = torch.device("cuda:0")
    sc = scenes.make_scene((16, 24, 32), seed=5, vel_cells=0.4, B=1)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    m = FluidNetModel.from_mconf(_mconf(2, "mres", "concat", "off", addPressureSkip=True), True, seed=1)
    with pytest.raises(TfluidsError, match="addPressureSkip with pooling / upsampling layers"):
        m.forward([tp, tU, tf])
    good = FluidNetModel.from_mconf(_mconf(2, "dilate", "add", "off"), True, seed=1)
    bad = [(w[:, :4] if i == 2 else w, b) for i, (w, b) in enumerate(good.layers)]   # bank 2 takes other inputs than bank 1
    with pytest.raises(TfluidsError, match="same shape"):
        FluidNetModel(bad, True, graph=good.graph).forward([tp, tU, tf])


def test_pyramid_below_an_upsampling_bank_stage(oracle):
    """mres banks whose first stage upsamples: the grid must still be divisible by the pyramid's coarsest level (grid / 4
    here, though no activation is coarser than grid / 2 after the banks' upsampling)."""
    import torch
    from fluidnet_amd import FluidNetModel, TfluidsError
    rng = np.random.RandomState(3)
    conv = lambda co, ci, k: ((rng.randn(co, ci, k, k, k) * 0.2).astype(np.float32), (rng.randn(co) * 0.01).astype(np.float32))  # noqa: E731
    layers = [conv(8, 3, 3), conv(8 * 8, 8, 3), conv(8 * 8, 8, 3), conv(8, 16, 3), conv(1, 8, 1)]
    model = FluidNetModel(layers, True, pool=[2, 1, 1, 1, 1], up=[1, 2, 2, 1, 1],
                          graph=dict(banksNum=2, banksType="mres", banksSplitStage=2, banksJoinStage=3))
    _check(oracle, model, (16, 24, 32))
    dev = torch.device("cuda:0")
    sc = scenes.make_scene((16, 24, 18), seed=5, vel_cells=0.4, B=1)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    with pytest.raises(TfluidsError, match="not divisible by the model's downsampling factor 4"):
        model.forward([tp, tU, tf])


def test_native_step_refuses_a_grid_before_writing():
    """tfl_simulate_step refuses a grid the model's pyramid cannot halve at its entry gate: nothing of the step is written."""
    import torch
    from fluidnet_amd import FluidNetModel, TfluidsError
    from fluidnet_amd.simulate import simulate_native
    dev = torch.device("cuda:0")
    model = FluidNetModel.from_mconf(_mconf(3, "mres", "concat", "affine"), True, seed=5)     # factor 4
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.5, gravityScale=0,
                 vorticityConfinementAmp=1.0, simMethod="convnet")
    b = _plume((16, 24, 30), dev)
    before = {k: b[k].clone() for k in ("pDiv", "UDiv", "density")}
    with pytest.raises(TfluidsError, match="not divisible"):
        simulate_native(None, mconf, b, model)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(b[k], v), k


@pytest.mark.parametrize("mc", [dict(banksNum=3, banksType="mres", banksAggregateMethod="concat", banksSplitStage=2,
                                     banksJoinStage=4, addBatchNorm=True),
                                dict(modelType="tog", banksNum=2, banksType="dilate", banksAggregateMethod="add",
                                     banksSplitStage=3, banksJoinStage=5, poolType="max", addBatchNorm=True,
                                     batchNormAffine=False)])
def test_loaded_file_equals_the_model_from_its_arrays(tmp_path, mc):
    """A file written by the fixture writer (the reference's gModule layout), read by load_model, runs bit for bit as the
    model built from the same arrays."""
    import torch
    import t7_fixture
    from fluidnet_amd import FluidNetModel, load_model
    dev = torch.device("cuda:0")
    want = FluidNetModel.from_mconf(mc, True, seed=8)
    p = str(tmp_path / "m")
    t7_fixture.write_model(p, want, dict(mc, is3D=True))
    _, got = load_model(p)
    sc = scenes.make_scene((32, 32, 32), seed=5, vel_cells=0.4, B=2)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    a, b = want.forward([tp, tU, tf]), got.forward([tp, tU, tf])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
