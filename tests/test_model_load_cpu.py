"""CPU checks of fluidnet_amd.load_model / FluidNetModel.from_torch7 on gModule files: the fixture writer
(tests/t7_fixture.py) pinned to the reference's shipped model, the loader on written files for every defineModelGraph
knob, and each refusal with its reason."""
import os

import numpy as np
import pytest

import t7_fixture
from fluidnet_amd import FluidNetModel, TfluidsError, load_model, torch7

MODEL2D = "/root/reference/data/models/myModel2D"
needs_ref = pytest.mark.skipif(not os.path.exists(MODEL2D), reason="the reference's data/models is not present")


def _names(gm):
    return sorted((nid, name) for nid, (_, name, _) in torch7._nodes(gm).items())


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b or (a != a and b != b)


@needs_ref
def test_writer_round_trips_the_shipped_model(tmp_path):
    gm, mc = torch7.load(MODEL2D), torch7.load(MODEL2D + "_mconf.bin")
    p = str(tmp_path / "m")
    t7_fixture.write(p, gm)
    t7_fixture.write(p + "_mconf.bin", mc)
    gm2, mc2 = torch7.load(p), torch7.load(p + "_mconf.bin")
    a, b = torch7.conv_layers(gm), torch7.conv_layers(gm2)
    assert len(a) == len(b) == 5
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert _names(gm) == _names(gm2)
    assert _same(mc, mc2)


@needs_ref
def test_from_torch7_on_the_shipped_model_is_unchanged():
    m = FluidNetModel.from_torch7(MODEL2D)
    flat = torch7.conv_layers(torch7.load(MODEL2D))
    assert m.graph is None and not m.is3D and m.pool == [1] * 5 and m.up == [1] * 5
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(m.layers, flat))
    assert m.opts == FluidNetModel(flat, False).opts


MCONFS = [
    dict(banksNum=2, banksType="mres", banksAggregateMethod="concat", banksSplitStage=2, banksJoinStage=4),
    dict(banksNum=3, banksType="dilate", banksAggregateMethod="add", banksSplitStage=1, banksJoinStage=3,
         addBatchNorm=True, batchNormAffine=False),
    dict(banksNum=3, banksType="mres", banksAggregateMethod="add", banksSplitStage=2, banksJoinStage=4, addBatchNorm=True),
    dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5, poolType="max", addBatchNorm=True),
    dict(modelType="tog"),
    dict(modelType="yang", addBatchNorm=True, nonlinType="relu6", normalizeInputChan="pDiv"),
]


@pytest.mark.parametrize("is3d", [False, True])
@pytest.mark.parametrize("mc", MCONFS)
def test_loader_yields_the_written_structure(tmp_path, is3d, mc):
    want = FluidNetModel.from_mconf(mc, is3d, seed=3)
    p = str(tmp_path / "m")
    t7_fixture.write_model(p, want, dict(mc, is3D=is3d))
    mconf, got = load_model(p)
    assert mconf["is3D"] == is3d and got.is3D == is3d
    assert got.pool == want.pool and got.up == want.up and got.opts == want.opts
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(got.layers, want.layers))
    if want.graph is None or (want.graph["banksNum"] == 1 and not want.graph["addBatchNorm"] and want.graph["poolType"] == "avg"):
        assert got.graph is None
    else:
        for k in ("banksNum", "banksType", "banksAggregateMethod", "banksSplitStage", "banksJoinStage", "poolType", "addBatchNorm"):
            assert got.graph[k] == want.graph[k], k
        for a, b in zip(got.graph["bn"] or [], want.graph["bn"] or []):
            assert all(_same(a[k], b[k]) for k in ("running_mean", "running_var", "weight", "bias")) and a["eps"] == b["eps"]
    assert _same(FluidNetModel.from_torch7(p).layers[0][0], got.layers[0][0])


@pytest.mark.parametrize("plant,msg", [(dict(bn_train=True), "training mode"), (dict(gated=True), "gated"),
                                       (dict(low_rank=True), "low-rank")])
def test_loader_refusals(tmp_path, plant, msg):
    mc = dict(banksNum=2, banksType="dilate", banksSplitStage=2, banksJoinStage=4, addBatchNorm=True)
    m = FluidNetModel.from_mconf(mc, True, seed=1)
    p = str(tmp_path / "m")
    t7_fixture.write_model(p, m, dict(mc, is3D=True), **plant)
    with pytest.raises(TfluidsError, match=msg):
        load_model(p)


def test_loader_refuses_weight_sharing_and_a_mismatched_mconf(tmp_path):
    mc = dict(banksNum=2, banksType="dilate", banksSplitStage=2, banksJoinStage=4)
    m = FluidNetModel.from_mconf(mc, True, seed=1)
    p = str(tmp_path / "m")
    t7_fixture.write_model(p, m, dict(mc, is3D=True, banksWeightShare=True))
    with pytest.raises(TfluidsError, match="weight sharing"):
        load_model(p)
    t7_fixture.write_model(p, m, dict(mc, is3D=True, banksType="mres"))      # the graph's dilation says otherwise
    with pytest.raises(TfluidsError, match="dilation"):
        load_model(p)


def test_from_torch7_without_mconf_refuses_what_it_would_drop(tmp_path):
    m = FluidNetModel.from_mconf(dict(addBatchNorm=True), True, seed=1)
    p = str(tmp_path / "m")
    t7_fixture.write_model(p, m, dict(addBatchNorm=True, is3D=True))
    os.remove(p + "_mconf.bin")
    with pytest.raises(TfluidsError, match="_mconf.bin is needed"):
        FluidNetModel.from_torch7(p)
