"""CPU checks of the model-graph form of the projection net (tfl_model_create_graph, FluidNetModel(..., graph=...)):
the PyTorch-CPU restatement of lib/model.lua:253-392 in tests/model_graph_ref.py is pinned to oracle/simulate_np.conv_stack
on the graphs both cover, FluidNetModel.from_mconf to the existing seeded stand-ins, the Python-side refusals, and the new
kernels to a gfx950 compile."""
import os
import subprocess

import numpy as np
import pytest
import torch

import model_graph_ref as R
from fluidnet_amd import FluidNetModel, TfluidsError
from oracle import simulate_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x(model, dims, seed=0):
    ci = model.layers[0][0].shape[1]
    return np.random.RandomState(seed).randn(2, ci, *dims).astype(np.float32)


@pytest.mark.parametrize("mt,is3d,dims", [("default", False, (1, 16, 20)), ("default", True, (8, 12, 16)),
                                          ("tog", True, (8, 12, 16)), ("tog", False, (1, 16, 20)),
                                          ("yang", True, (8, 12, 16))])
def test_one_bank_restatement_equals_conv_stack(mt, is3d, dims):
    model = FluidNetModel.from_mconf(dict(modelType=mt, nonlinType="relu6"), is3d, seed=4)
    x = _x(model, dims)
    want = S.conv_stack(x, model.layers, is3d, pool=model.pool, up=model.up, nonlin="relu6")
    assert np.array_equal(R.graph_stack(x, model), want)


def test_from_mconf_generalises_the_seeded_stand_ins():
    for a, b in ((FluidNetModel.from_mconf({}, True, seed=3), FluidNetModel.default_3d(seed=3)),
                 (FluidNetModel.from_mconf(dict(modelType="tog"), True, seed=2), FluidNetModel.tog(True, seed=2)),
                 (FluidNetModel.from_mconf(dict(modelType="tog"), False, seed=2), FluidNetModel.tog(False, seed=2))):
        assert a.pool == b.pool and a.up == b.up
        assert all(np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) for u, v in zip(a.layers, b.layers))
    # the banks' convs come in creation order (stage, bank); BN statistics are drawn after every conv
    m = FluidNetModel.from_mconf(dict(banksNum=3, banksSplitStage=2, banksJoinStage=4, addBatchNorm=True), True, seed=3)
    assert [w.shape[:2] for w, _ in m.layers] == [(8, 3)] + [(8, 8)] * 6 + [(8, 24), (1, 8)]
    assert len(m.graph["bn"]) == len(m.layers) - 1
    assert np.array_equal(m.layers[0][0], FluidNetModel.default_3d(seed=3).layers[0][0])


def test_restatement_banks_by_hand():
    """Two dilated banks added, one stage each, against torch.nn.functional written out for this one graph."""
    import torch.nn.functional as F
    m = FluidNetModel.from_mconf(dict(banksNum=2, banksType="dilate", banksAggregateMethod="add", banksSplitStage=2,
                                      banksJoinStage=3, addBatchNorm=True, batchNormAffine=False), False, seed=5)
    x = _x(m, (1, 16, 20))
    t = lambda a: torch.from_numpy(np.asarray(a))      # noqa: E731
    bn = lambda h, d: (h - t(d["running_mean"]).view(1, -1, 1, 1)) / torch.sqrt(t(d["running_var"]).view(1, -1, 1, 1) + d["eps"])  # noqa: E731
    h = t(x)[:, :, 0]
    h = bn(torch.relu(F.conv2d(h, t(m.layers[0][0]), t(m.layers[0][1]), padding=1)), m.graph["bn"][0])
    b1 = bn(torch.relu(F.conv2d(h, t(m.layers[1][0]), t(m.layers[1][1]), padding=1)), m.graph["bn"][1])
    b2 = bn(torch.relu(F.conv2d(h, t(m.layers[2][0]), t(m.layers[2][1]), padding=2, dilation=2)), m.graph["bn"][2])
    h = b1 + b2
    for i in (3, 4, 5):
        h = F.conv2d(h, t(m.layers[i][0]), t(m.layers[i][1]), padding=(m.layers[i][0].shape[-1] - 1) // 2)
        if i < 5:
            h = bn(torch.relu(h), m.graph["bn"][i])
    assert np.array_equal(R.graph_stack(x, m), h.unsqueeze(2).numpy())


def test_restatement_mres_concat_shapes_and_max_pool():
    m = FluidNetModel.from_mconf(dict(modelType="tog", banksNum=3, banksSplitStage=2, banksJoinStage=5, poolType="max"),
                                 True, seed=1)
    x = _x(m, (16, 16, 32))
    out = R.graph_stack(x, m)
    assert out.shape == (2, 1, 16, 16, 32) and np.isfinite(out).all()
    m2 = FluidNetModel.from_mconf(dict(modelType="tog", banksNum=3, banksSplitStage=2, banksJoinStage=5), True, seed=1)
    assert not np.array_equal(R.graph_stack(x, m2), out)       # max pooling is not average pooling


@pytest.mark.parametrize("graph,msg", [(dict(banksWeightShare=True), "weight sharing"),
                                       (dict(banksType="concat"), "banksType"),
                                       (dict(banksAggregateMethod="mul"), "banksAggregateMethod"),
                                       (dict(poolType="l2"), "poolType")])
def test_python_refusals(graph, msg):
    with pytest.raises(TfluidsError, match=msg):
        FluidNetModel.from_mconf(graph, True)
    m = FluidNetModel.from_mconf({}, True)
    with pytest.raises(TfluidsError, match="unknown model graph field"):
        FluidNetModel(m.layers, True, graph=dict(gatedConv=True))


def test_binding_declares_the_graph_entry_point():
    from fluidnet_amd import _lib
    assert "tfl_model_create_graph" in _lib.SIGNATURES
    names = [f[0] for f in _lib.tfl_model_graph._fields_]
    assert names[:7] == ["banks_num", "bank_type", "aggregate", "split_stage", "join_stage", "pool_type", "batch_norm"]
    lua = open(os.path.join(ROOT, "fluidnet_amd", "lua", "tfluids_hip.lua")).read()
    assert "tfl_model_create_graph" in lua and "tfl_model_graph" in lua


def test_graph_kernels_cross_compile_for_gfx950(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "fluidnet_amd", "csrc", "conv.hip")
    obj = str(tmp_path / "conv.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", "-o", obj, src])
    syms = subprocess.check_output(["nm", "-C", obj]).decode()
    for k in ("k_conv_direct_ex<true, 8, 8>", "k_conv_direct_ex<false, 16, 16>", "k_pool2_ex<true, true>",
              "k_pool2_ex<false, false>", "k_bank_join<true, false>", "k_bank_join<false, true>"):
        assert k in syms, k
