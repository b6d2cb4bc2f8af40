"""The z-slab rank-step (tfl_simulate_step_slab, fluidnet_amd.dist.SlabSimulation) with every projection net that is not a
graph model: the `tog` and `yang` layer tables, the tfl_model_opts switches and the default topology on the
shape-generic kernels. Virtual ranks (ThreadComm) on uneven cuts that are multiples of the model's downsampling factor, the
plume with obstacles through the cuts and a z-jet (tests/test_hip_slab_methods.py scene), 6 steps; the owned planes are
compared with the un-cut native step: exact at world 1, within 1e-7 otherwise (the fp64 order of the input-scale all-reduce),
and bit for bit at every world when the input is not normalised."""
import os
import subprocess
import sys

import pytest

from test_hip_slab_jacobi import stub_so  # noqa: F401  (fixture: tests/stub_rccl.cpp built once per module)

HERE = os.path.dirname(os.path.abspath(__file__))
STATE = ("pDiv", "UDiv", "density")


def net(name, **opts):
    """a fresh FluidNetModel (each rank creates its own handle, as a process per GPU would)"""
    from fluidnet_amd import FluidNetModel
    from oracle import simulate_np as S
    if name == "tog" and not opts:
        return FluidNetModel.tog(True, seed=3)
    if name == "default":
        return FluidNetModel(S.default_3d_layers(seed=2), True, opts=opts or None)
    return FluidNetModel.from_mconf(dict(modelType=name, **opts), True, seed=3)


def cuts_for(Zt, world, F):
    """uneven owned ranges on multiples of F, each at least as thick as the model halo (16 for tog)"""
    if world == 1:
        return [0, Zt]
    if F == 1:
        import test_hip_slab_jacobi as J
        return J.uneven_cuts(Zt, world)
    w = [16 + 4 * (r % 2) for r in range(world)]
    w[-1] += Zt - sum(w)
    assert min(w) >= 16 and all(x % F == 0 for x in w), w
    out = [0]
    for x in w:
        out.append(out[-1] + x)
    return out


def layout(cuts, rank, model, reach=1, halo=None):
    from fluidnet_amd.dist import SlabLayout, slab_halo
    world = len(cuts) - 1
    lay = SlabLayout(cuts[-1], 1, 0, reach)          # then re-cut: SlabLayout itself only makes equal slabs
    lay.world, lay.rank, lay.model = world, rank, model
    lay.halo = (halo if halo is not None else slab_halo(reach, model)) if world > 1 else 0
    lay.z0, lay.z1 = int(cuts[rank]), int(cuts[rank + 1])
    lay.lo, lay.hi = max(lay.z0 - lay.halo, 0), min(lay.z1 + lay.halo, lay.z_total)
    lay.c0, lay.c1 = lay.z0 - lay.lo, lay.z1 - lay.lo
    lay.has_lower, lay.has_upper = rank > 0, rank < world - 1
    return lay


def sims(ref, conf, cuts, make, halo=None, check_reach=True, overlap=None, poison=False):
    import torch
    from fluidnet_amd.dist import SlabSimulation, ThreadComm
    world = len(cuts) - 1
    hub = ThreadComm.Hub(world)
    out = []
    for r in range(world):
        model = make()
        lay = layout(cuts, r, model, halo=halo)
        loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
        if poison:      # NaN into every stored-halo plane beyond the model halo
            from fluidnet_amd.dist import slab_halo
            h = slab_halo(1, model)
            for k in STATE:
                if lay.has_lower:
                    loc[k][:, :, :lay.c0 - h] = float("nan")
                if lay.has_upper:
                    loc[k][:, :, lay.c1 + h:] = float("nan")
        out.append(SlabSimulation(loc, conf, model, lay, ThreadComm(hub, r) if world > 1 else None, check_reach=check_reach,
                                  overlap=overlap, own_context=True))
    return out


def conf(method="maccormack"):
    import test_hip_slab_methods as M
    return M.mconf(method, "convnet")


def scene(Zt, **kw):
    import test_hip_slab_methods as M
    return M._dev(M.scene(Zt, **kw))


def compare(ref, c, ss, make, tol):
    import test_hip_slab_methods as M
    M.run_and_compare(ref, c, ss, model=make(), tol=tol)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["tog", "yang"])
def test_tog_and_yang_slabs_equal_uncut(name, world):
    from fluidnet_amd.dist import model_cone
    F = model_cone(net(name))["F"]
    Zt = 72 if F > 1 else 9 * world + 4
    ref = scene(Zt, Y=20, X=24)
    c = conf()
    ss = sims(ref, c, cuts_for(Zt, world, F), lambda: net(name))
    if world > 1:
        assert all(s.lay.halo == (16 if name == "tog" else 4) for s in ss)
    compare(ref, c, ss, lambda: net(name), 0.0 if world == 1 else 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["tog", "yang"])
def test_unnormalised_input_is_bit_exact(name, world):
    """normalizeInput = false: no all-reduce at all, so every world equals the un-cut step bit for bit"""
    F = 4 if name == "tog" else 1
    Zt = 72 if F > 1 else 9 * world + 4
    ref = scene(Zt, Y=20, X=24)
    c = conf("maccormackOurs")
    make = (lambda: net(name, normalizeInput=False))
    compare(ref, c, sims(ref, c, cuts_for(Zt, world, F), make), make, 0.0)


OPTS = {
    "UDiv-input": dict(inputChannels=dict(pDiv=True, UDiv=True, div=True, flags=True)),
    "norm-pDiv": dict(normalizeInputChan="pDiv"),
    "norm-div": dict(normalizeInputChan="div"),
    "l2": dict(normalizeInputFunc="norm"),
    "l2-UDiv-input": dict(normalizeInputFunc="norm", inputChannels=dict(pDiv=False, UDiv=True, div=True, flags=True)),
    "pressure-skip": dict(addPressureSkip=True),
    "relu6": dict(nonlinType="relu6"),
    "sigmoid": dict(nonlinType="sigmoid"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_model_opts_slabs_equal_uncut(opt, world):
    """every tfl_model_opts switch (on the yang table): the scale over the owned planes, the UDiv channels through message T3"""
    import torch
    Zt = 9 * world + 4
    ref = scene(Zt, Y=20, X=24)
    torch.manual_seed(3)        # a pressure to start from: std(pDiv) of the plume's zero pressure would be 0 (normalizeInputChan pDiv)
    ref["pDiv"].copy_(0.01 * torch.randn_like(ref["pDiv"]))
    c = conf()
    make = (lambda: net("yang", **OPTS[opt]))
    compare(ref, c, sims(ref, c, cuts_for(Zt, world, 1), make, overlap=world > 1), make, 0.0 if world == 1 else 1e-7)


@pytest.mark.gpu
def test_tog_with_opts_and_overlap():
    make = (lambda: net("tog", inputChannels=dict(pDiv=True, UDiv=True, div=True, flags=True), normalizeInputChan="div",
                        nonlinType="relu6"))
    ref = scene(72, Y=20, X=24)
    c = conf()
    compare(ref, c, sims(ref, c, cuts_for(72, 3, 4), make, overlap=True), make, 1e-7)


@pytest.mark.gpu
def test_default_topology_on_the_direct_path():
    """the default topology under TFL_CONV_PATH=direct (child process: the path is chosen when a model is created)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_models_run.py"), "direct"],
                       env=dict(os.environ, TFL_CONV_PATH="direct"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "slab models direct ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["native", "graph"])
def test_native_transport_and_graph_replay(stub_so, mode):  # noqa: F811
    env = dict(os.environ, TFL_RCCL_LIBRARY=stub_so)
    if mode == "graph":
        env["STUB_RCCL_NULL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_models_run.py"), mode], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "slab models %s ok" % mode in r.stdout


@pytest.mark.gpu
def test_reach_relayout_keeps_the_model_halo():
    """check_reach = "exact" with a tog net: the re-layout to R = 2 keeps the 16-plane model halo and the alignment"""
    from fluidnet_amd.dist import SlabLayout, SlabSimulation, ThreadComm
    import torch
    ref = scene(48, Y=16, X=16, jet=1.5)
    c = conf()
    hub = ThreadComm.Hub(2)
    ss = []
    for r in range(2):
        model = net("tog")
        lay = SlabLayout(48, 2, r, 1, model=model)
        assert lay.halo == 16
        loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
        ss.append(SlabSimulation(loc, c, model, lay, ThreadComm(hub, r), check_reach="exact", own_context=True))
    compare(ref, c, ss, lambda: net("tog"), 1e-7)
    for s in ss:
        assert s.relayouts == [2] and s.lay.halo == 16, (s.lay.rank, s.relayouts, s.lay.halo)


@pytest.mark.gpu
def test_nan_beyond_the_model_halo_does_not_reach_the_owned_planes():
    """a stored halo of 24 planes, NaN in every state plane deeper than the 16 the tog cone needs"""
    import torch
    ref = scene(80, Y=20, X=24)
    c = conf()
    ss = sims(ref, c, [0, 24, 56, 80], lambda: net("tog"), halo=24, check_reach=False, poison=True)
    assert any(torch.isnan(s.batch["pDiv"]).any() for s in ss)
    compare(ref, c, ss, lambda: net("tog"), 1e-7)


def _refused(ref, c, cuts, halo, match):
    import torch
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.dist import ThreadComm, SlabSimulation
    hub = ThreadComm.Hub(len(cuts) - 1)
    for r in range(len(cuts) - 1):
        model = net("tog")
        lay = layout(cuts, r, model, halo=halo)
        loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
        before = {k: loc[k].clone() for k in STATE}
        with pytest.raises(TfluidsError, match=match):
            sim = SlabSimulation(loc, c, model, lay, ThreadComm(hub, r), own_context=True)
            sim.step(eager=True)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(loc[k], before[k]), (r, k)


@pytest.mark.gpu
def test_thin_halo_and_misaligned_cuts_are_refused_before_writing():
    ref = scene(48, Y=20, X=24)
    c = conf()
    _refused(ref, c, [0, 24, 48], 4, "halo too thin")                       # the default-topology halo
    _refused(ref, c, [0, 22, 48], 18, "multiples of 4")                     # owned boundary off the pooling grid
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.dist import slab_halo
    from fluidnet_amd import FluidNetModel
    with pytest.raises(TfluidsError, match="un-sharded"):
        slab_halo(1, FluidNetModel.from_mconf(dict(banksNum=2, banksType="dilate"), True))


@pytest.mark.gpu
def test_native_halo_entry_agrees_with_the_cone():
    from fluidnet_amd.dist import model_cone, slab_halo
    for name, want in (("default", 4), ("yang", 4), ("tog", 16)):
        m = net(name)
        assert slab_halo(1, m) == max(4, model_cone(m)["halo"]) == want, name
        assert slab_halo(3, m) == max(7, want), name
    assert slab_halo(9, net("tog")) == 20          # max(19, 15) rounded up to 4
    assert slab_halo(2, net("default", nonlinType="sigmoid")) == 5
