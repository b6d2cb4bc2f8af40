"""The z-slab rank-step (tfl_simulate_step_slab, fluidnet_amd.dist.SlabSimulation) with every advection method of
tfl_simulate_step -- euler, maccormack (the Manta form, lib/default_conf.lua's default), eulerOurs, rk2Ours, rk3Ours and
maccormackOurs -- and with several density channels. The scene has obstacles (one box runs through every cut plane, so the
line traces hit walls next to the cuts) and a jet along z whose back-traces reach close to the layout's R. Under Jacobi the
owned planes must equal the un-cut native step bit for bit at every world size; under the ConvNet exactly at world 1 and
within 1e-7 otherwise (the fp64 summation order of the std all-reduce, as in the existing z-slab tests)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from flavours import EXP_LIB, is_experiments_process
from test_hip_slab_jacobi import stub_so  # noqa: F401  (fixture: tests/stub_rccl.cpp built once per module)

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ["euler", "maccormack", "eulerOurs", "rk2Ours", "rk3Ours", "maccormackOurs"]


def scene(Zt, Y=20, X=24, B=1, channels=1, jet=0.65, dt=0.1):
    """tests/test_hip_slab_jacobi.py's plume with obstacles, a smooth non-zero density everywhere and a jet of `jet` cells per
    step along +z through the cuts; channels > 1: the RGB density of the reference's drivers (one BC value per channel)."""
    import test_hip_slab_jacobi as J
    from oracle import simulate_np as S
    b = J.scene(Zt, Y, X, B)
    rng = np.random.RandomState(5)
    base = (np.abs(scenes.smooth_field(b["density"].shape, rng)) + 0.1).astype(np.float32)
    if channels > 1:
        assert B == 1
        b["density"] = [np.ascontiguousarray(base * f) for f in (1.0, 0.5, 0.25)[:channels]]
        S.create_plume_bcs(b, [1.0, 0.5, 0.25][:channels], 0.6, 0.15)
    else:
        b["density"] = np.ascontiguousarray(b["density"] + base)
    b["UDiv"][:, 2, 3:Zt - 3, 4:Y - 4, 4:X // 2] = jet / dt
    return b


def mconf(method, sim="jacobi"):
    import test_hip_slab_jacobi as J
    c = dict(J.mconf(12), advectionMethod=method)
    if sim == "convnet":
        c = dict(c, simMethod="convnet")
        del c["maxIter"]
    return c


def sims_for(ref, conf, cuts, reach=1, overlap=None, check_reach=True, layers=None):
    """virtual ranks (threads, ThreadComm) on the uneven `cuts`; density may be a list of channels"""
    import torch
    import test_hip_slab_jacobi as J
    from fluidnet_amd import FluidNetModel
    from fluidnet_amd.dist import SlabSimulation, ThreadComm
    world = len(cuts) - 1
    hub = ThreadComm.Hub(world)
    sims = []
    for r in range(world):
        lay = J.layout(cuts, r, reach)

        def cut(v):
            if torch.is_tensor(v):
                return lay.extract(v)
            return [lay.extract(x) for x in v] if isinstance(v, list) else v
        loc = {k: cut(v) for k, v in ref.items()}
        model = FluidNetModel(layers, True) if layers is not None else None
        comm = ThreadComm(hub, r) if world > 1 else None
        sims.append(SlabSimulation(loc, conf, model, lay, comm, check_reach=check_reach, overlap=overlap, own_context=True))
    return sims


def _chans(v):
    return v if isinstance(v, list) else [v]


def assert_owned(sims, ref, tol=0.0):
    import torch
    for s in sims:
        lay = s.lay
        pairs = [("pDiv", s.batch["pDiv"], ref["pDiv"]), ("UDiv", s.batch["UDiv"], ref["UDiv"])]
        pairs += [("density%d" % i, a, b) for i, (a, b) in enumerate(zip(_chans(s.batch["density"]), _chans(ref["density"])))]
        for k, a, b in pairs:
            got, want = lay.owned(a), b[:, :, lay.z0:lay.z1]
            if tol == 0.0:
                assert torch.equal(got, want), (lay.rank, k, int((got != want).sum()))
            else:
                rel = float((got - want).norm() / want.norm().clamp_min(1e-30))
                assert rel <= tol, (lay.rank, k, rel)


def run_and_compare(ref, conf, sims, model=None, tol=0.0, rounds=3, steps=2):
    """rounds x steps steps (6 by default), compared after every round"""
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate_native
    for _ in range(rounds):
        for _ in range(steps):
            simulate_native(None, conf, ref, model)
        run_virtual_ranks(sims, steps)
        assert_owned(sims, ref, tol)
    for s in sims:
        s.close()


def _dev(b):
    import torch
    import test_hip_simulate as T
    return T._to_dev(b, torch.device("cuda:0"))


def _reach_used(ref, dt=0.1):
    return float(ref["UDiv"][:, 2].abs().max()) * dt


@pytest.mark.gpu
@pytest.mark.parametrize("world,overlap", [(1, False), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True)],
                         ids=["1", "2", "2-overlap", "3", "3-overlap", "4", "4-overlap"])
@pytest.mark.parametrize("method", METHODS)
def test_methods_jacobi_slabs_equal_uncut(method, world, overlap):
    """Every method (maccormackOurs: the control), uneven slabs, Jacobi: owned planes torch.equal after 2, 4 and 6 steps."""
    import test_hip_slab_jacobi as J
    ref = _dev(scene(9 * world + 4))
    assert _reach_used(ref) > 0.6
    conf = mconf(method)
    sims = sims_for(ref, conf, J.uneven_cuts(ref["flags"].size(2), world), overlap=overlap)
    run_and_compare(ref, conf, sims)
    assert float(ref["pDiv"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("method", METHODS)
def test_methods_convnet_slabs_equal_uncut(method, world):
    """Every method under the ConvNet projection on uneven slabs: exact at world 1, <= 1e-7 otherwise."""
    import test_hip_slab_jacobi as J
    from fluidnet_amd import FluidNetModel
    from oracle import simulate_np as S
    ref = _dev(scene(9 * world + 4, 24, 32))
    layers = S.default_3d_layers(seed=2)
    conf = mconf(method, "convnet")
    sims = sims_for(ref, conf, J.uneven_cuts(ref["flags"].size(2), world), layers=layers)
    run_and_compare(ref, conf, sims, model=FluidNetModel(layers, True), tol=0.0 if world == 1 else 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("sim", ["jacobi", "convnet"])
@pytest.mark.parametrize("method", ["maccormack", "rk3Ours", "maccormackOurs"])
def test_three_density_channels(method, sim):
    """RGB density (three channels with their own BC pairs): every channel rides in message T2; buoyancy reads channel 0."""
    import torch
    import test_hip_slab_jacobi as J
    from fluidnet_amd import FluidNetModel
    from oracle import simulate_np as S
    ref = _dev(scene(31, 24, 32, channels=3))
    assert isinstance(ref["density"], list) and len(ref["density"]) == 3
    layers = S.default_3d_layers(seed=2) if sim == "convnet" else None
    conf = mconf(method, sim)
    sims = sims_for(ref, conf, J.uneven_cuts(31, 3), overlap=True, layers=layers)
    run_and_compare(ref, conf, sims, model=FluidNetModel(layers, True) if layers else None, tol=0.0 if sim == "jacobi" else 1e-7)
    assert not torch.equal(ref["density"][0], ref["density"][2])


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["maccormack", "eulerOurs"])
def test_batch_of_two(method):
    import test_hip_slab_jacobi as J
    ref = _dev(scene(34, B=2))
    assert ref["UDiv"].size(0) == 2
    conf = mconf(method)
    run_and_compare(ref, conf, sims_for(ref, conf, J.uneven_cuts(34, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["maccormack", "rk3Ours", "euler"])
def test_reach_two_layout(method):
    """R = 2 (5 halo planes): a jet of 1.6 cells per step, deeper than any reach-1 cone, stays exact."""
    ref = _dev(scene(36, jet=1.6))
    assert 1.5 < _reach_used(ref) < 2.0
    conf = mconf(method)
    sims = sims_for(ref, conf, [0, 12, 24, 36], reach=2, overlap=True)
    assert all(s.lay.halo == 5 for s in sims)
    run_and_compare(ref, conf, sims)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["maccormack", "rk2Ours"])
def test_exact_reach_relayout(method):
    """check_reach = "exact": a jet of 1.5 cells per step forces the re-layout to R = 2 under the running simulation."""
    import test_hip_slab_jacobi as J
    ref = _dev(scene(24, 16, 16, jet=1.5))
    conf = mconf(method)
    sims = J.slab_sims(ref, conf, [0, 12, 24], check_reach="exact")
    run_and_compare(ref, conf, sims)
    for s in sims:
        assert s.relayouts == [2] and s.lay.halo == 5, (s.lay.rank, s.relayouts)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["maccormack", "eulerOurs"])
def test_reach_violation_is_reported(method):
    import test_hip_slab_jacobi as J
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import run_virtual_ranks
    sims = J.slab_sims(_dev(scene(24, 16, 16, jet=1.5)), mconf(method), [0, 12, 24])
    with pytest.raises(tfluids.TfluidsError, match="reach"):
        run_virtual_ranks(sims, 4)
    for s in sims:
        s.close()


@pytest.mark.gpu
def test_unknown_method_is_refused_before_writing():
    import ctypes
    import torch
    from fluidnet_amd.dist import SlabLayout, SlabSimulation
    ref = _dev(scene(16))
    sim = SlabSimulation(dict(ref), mconf("maccormack"), None, SlabLayout(16, 1, 0), None, graph=False)
    lib, ctx = sim._context()
    prm = type(sim.prm).from_buffer_copy(sim.prm)
    prm.advectionMethod = b"semiLagrange"
    before = ref["UDiv"].clone()
    rc = lib.tfl_simulate_step_slab(ctx, ctypes.byref(prm), ctypes.byref(sim.st), ctypes.byref(sim.slab), None,
                                    ctypes.c_void_p(sim.ws.data_ptr()), sim.ws.numel())
    torch.cuda.synchronize()
    assert rc == -1, rc                          # TFL_EINVAL
    assert "semiLagrange" in lib.tfl_last_error(ctx).decode()
    assert torch.equal(before, ref["UDiv"])
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_methods_native_transport(stub_so, world):  # noqa: F811
    env = dict(os.environ, TFL_RCCL_LIBRARY=stub_so)
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_methods_run.py"), "native", str(world), "maccormack"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "methods native transport ok" in r.stdout


@pytest.mark.gpu
def test_methods_rank_step_graph_equals_eager_step(stub_so):  # noqa: F811
    env = dict(os.environ, TFL_RCCL_LIBRARY=stub_so, STUB_RCCL_NULL="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_methods_run.py"), "graph", "0", "maccormack"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "methods slab graph ok" in r.stdout


@pytest.mark.gpu
def test_methods_in_the_experiments_flavour():
    """The same virtual-rank checks against libtfluids_hip_exp.so (child process: the library is chosen at load time)."""
    if is_experiments_process():
        pytest.skip("already the experiments flavour")
    if not os.path.exists(EXP_LIB):
        pytest.fail("fluidnet_amd/libtfluids_hip_exp.so is not built")
    env = dict(os.environ, TFL_LIBRARY=EXP_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "(jacobi_slabs and 3-overlap) or three_density or batch_of_two"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
