"""The z-slab rank-step with the Jacobi pressure projection (simMethod = 'jacobi', no model; tfl_simulate_step_slab,
fluidnet_amd.dist.SlabSimulation). A cut Jacobi solve has no all-reduce in it: the owned planes must equal the un-cut native
step bit for bit at every world size, slab thickness, iteration count and halo depth."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from flavours import EXP_LIB, is_experiments_process

HERE = os.path.dirname(os.path.abspath(__file__))


def scene(Zt, Y=20, X=24, B=1):
    """3-D plume with obstacles; one box runs through every cut plane along z. B = 2: a second, faster plume beside it."""
    import test_hip_simulate as T
    items = []
    for b in range(B):
        d = T._plume_batch((Zt, Y, X), 0.15, 0.6 + 0.5 * b, obstacles_seed=11 + b)
        d["flags"][:, :, 2:Zt - 2, Y // 2:Y // 2 + 3, X // 3:X // 3 + 4] = scenes.OBSTACLE
        items.append(d)
    if B == 1:
        return items[0]
    return {k: (np.ascontiguousarray(np.concatenate([d[k] for d in items])) if isinstance(items[0][k], np.ndarray) else items[0][k])
            for k in items[0]}


def mconf(max_iter):
    return dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.0, gravityScale=0.2,
                vorticityConfinementAmp=2.0, simMethod="jacobi", maxIter=max_iter)


def uneven_cuts(Zt, world):
    """owned ranges of unequal thickness (>= 6 planes each): rank r owns [cuts[r], cuts[r + 1])"""
    if world == 1:
        return [0, Zt]
    w = [6 + (3 * r) % 5 for r in range(world)]
    w[-1] += Zt - sum(w)
    assert min(w) >= 6, w
    return [0] + [int(x) for x in np.cumsum(w)]


def layout(cuts, rank, reach=1):
    from fluidnet_amd.dist import SlabLayout, slab_halo
    world = len(cuts) - 1
    lay = SlabLayout(cuts[-1], 1, 0, reach)          # then re-cut: SlabLayout itself only makes equal slabs
    lay.world, lay.rank = world, rank
    lay.halo = slab_halo(reach) if world > 1 else 0
    lay.z0, lay.z1 = int(cuts[rank]), int(cuts[rank + 1])
    lay.lo, lay.hi = max(lay.z0 - lay.halo, 0), min(lay.z1 + lay.halo, lay.z_total)
    lay.c0, lay.c1 = lay.z0 - lay.lo, lay.z1 - lay.lo
    lay.has_lower, lay.has_upper = rank > 0, rank < world - 1
    return lay


def slab_sims(ref, conf, cuts, reach=1, overlap=None, check_reach=True, transport="thread"):
    import torch
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import RcclComm, SlabSimulation, ThreadComm
    world = len(cuts) - 1
    hub = ThreadComm.Hub(world)
    uid = RcclComm.unique_id(tfluids._context(ref["flags"])[1]) if transport == "native" and world > 1 else None
    sims = []
    for r in range(world):
        lay = layout(cuts, r, reach)
        loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
        comm = None
        if world > 1:
            comm = ThreadComm(hub, r) if transport == "thread" else (lambda ctx, r=r: RcclComm(ctx, uid, r, world))
        sims.append(SlabSimulation(loc, conf, None, lay, comm, check_reach=check_reach, overlap=overlap, own_context=True))
    return sims


def assert_owned_equal(sims, ref):
    import torch
    for s in sims:
        for k in ("pDiv", "UDiv", "density"):
            got, want = s.lay.owned(s.batch[k]), ref[k][:, :, s.lay.z0:s.lay.z1]
            assert torch.equal(got, want), (s.lay.rank, k, int((got != want).sum()))


def assert_halos_equal(sims, ref):
    """after drain() the halo planes the end-of-step message refreshes are valid too: U (2, 2), p (4 below, 3 above)"""
    import torch
    for s in sims:
        lay = s.lay
        for k, below, above in (("UDiv", 2, 2), ("pDiv", 4, 3)):
            a = lay.c0 - (below if lay.has_lower else 0)
            b = lay.c1 + (above if lay.has_upper else 0)
            assert torch.equal(s.batch[k][:, :, a:b], ref[k][:, :, lay.lo + a:lay.lo + b]), (lay.rank, k)


def run_and_compare(ref, conf, sims, rounds=3, steps=1):
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate_native
    for _ in range(rounds):
        for _ in range(steps):
            simulate_native(None, conf, ref, None)
        run_virtual_ranks(sims, steps)
        assert_owned_equal(sims, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True], ids=["no-overlap", "overlap"])
@pytest.mark.parametrize("max_iter", [1, 3, 4, 34])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_jacobi_slab_virtual_ranks_equal_uncut(world, max_iter, overlap):
    """Virtual ranks (threads, ThreadComm) on uneven slabs; maxIter 1 (a lone last round), 3 (< the halo: no p exchange),
    4 (= the halo: a round that ends on the owned planes, then the final exchange) and 34 (the 3-D driver's count: 8 exchanges).
    Owned planes of pDiv, UDiv and density are torch.equal to simulate_native after every round of steps."""
    import torch
    import test_hip_simulate as T
    ref = T._to_dev(scene(9 * world + 4), torch.device("cuda:0"))
    conf = mconf(max_iter)
    sims = slab_sims(ref, conf, uneven_cuts(ref["flags"].size(2), world), overlap=overlap)
    run_and_compare(ref, conf, sims, rounds=3, steps=2)
    assert float(ref["UDiv"].abs().max()) > 0.1 and float(ref["pDiv"].abs().max()) > 0
    assert_halos_equal(sims, ref)
    for s in sims:
        s.close()


@pytest.mark.gpu
def test_jacobi_slab_batch_of_two():
    import torch
    import test_hip_simulate as T
    ref = T._to_dev(scene(34, B=2), torch.device("cuda:0"))
    assert ref["UDiv"].size(0) == 2
    conf = mconf(34)
    sims = slab_sims(ref, conf, uneven_cuts(34, 3))
    run_and_compare(ref, conf, sims, rounds=3)
    assert not torch.equal(ref["pDiv"][0], ref["pDiv"][1])
    for s in sims:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [5, 34])
def test_jacobi_slab_exchange_interval_follows_the_halo(max_iter):
    """A reach-2 layout stores 5 halo planes: the p exchanges come every 5 sweeps instead of every 4."""
    import torch
    import test_hip_simulate as T
    ref = T._to_dev(scene(36), torch.device("cuda:0"))
    conf = mconf(max_iter)
    sims = slab_sims(ref, conf, [0, 12, 24, 36], reach=2)
    assert all(s.lay.halo == 5 for s in sims)
    run_and_compare(ref, conf, sims, rounds=3)
    for s in sims:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_jacobi_slab_exact_reach_relayout(world):
    """check_reach = "exact": a flow of 1.5 cells per step along z through the cuts forces a re-layout to reach 2 (halo 5, so
    the exchange interval changes under the running simulation); the cut run still equals the un-cut one."""
    import torch
    import test_hip_simulate as T
    Zt = 12 * world
    b = scene(Zt, 16, 16)
    b["UDiv"][:, 2, 4:Zt - 4, 4:12, 4:12] = 15.0
    ref = T._to_dev(b, torch.device("cuda:0"))
    conf = mconf(34)
    sims = slab_sims(ref, conf, [12 * r for r in range(world + 1)], check_reach="exact")
    run_and_compare(ref, conf, sims, rounds=3)
    for s in sims:
        assert s.relayouts == [2] and s.lay.halo == 5, (s.lay.rank, s.relayouts)
        s.close()


@pytest.mark.gpu
def test_jacobi_slab_reach_violation_is_reported():
    """check_reach = 1 has no projection kernel to ride on here: k_absmax and a publication launch of its own must still report
    a flow faster than the layout's reach."""
    import torch
    import test_hip_simulate as T
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import run_virtual_ranks
    b = scene(24, 16, 16)
    b["UDiv"][:, 2, 4:20, 4:12, 4:12] = 15.0
    sims = slab_sims(T._to_dev(b, torch.device("cuda:0")), mconf(34), [0, 12, 24])
    with pytest.raises(tfluids.TfluidsError, match="reach"):
        run_virtual_ranks(sims, 4)
    for s in sims:
        s.close()


@pytest.fixture(scope="module")
def stub_so(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stub") / "libstub_rccl.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "-O2", "-o", out, os.path.join(HERE, "stub_rccl.cpp")])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_jacobi_slab_native_transport(stub_so, world):
    env = dict(os.environ, TFL_RCCL_LIBRARY=stub_so)
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_jacobi_run.py"), "native", str(world)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "jacobi native transport ok" in r.stdout


@pytest.mark.gpu
def test_jacobi_rank_step_graph_equals_eager_step(stub_so):
    env = dict(os.environ, TFL_RCCL_LIBRARY=stub_so, STUB_RCCL_NULL="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_jacobi_run.py"), "graph"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "jacobi slab graph ok" in r.stdout


@pytest.mark.gpu
def test_pcg_slab_is_refused():
    """PCG stays out: SlabSimulation says so, and so does the native step (TFL_EUNSUPPORTED and a message)."""
    import ctypes
    import torch
    import test_hip_simulate as T
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import SlabLayout, SlabSimulation
    ref = T._to_dev(scene(16), torch.device("cuda:0"))
    with pytest.raises(tfluids.TfluidsError, match="PCG"):
        SlabSimulation(dict(ref), dict(mconf(10), simMethod="pcg"), None, SlabLayout(16, 1, 0), None)
    sim = SlabSimulation(dict(ref), mconf(10), None, SlabLayout(16, 1, 0), None, graph=False)
    lib, ctx = sim._context()
    prm = type(sim.prm).from_buffer_copy(sim.prm)
    prm.simMethod = b"pcg"
    rc = lib.tfl_simulate_step_slab(ctx, ctypes.byref(prm), ctypes.byref(sim.st), ctypes.byref(sim.slab), None,
                                    ctypes.c_void_p(sim.ws.data_ptr()), sim.ws.numel())
    assert rc == -3, rc                          # TFL_EUNSUPPORTED
    assert "PCG" in lib.tfl_last_error(ctx).decode()
    sim.close()


@pytest.mark.gpu
def test_jacobi_slab_in_the_experiments_flavour():
    """The same virtual-rank checks against libtfluids_hip_exp.so (child process: the library is chosen at load time)."""
    if is_experiments_process():
        pytest.skip("already the experiments flavour")
    if not os.path.exists(EXP_LIB):
        pytest.fail("fluidnet_amd/libtfluids_hip_exp.so is not built")
    env = dict(os.environ, TFL_LIBRARY=EXP_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "virtual_ranks and 34 or batch_of_two or follows_the_halo"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
