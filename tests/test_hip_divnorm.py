"""The divergence-norm rollout on the device: tfluids.velocityDivergenceNorm (tfl_velocityDivergenceNorm, divnorm.hip),
SlabSimulation.divergence_norm (tfl_slab_divergence_norm) and stats.calcStats (the rollout of lib/calc_stats.lua:98-118).

The operator is held to |norm - exact| <= (N + 2) 2^-53 exact per sample (tests/divnorm_ref.py: derived from the reduction,
no margin), with exact > 1e-3 asserted for every sample; the z-slab form and calcStats are held to torch.equal."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import divnorm_ref as R
import flavours

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

from test_hip_slab_jacobi import stub_so  # noqa: E402,F401  (fixture: tests/stub_rccl.cpp built once per module)


def _dev_pair(U, flags, how):
    """device tensors of (U, flags); "misaligned": contiguous views that start 4 bytes past a 16-byte boundary"""
    import torch
    dev = torch.device("cuda:0")
    out = []
    for a in (U, flags):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if how == "misaligned":
            buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            out.append(v)
        else:
            out.append(t.to(dev))
            assert out[-1].data_ptr() % 16 == 0
    return out


def _check(name, dims, got, exact):
    lim = R.bound(dims, exact)
    for b in range(len(exact)):
        err = abs(float(got[b]) - exact[b])
        print("divnorm %-24s b=%d exact=%.17g got=%.17g |err|=%.3e bound=%.3e" % (name, b, exact[b], float(got[b]), err, lim[b]))
    for b in range(len(exact)):
        assert exact[b] > R.MIN_EXACT, (name, b, exact[b])
        assert abs(float(got[b]) - exact[b]) <= lim[b], (name, b, float(got[b]), exact[b], lim[b])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_operator_against_the_exact_norm(oracle, name):
    import torch
    from fluidnet_amd import tfluids
    _, dims, B, how = next(c for c in R.CASES if c[0] == name)
    U, flags = R.make_case(name)
    tU, tf = _dev_pair(U, flags, how)
    before = tU.clone()
    got = tfluids.velocityDivergenceNorm(tU, tf)
    assert got.dtype == torch.float64 and got.shape == (B,) and got.is_cuda
    again = tfluids.velocityDivergenceNorm(tU, tf)
    assert torch.equal(got, again) and torch.equal(tU, before)      # fixed order: the same bits every time; nothing written
    _check(name, dims, got.cpu().numpy(), R.exact_norm(oracle, U, flags))


@pytest.mark.gpu
def test_at_128_cubed_after_three_steps(oracle):
    """BASELINE config 4's scene (bench.py build_scene) after three steps of the native step"""
    import torch
    import bench
    from fluidnet_amd import FluidNetModel, tfluids
    from fluidnet_amd.simulate import simulate_native
    batch, mconf = bench.build_scene(128, 128, None, torch.device("cuda:0"))
    model = FluidNetModel.default_3d(seed=1)
    for _ in range(3):
        simulate_native(None, mconf, batch, model)
    got = tfluids.velocityDivergenceNorm(batch["UDiv"], batch["flags"]).cpu().numpy()
    exact = R.exact_norm(oracle, batch["UDiv"].cpu().numpy(), batch["flags"].cpu().numpy())
    _check("128^3 config 4, 3 steps", (128, 128, 128), got, exact)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3d-32x32x32-b2", "3d-ragged-b2", "2d-64x96-b2"])
def test_batch_items_do_not_depend_on_the_batch(name):
    import torch
    from fluidnet_amd import tfluids
    U, flags = R.make_case(name)
    tU, tf = _dev_pair(U, flags, "aligned")
    both = tfluids.velocityDivergenceNorm(tU, tf)
    for b in range(2):
        one = tfluids.velocityDivergenceNorm(tU[b:b + 1].contiguous(), tf[b:b + 1].contiguous())
        assert torch.equal(one[0], both[b]), (name, b)


@pytest.mark.gpu
def test_two_launches_both_from_divnorm_hip():
    from fluidnet_amd import _kernels, tfluids
    U, flags = R.make_case("3d-16x24x32")
    tU, tf = _dev_pair(U, flags, "aligned")
    tfluids.velocityDivergenceNorm(tU, tf)
    with tfluids.profile(tU) as prof:
        tfluids.velocityDivergenceNorm(tU, tf)
    assert sorted(prof.kernels) == ["k_divnorm_finish", "k_divnorm_planes"], prof.kernels
    assert all(v["calls"] == 1 for v in prof.kernels.values()), prof.kernels
    assert all(_kernels.source_of(k) == "divnorm.hip" for k in prof.kernels)
    assert "k_divergence" not in prof.kernels


@pytest.mark.gpu
def test_captured_call_replays_on_new_data():
    import torch
    from fluidnet_amd import tfluids
    U, flags = R.make_case("3d-32x32x32-b2")
    tU, tf = _dev_pair(U, flags, "aligned")
    U2 = torch.from_numpy(R.make_case("3d-32x32x32-b2")[0] * np.float32(1.7) + np.float32(0.01)).to(tU.device)
    want2 = tfluids.velocityDivergenceNorm(U2, tf).clone()
    out = torch.zeros(2, dtype=torch.float64, device=tU.device)
    tfluids.velocityDivergenceNorm(tU, tf, out=out)             # warm-up: the scratch exists before the capture
    first = out.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tfluids.velocityDivergenceNorm(tU, tf, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    tU.copy_(U2)                                                # overwritten in place
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2) and not torch.equal(out, first)


# ---- z-slabs ---------------------------------------------------------------------------------------------------------
def run_ranks(sims, fn):
    """fn(sim) on every virtual rank, one thread each (ThreadComm's barriers need them side by side); the results by rank"""
    import torch
    dev = sims[0].batch["UDiv"].device
    out, errs = [None] * len(sims), []

    def work(i, sim):
        try:
            torch.cuda.set_device(dev)
            out[i] = fn(sim)
        except Exception as e:   # noqa: BLE001
            errs.append(e)
            try:
                sim.comm.hub.barrier.abort()
            except Exception:
                pass

    ts = [threading.Thread(target=work, args=(i, s)) for i, s in enumerate(sims)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize(dev)
    if errs:
        raise errs[0]
    return out


def slab_case(world, transport="thread"):
    """48 planes in `world` equal slabs with 4-plane halos, the Jacobi projection (bit-equal to the un-cut step at any world)"""
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    ref = M._dev(M.scene(48))
    conf = M.mconf("maccormackOurs")
    cuts = [48 * r // world for r in range(world + 1)]
    sims = J.slab_sims(ref, conf, cuts, transport=transport)
    assert all(s.lay.halo == (4 if world > 1 else 0) for s in sims)
    return ref, conf, sims


def slab_norms_equal_uncut(world, transport="thread"):
    import torch
    import test_hip_slab_jacobi as J
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    ref, conf, sims = slab_case(world, transport)
    for _ in range(3):
        simulate_native(None, conf, ref, None)
    want = tfluids.velocityDivergenceNorm(ref["UDiv"], ref["flags"]).clone()
    assert float(want.min()) > R.MIN_EXACT

    def three_steps_then_norm(sim):
        for _ in range(3):
            sim.step()
        return sim.divergence_norm().clone()        # the U / p message of the third step is still in flight here
    got = run_ranks(sims, three_steps_then_norm)
    for r, g in enumerate(got):
        print("slab divnorm world %d rank %d: %.17g (un-cut %.17g)" % (world, r, float(g[0]), float(want[0])))
        assert torch.equal(g, want), (world, r, g, want)
    # the next step is not disturbed: it still gives the un-cut step's bits
    simulate_native(None, conf, ref, None)

    def one_more(sim):
        sim.step()
        sim.drain()
    run_ranks(sims, one_more)
    J.assert_owned_equal(sims, ref)
    for s in sims:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_slab_norm_equals_uncut_bit_for_bit(world):
    """world 1 = a slab without neighbours (no all-reduce)"""
    slab_norms_equal_uncut(world)


@pytest.mark.gpu
def test_slab_norm_native_transport(stub_so):  # noqa: F811
    r = subprocess.run([sys.executable, os.path.join(HERE, "slab_divnorm_run.py"), "native"], env=dict(os.environ, TFL_RCCL_LIBRARY=stub_so),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "slab divnorm native ok" in r.stdout


@pytest.mark.gpu
def test_slab_norm_refuses_2d():
    import torch
    import test_hip_simulate as T
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.dist import SlabLayout, SlabSimulation
    b = T._to_dev(T._plume_batch((1, 32, 32), 0.05, 10.0), torch.device("cuda:0"))
    conf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.0, gravityScale=0,
                vorticityConfinementAmp=0, simMethod="jacobi", maxIter=4)
    sim = SlabSimulation(b, conf, None, SlabLayout(1, 1, 0), None)
    with pytest.raises(TfluidsError, match="no z to cut"):
        sim.divergence_norm()


# ---- calcStats -------------------------------------------------------------------------------------------------------
def _calc_stats_case(kind):
    import torch
    import test_hip_simulate as T
    from fluidnet_amd import FluidNetModel
    dev = torch.device("cuda:0")
    if kind == "convnet":      # 3-D default topology, seeded weights
        b = T._plume_batch((24, 24, 24), 0.15, 1.0 * 24 / 128, 7)
        conf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=2.0 * 24 / 128, gravityScale=0.3,
                    vorticityConfinementAmp=3.0, simMethod="convnet")
        model = FluidNetModel.default_3d(seed=1)
    else:                      # 2-D 64^2, Jacobi with 20 iterations
        b = T._plume_batch((1, 64, 64), 0.05, 10.0)
        conf = dict(dt=4 / 60, advectionMethod="maccormackOurs", maccormackStrength=0.75, buoyancyScale=1.0, gravityScale=0.3,
                    vorticityConfinementAmp=0, simMethod="jacobi", maxIter=20)
        model = None
    rng = np.random.RandomState(3)      # a start state with a divergence of its own (column 0)
    b["UDiv"] = (b["UDiv"] + 0.05 * rng.randn(*b["UDiv"].shape)).astype(np.float32)
    return T._to_dev(b, dev), T._to_dev(b, dev), conf, model


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["convnet", "jacobi"])
def test_calc_stats_equals_the_step_by_step_loop(kind):
    import torch
    from fluidnet_amd import stats, tfluids
    from fluidnet_amd.simulate import simulate_native
    n = 6
    ba, bb, conf, model = _calc_stats_case(kind)
    kept = dict(conf)
    got = stats.calcStats(conf, ba, model, n)["normDiv"]
    assert conf == kept and conf["gravityScale"] == 0.3          # the caller's mconf is as it was
    assert got.dtype == torch.float64 and got.shape == (1, n) and not got.is_cuda
    loop_conf = dict(conf, gravityScale=0)
    cols = [tfluids.velocityDivergenceNorm(bb["UDiv"], bb["flags"]).cpu()]
    start = cols[0].clone()
    for _ in range(1, n):
        simulate_native(None, loop_conf, bb, model)
        cols.append(tfluids.velocityDivergenceNorm(bb["UDiv"], bb["flags"]).cpu())
    want = torch.stack(cols, dim=1)
    print("calcStats %s normDiv:" % kind, [float(v) for v in got[0]])
    assert torch.equal(got, want), (got, want)
    assert torch.equal(got[:, 0], start) and float(start[0]) > R.MIN_EXACT
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(ba[k], bb[k]), k                         # the state advanced in place, as in the reference
    assert len(set(float(v) for v in got[0])) == n


@pytest.mark.gpu
def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same kernels: this file in a child process against it"""
    if flavours.is_experiments_process():
        return
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
