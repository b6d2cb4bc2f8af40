"""Every cell-type word, border included, through every flag reader of the library.

The parity tests hold the kernels to the oracle bit for bit on the flag fields tests/scenes.py make_scene / rough_scene can make:
obstacle blobs, stick on whole spheres, one slab of empty cells, an obstacle border. Here the fields are the flag ALPHABET
(scenes.ALPHABET: every cell-type bit, the composite words, the word 0) scattered over a third of the cells, on request over the
border shell too (scenes.alphabet_scene), and scenes.neighbourhood_scene, whose 3 x 3 (x 3) stencils run through every ordered
(centre word, face, neighbour word) triple and every pair of opposite-face words (the cover is asserted on the CPU,
tests/test_oracle.py). tests/flag_alphabet.py holds the shapes -- small and ragged against 64 x 4 blocks, 4 cells per thread and
6-wide guarded rows -- and the comparison; tests/test_oracle.py pins the oracle to the compiled reference on the same scenes.

An operator in which the oracle raises (a reference THError path) must report the same on the device (TfluidsError, or a non-zero
traceErrors()); one side alone is a failure. Run with -s for the compared-word counts; profiles/flag_alphabet.md keeps them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import flag_alphabet as FA
import scenes
from backward_cases import run_backward_ops_on
from flavours import child_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RUN = os.path.join(HERE, "flag_alphabet_run.py")
SWITCHES = ("TFL_VEL3_KZ", "TFL_SCAL3_TZ", "TFL_ADVECT_GATHER", "TFL_SCALAR_GATHER", "TFL_ADVECT_MODE", "TFL_SCAL3M_CZ_A", "TFL_SCAL3M_CZ_B",
            "TFL_SCAL3_MARCH", "TFL_ADV_PAIR", "TFL_VORT_FUSED", "TFL_VORT_PIPE", "TFL_VORT_CZ", "TFL_VORT_TILE", "TFL_JACOBI_LDS")


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    from hip_adapter import HipTfluids
    return HipTfluids()


def _report(name, words, t0, extra=""):
    print("%-58s words %9d mismatches 0  %.2fs %s" % (name, words, time.time() - t0, extra))


@pytest.mark.parametrize("kind,dims,border", FA.CASES, ids=FA.CASE_IDS)
def test_every_operator_bit_exact(hip, oracle, kind, dims, border):
    """run_ops (all six advection methods on both fields, setWallBcs, divergence, velocityUpdate, the two-launch confinement,
    buoyancy, gravity), the backward operators, setWallBcsBackward, the divergence norm (its own bound) and the result of
    flagsToOccupancy"""
    import torch
    import divnorm_ref as D
    from fluidnet_amd import tfluids
    t0 = time.time()
    name = FA.case_id(kind, dims, border)
    sc = FA.scene(kind, dims, border)
    hip.traceErrors()
    words, raised = FA.compare_ops(FA.guarded_ops(hip, sc), FA.guarded_ops(oracle, sc), name)
    assert hip.traceErrors() == 0
    seed = FA.seed_of(dims, kind, border)
    a, b = run_backward_ops_on(hip, sc, seed), run_backward_ops_on(oracle, sc, seed)
    for k in sorted(b):
        assert np.array_equal(a[k], b[k]), (name, k, int((a[k] != b[k]).sum()))
        words += b[k].size
    # setWallBcsBackward = mask * gradOutput with mask = setWallBcsForward(ones) (tfluids/set_wall_bcs.lua:50-66)
    g = np.random.RandomState(seed).randn(*sc["U"].shape).astype(np.float32)
    mask = np.ones_like(sc["U"])
    oracle.setWallBcsForward(mask, sc["flags"])
    assert np.array_equal(mask == 0, FA.wall_mask_np(sc["flags"], sc["is3d"]))
    tg, tf = torch.from_numpy(g).to(hip.dev), torch.from_numpy(sc["flags"]).to(hip.dev)
    got = tfluids.setWallBcsBackward(tf, tg).cpu().numpy()
    assert np.array_equal(got, mask * g), (name, "setWallBcsBackward", int((got != mask * g).sum()))
    words += got.size
    # the divergence norm, within the bound of tests/divnorm_ref.py
    exact = D.exact_norm(oracle, sc["U"], sc["flags"])
    norm = tfluids.velocityDivergenceNorm(torch.from_numpy(sc["U"]).to(hip.dev), tf).cpu().numpy()
    # (the comparison must not pass on nothing; on 3 x 3 x 3 a sample's one interior cell may hold no fluid: norm exactly 0)
    assert exact.max() > D.MIN_EXACT and (min(dims[1:]) == 3 or np.all(exact > D.MIN_EXACT)), (name, exact)
    assert np.all(np.abs(norm - exact) <= D.bound(dims, exact)), (name, norm, exact)
    # flagsToOccupancy: the CUDA build's contract on every word (fluid bit -> 0, obstacle bit -> 1, else -1, nothing raises);
    # on the two plain words that is also the compiled CPU function's answer (the oracle's)
    occ = np.full_like(sc["flags"], 5.0)
    hip.flagsToOccupancy(sc["flags"], occ)
    assert np.array_equal(occ, FA.occupancy_np(sc["flags"])), (name, int((occ != FA.occupancy_np(sc["flags"])).sum()))
    assert (occ == -1).any() and (occ == 0).any() and (occ == 1).any()
    words += occ.size
    if kind == "alphabet":
        so = scenes.alphabet_scene(dims, seed, B=FA.B, border=border, fluid_border=True, words=FA.PLAIN_WORDS)
        occ_a, occ_b = np.full_like(occ, 5.0), np.full_like(occ, 5.0)
        hip.flagsToOccupancy(so["flags"], occ_a)
        oracle.flagsToOccupancy(so["flags"], occ_b)
        assert np.array_equal(occ_a, occ_b)
        words += occ_a.size
    _report(name, words, t0, "raised on both sides: %s" % raised if raised else "")


def _child(mode, extra, timeout=600):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e = child_env(e, extra)
    t0 = time.time()
    r = subprocess.run([sys.executable, RUN, mode], env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "FLAG_ALPHABET_OK " + mode in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    words = int(r.stdout.split("words=")[1].split()[0])
    _report("%s %s" % (mode, extra), words, t0)


@pytest.mark.parametrize("env", [{}, {"TFL_VORT_FUSED": "1", "TFL_VORT_PIPE": "1"}, {"TFL_VORT_FUSED": "1", "TFL_VORT_PIPE": "0"}],
                         ids=["two-launch", "fused-pipelined", "fused-three-barrier"])
def test_vorticity_confinement_every_form(env):
    """in place and with USrc= (tfl_vorticityConfinementFrom), by default (small grids: the two launches) and with the fused
    route forced onto them, k_vort_pipe and k_vort_fused in turn"""
    _child("vort", env)


@pytest.mark.parametrize("env", [{}, {"TFL_VEL3_KZ": "1", "TFL_SCAL3_TZ": "1"}, {"TFL_VEL3_KZ": "2", "TFL_SCAL3_TZ": "12"},
                                 {"TFL_VEL3_KZ": "2", "TFL_SCAL3_TZ": "14"}, {"TFL_VEL3_KZ": "1", "TFL_SCAL3_TZ": "2"},
                                 {"TFL_SCAL3_MARCH": "1", "TFL_SCAL3M_CZ_A": "3", "TFL_SCAL3M_CZ_B": "2"}],
                         ids=["defaults", "kz1-scal-1x1", "kz2-scal-1x2", "kz2-scal-1x4", "kz1-scal-2x1", "marched"])
def test_advection_every_forced_block_shape(env):
    """all six methods in the exact mode on the 3-D cases under every forced block shape tests/test_hip_advect_bound.py lists"""
    _child("advect", env)


@pytest.mark.parametrize("env", [{}, {"TFL_JACOBI_LDS": "1"}, {"TFL_JACOBI_LDS": "0"}], ids=["default", "lds-on", "lds-off"])
def test_jacobi_generic_and_lds(env):
    """jacobi.hip:186: the one-launch LDS solve takes a 2-D grid of up to kJLdsMaxCells cells with a fixed iteration count unless
    TFL_JACOBI_LDS=0; the square grids of flag_alphabet_run.LDS_GRIDS are inside it, one or two per instantiation (1, 4 and 16
    cells per thread), so `lds-off` runs the launch-per-iteration kernel on the very same scenes"""
    _child("jacobi", env)


@pytest.mark.parametrize("kind,dims,border", FA.CASES, ids=FA.CASE_IDS)
def test_jacobi_every_case(hip, oracle, kind, dims, border):
    t0 = time.time()
    sc = FA.scene(kind, dims, border)
    f, U = sc["flags"], sc["U"].copy()
    oracle.setWallBcsForward(U, f)
    div = np.zeros_like(sc["p"])
    oracle.velocityDivergenceForward(U, f, div)
    words = 0
    for iters in (1, 2, 9):
        pa, pb = np.full_like(div, 3.0), np.full_like(div, -1.0)
        ra = oracle.solveLinearSystemJacobi(pa, f, div, sc["is3d"], 0.0, iters)
        rb = hip.solveLinearSystemJacobi(pb, f, div, sc["is3d"], 0.0, iters)
        assert np.array_equal(pa, pb), (iters, int((pa != pb).sum()))
        assert abs(ra - rb) <= 1e-5 * max(abs(ra), 1e-30), (ra, rb)
        words += pa.size
    _report("jacobi " + FA.case_id(kind, dims, border), words, t0)


PCG_CASES = [((1, 13, 21), False), ((5, 9, 21), False), ((1, 13, 21), True), ((5, 9, 21), True), ((4, 6, 68), True), ((1, 66, 130), True)]


@pytest.mark.parametrize("dims,border", PCG_CASES)
def test_pcg_on_the_alphabet(hip, oracle, dims, border):
    """all three preconditioners against the oracle with the tolerances of test_hip_parity's PCG test, on an alphabet scene
    without fluid on the border whose every multi-cell fluid component touches a cell that is neither fluid nor obstacle
    (checked, not assumed: the system is non-singular); then the refusal of fluid on the border"""
    from fluidnet_amd import TfluidsError
    from oracle.oracle import OracleError
    t0 = time.time()
    sc = FA.pcg_scene(dims, 77 + dims[2], border=border)
    f = sc["flags"]
    bad, multi, single = FA.singular_components(oracle, f, sc["is3d"])
    assert multi >= 2 and not any(bad), (multi, bad)
    U = sc["U"].copy()
    oracle.setWallBcsForward(U, f)
    div = np.zeros_like(sc["p"])
    oracle.velocityDivergenceForward(U, f, div)
    tol, words = 1e-5, 0
    nofluid = (f.astype(np.int64) & 1) == 0
    for pc in ("none", "ilu0", "ic0"):
        pa = np.random.RandomState(2).rand(*div.shape).astype(np.float32)
        pb = pa.copy()
        ra = hip.solveLinearSystemPCG(pa, f, div, sc["is3d"], tol, 1000, pc)
        rb = oracle.solveLinearSystemPCG(pb, f, div, sc["is3d"], tol, 1000, pc)
        assert ra < 2 * tol and rb < 2 * tol and np.isfinite(pa).all(), (pc, ra, rb)
        scale = max(np.abs(pb).max(), 1e-6)
        assert np.abs(pa - pb).max() < max(5e-5 * scale, 50 * tol), (pc, np.abs(pa - pb).max(), scale)
        assert np.all(pa[nofluid] == 0.0) and np.all(pb[nofluid] == 0.0)
        assert np.all(pa[single] == 0.0) and np.all(pb[single] == 0.0)          # a one-cell component is skipped
        words += pa.size
    fb = scenes.alphabet_scene(dims, 77 + dims[2], B=FA.B, border=True, fluid_border=True)["flags"]
    with pytest.raises(OracleError):
        oracle.solveLinearSystemPCG(np.zeros_like(div), fb, div, sc["is3d"], tol, 100, "none")
    with pytest.raises(TfluidsError):
        hip.solveLinearSystemPCG(np.zeros_like(div), fb, div, sc["is3d"], tol, 100, "none")
    _report("pcg %s border=%s (%d components)" % (dims, border, multi), words, t0)


def _layers2d():
    z = np.load(os.path.join(HERE, "golden", "myModel2D_weights.npz"))
    return [(z["w%d" % i], z["b%d" % i]) for i in range(5)]


# grids whose X is a multiple of four (the four-cells-per-thread k_bcs_div_stats_v4 / _code / k_project_v4) and not (the scalar
# forms); (8, 23, 52) and (1, 66, 132) x B = 2 hold the neighbourhood scene's full cover on the vec4 forms, (8, 23, 50) and
# (1, 66, 130) on the scalar ones
MODEL_CASES = [("alphabet", (5, 9, 36), False), ("alphabet", (5, 9, 36), True), ("alphabet", (6, 7, 130), True), ("alphabet", (5, 9, 21), True),
               ("neighbourhood", (8, 23, 52), False), ("neighbourhood", FA.COVER3, False), ("neighbourhood", (6, 7, 132), False),
               ("alphabet", (1, 13, 68), False), ("alphabet", (1, 13, 68), True), ("alphabet", (1, 9, 67), True),
               ("neighbourhood", (1, 66, 132), False), ("neighbourhood", (1, 66, 130), False)]


def _model_scene(kind, dims, border):
    seed = FA.seed_of(dims, kind, border) + 31
    if kind == "alphabet":          # (an open border holds fluid too: the model refuses nothing)
        return scenes.alphabet_scene(dims, seed, B=FA.B, border=border, fluid_border=True, vel_cells=0.4, noise=0.5)
    return scenes.neighbourhood_scene(dims, seed, B=FA.B, vel_cells=0.4, noise=0.5)


def _model(is3d):
    from fluidnet_amd import FluidNetModel
    return FluidNetModel.default_3d(seed=3) if is3d else FluidNetModel(_layers2d(), False)


@pytest.mark.parametrize("kind,dims,border", MODEL_CASES, ids=[FA.case_id(*c) for c in MODEL_CASES])
def test_model_flag_readers(oracle, monkeypatch, kind, dims, border):
    """model.forward on the FULL alphabet and on the neighbourhood scene (stick, empty, outflow, inflow, open, the composites, the
    word 0; alphabet scenes with `border` over the shell too, fluid included -- no kernel may lean on an obstacle border). The
    first forward with a flags tensor runs k_bcs_div_stats* / k_project* WITHOUT a wall plan, the second WITH one (k_wall_code,
    k_bcs_div_stats_code): they differ only in how they read flags and must agree bit for bit. The result is held to the
    per-voxel fp64 bound of tests/conv_bound.py against the oracle with the CUDA build's occupancy (FA.BitTestOccupancy: the
    net sees -1 at a cell that is neither fluid nor obstacle, on both sides), and U is bit-equal to the restatement wherever
    velocityUpdate leaves it alone -- a wrong setWallBcs or velocityUpdate decision at one cell is an O(1) error there."""
    import torch
    import conv_bound as CB
    from fluidnet_amd import simulate as sim, tfluids
    from oracle import simulate_np as S
    t0 = time.time()
    monkeypatch.setattr(sim, "_WALL_PLANS", True)          # (TFL_WALL_PLAN=0 in the environment must not turn both runs into one path)
    sc = _model_scene(kind, dims, border)
    is3d = sc["is3d"]
    model = _model(is3d)
    assert set(np.unique(sc["flags"]).astype(int)) == set(scenes.ALPHABET)
    if border:
        shell = scenes.border_mask(sc["flags"].shape, is3d)
        assert (sc["flags"][shell].astype(int) & 1).any() and (sc["flags"][shell].astype(int) & 128).any()
    dev = torch.device("cuda:0")
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    lib, ctx = tfluids._context(tU)
    p1, U1 = model.forward([tp, tU, tf])
    assert not sim._wall_cache.get(tf, tf), "the first forward with a flags tensor must run without a wall plan"
    p2, U2 = model.forward([tp, tU, tf])
    hit = sim._wall_cache.get(tf, tf)
    planned = bool(hit) and ctx in hit
    assert planned, "the second forward with the same flags must run with a wall plan"
    assert torch.equal(p1, p2) and torch.equal(U1, U2), (int((p1 != p2).sum()), int((U1 != U2).sum()))
    assert model.range_errors(tp) == 0
    p, U = p2.cpu().numpy(), U2.cpu().numpy()
    ops = FA.BitTestOccupancy(oracle)
    path = CB.conv_path(model, None)
    p64, U64, bp, bU, info = CB.forward_bound(ops, model, sc["p"], sc["U"], sc["flags"], path=path)
    p_ref, U_ref = S.model_forward(ops, model.layers, sc["p"], sc["U"], sc["flags"], pool=model.pool, up=model.up, opts=model.opts)
    assert np.isfinite(p).all() and np.isfinite(U).all()
    for b in range(p.shape[0]):
        assert CB.worst(p[b:b + 1], p64[b:b + 1], bp[b:b + 1])[0] <= 1.0, CB.report("p", p[b:b + 1], p64[b:b + 1], bp[b:b + 1], (32, 8, 4))
        assert CB.worst(U[b:b + 1], U64[b:b + 1], bU[b:b + 1])[0] <= 1.0, CB.report("U", U[b:b + 1], U64[b:b + 1], bU[b:b + 1], (32, 8, 4))
    m = info["untouched"]
    assert m.any() and np.array_equal(U[m], U_ref[m]), int((U[m] != U_ref[m]).sum())
    _report("model " + FA.case_id(kind, dims, border), 2 * (p.size + U.size), t0,
            "plan %s, max err/bound p %.3g U %.3g" % (planned, CB.worst(p, p64, bp)[0], CB.worst(U, U64, bU)[0]))


@pytest.mark.parametrize("kind,dims,border", MODEL_CASES, ids=[FA.case_id(*c) for c in MODEL_CASES])
def test_model_begin_bit_exact(oracle, monkeypatch, kind, dims, border):
    """model.begin = setWallBcs in place + divergence + {sum u, sum u^2} (k_bcs_div_stats*, no occupancy involved): U bit-equal
    to oracle.setWallBcsForward without a plan (first call with the flags tensor) and with one (second call), the sums within
    the rounding of an fp64 sum of N terms in any order, N 2^-53 sum|x|"""
    import torch
    from fluidnet_amd import simulate as sim, tfluids
    t0 = time.time()
    monkeypatch.setattr(sim, "_WALL_PLANS", True)
    sc = _model_scene(kind, dims, border)
    model = _model(sc["is3d"])
    want = sc["U"].copy()
    oracle.setWallBcsForward(want, sc["flags"])
    dev = torch.device("cuda:0")
    tf = torch.from_numpy(sc["flags"]).to(dev)
    lib, ctx = tfluids._context(tf)
    x = want.astype(np.float64).reshape(want.shape[0], -1)
    n = x.shape[1]
    words = 0
    for call in range(2):
        tU = torch.from_numpy(sc["U"]).to(dev)
        stats = torch.zeros(want.shape[0], 2, dtype=torch.float64, device=dev)
        model.begin(tU, tf, 0, dims[0], stats)
        hit = sim._wall_cache.get(tf, tf)
        assert (bool(hit) and ctx in hit) == (call == 1), call
        got = tU.cpu().numpy()
        assert np.array_equal(got, want), (call, int((got != want).sum()))
        st = stats.cpu().numpy()
        assert np.all(np.abs(st[:, 0] - x.sum(1)) <= n * 2.0 ** -53 * np.abs(x).sum(1) + 1e-300), (call, st[:, 0], x.sum(1))
        assert np.all(np.abs(st[:, 1] - (x * x).sum(1)) <= n * 2.0 ** -53 * (x * x).sum(1) + 1e-300), (call, st[:, 1], (x * x).sum(1))
        words += got.size
    _report("model.begin " + FA.case_id(kind, dims, border), words, t0)


# ---- the native step and the z-slab step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_steps_on_an_alphabet_plume(oracle, world):
    """two steps with the Jacobi projection: simulate() and the z-slab step (virtual ranks on uneven cuts) against
    oracle/simulate_np.simulate, bit for bit; the un-cut native step in between"""
    import torch
    import test_hip_simulate as T
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate, simulate_native
    from oracle import simulate_np as S
    t0 = time.time()
    dev = torch.device("cuda:0")
    nb = FA.plume(9 * world + 4, scenes.ALPHABET, 5 + world)
    conf = M.mconf("maccormackOurs")
    ta, tb, tc = T._to_dev(nb, dev), T._to_dev(nb, dev), T._to_dev(nb, dev)
    sims = J.slab_sims(tc, conf, J.uneven_cuts(nb["flags"].shape[2], world))
    for _ in range(2):
        S.simulate(oracle, conf, nb, None)
        simulate(None, conf, ta, None)
        simulate_native(None, conf, tb, None)
    run_virtual_ranks(sims, 2)
    words = 0
    for k in ("pDiv", "UDiv", "density"):
        assert np.array_equal(ta[k].cpu().numpy(), nb[k]), ("simulate", k, int((ta[k].cpu().numpy() != nb[k]).sum()))
        assert torch.equal(ta[k], tb[k]), ("simulate_native", k)
        words += 3 * nb[k].size
    J.assert_owned_equal(sims, tb)
    for s in sims:
        s.close()
    assert float(np.abs(nb["pDiv"]).max()) > 0
    _report("steps jacobi world %d" % world, words, t0)


def test_convnet_step_slab_equals_uncut():
    """the ConvNet projection on an alphabet plume: exact at world 1, within 1e-7 at world 2 (the fp64
    summation order of the std all-reduce), as tests/test_hip_slab_methods.py holds its scenes"""
    import torch
    import test_hip_simulate as T
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    from fluidnet_amd import FluidNetModel
    from oracle import simulate_np as S
    t0 = time.time()
    layers = S.default_3d_layers(seed=2)
    conf = M.mconf("maccormackOurs", "convnet")
    words = 0
    for world, tol in ((1, 0.0), (2, 1e-7)):
        ref = T._to_dev(FA.plume(9 * world + 4, scenes.ALPHABET, 9, 24, 32), torch.device("cuda:0"))
        sims = M.sims_for(ref, conf, J.uneven_cuts(ref["flags"].size(2), world), layers=layers)
        M.run_and_compare(ref, conf, sims, model=FluidNetModel(layers, True), tol=tol, rounds=1, steps=2)
        words += sum(ref[k].numel() for k in ("pDiv", "UDiv", "density"))        # the ranks' owned planes tile the grid
    _report("steps convnet world 1, 2", words, t0, "world 1 in bits, world 2 within 1e-7 (rel-L2 per field and rank)")


@pytest.mark.parametrize("env", [{"TFL_ADV_PAIR": "0"}, {"TFL_ADV_PAIR": "1"}], ids=["separate-advection-kernels", "pair-kernels"])
def test_slab_step_without_and_with_the_pair_kernels(env):
    """the z-slab step's fused advection pair kernels (advect_pair3.hip) switched off and on (read once per process): two steps
    of the un-cut native step against the oracle, and virtual ranks at world 2 and 3 against the un-cut step, bit for bit"""
    _child("slab", env)
