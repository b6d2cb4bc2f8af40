"""GPU checks of the generator's batched form: a set generated R runs at a time holds the VALUES of the set
generated one run at a time -- torch.equal throughout (the sign of a zero is outside the contract: the identity-pair note there).
 1. the per-item force operators against per-item calls of the single-item operators on B = 1 slices, the scalar and the
    four-cell paths, a misaligned view, an item that is off coming back bit for bit (-0 and NaN included);
 2. simulate_items against simulate_native item by item, and outputDiv + project_items against one items step;
 3. generate(batch_runs=R) against generate(): every tensor of every slot, runs, report, the files of the disk sink;
 4. the same with a divergence threshold that makes the serial generator retry a run;
 5. the refusals, each leaving every tensor untouched;
 6. twice the same behind another solve, and this file against the second library flavour."""
import ctypes
import filecmp
import os
import warnings

import numpy as np
import pytest
import torch

import datagen_batched_cases as C
import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")
STATE = ("pDiv", "UDiv", "density")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the per-item force operators -----------------------------------------------------------------------------------------------
# items: on, off, on along another axis with another strength
GRAV = ([0.0, -0.7, 0.0], [0.3, 0.3, 0.3], [1.3, 0.0, 0.25])
AMPS = (0.4, 9.0, 0.07)
ON = (1, 0, 1)
KERNEL_SHAPES = [((1, 9, 13), False), ((1, 12, 16), False), ((5, 6, 7), False), ((6, 8, 12), False), ((1, 12, 16), True), ((6, 8, 12), True)]


def _pattern(shape):
    """what the item that is off holds: -0, a NaN, and ordinary words"""
    t = torch.arange(int(np.prod(shape)), device=DEV, dtype=torch.float32).reshape(shape).remainder(7.0) - 3.0
    flat = t.view(-1)
    flat[::3] = -0.0
    flat[1::5] = float("nan")
    return t


def _offset(t):
    """the same values in a tensor that starts 4 bytes behind a 16-byte boundary: the four-cell kernels must not take it"""
    buf = torch.empty(t.numel() + 1, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("dims,misaligned", KERNEL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("off4" if v else "al"))
def test_item_force_operators_equal_the_single_item_operators(dims, misaligned):
    from fluidnet_amd import tfluids
    sc = scenes.rough_scene(dims, seed=5, B=3, obstacle_frac=0.12, empty_frac=0.12)
    is3D, dt = sc["is3d"], 0.1
    flags, rho = _dev(sc["flags"]), _dev(sc["density"])
    assert int((flags == scenes.OBSTACLE).sum()) > 0 and int((flags == scenes.EMPTY).sum()) > 0
    U0 = _dev(sc["U"])
    U0[1] = _pattern(U0[1].shape)
    place = _offset if misaligned else (lambda t: t.clone())

    def single(op, b):
        Ub = U0[b:b + 1].clone()
        op(Ub, flags[b:b + 1].clone(), b)
        return Ub

    def check(U, op, what):
        for b in range(3):
            if ON[b]:
                assert torch.equal(U[b:b + 1], single(op, b)), (what, b)
                assert not torch.equal(U[b], U0[b]), (what, b)       # the force did something
            else:
                assert torch.equal(_bits(U[b]), _bits(U0[b])), (what, b)

    U = place(U0)
    tfluids.addBuoyancyItems(U, flags, rho, GRAV, dt, on=ON)
    check(U, lambda Ub, fb, b: tfluids.addBuoyancy(Ub, fb, rho[b:b + 1].clone(), GRAV[b], dt), "buoyancy in place")
    # source != destination: every cell written, the item that is off copied
    Usrc, U = place(U0), place(torch.full_like(U0, 7.0))
    tfluids.addBuoyancyItems(U, flags, rho, GRAV, dt, on=ON, USrc=Usrc)
    check(U, lambda Ub, fb, b: tfluids.addBuoyancy(Ub, fb, rho[b:b + 1].clone(), GRAV[b], dt), "buoyancy from")
    assert torch.equal(_bits(Usrc), _bits(U0))
    U = place(U0)
    tfluids.addGravityItems(U, flags, GRAV, dt, on=ON)
    check(U, lambda Ub, fb, b: tfluids.addGravity(Ub, fb, GRAV[b], dt), "gravity")
    U = place(U0)
    tfluids.vorticityConfinementItems(U, flags, AMPS, on=ON)
    check(U, lambda Ub, fb, b: tfluids.vorticityConfinement(Ub, fb, AMPS[b]), "confinement")
    # on = None: every item has the force (item 1 holds ordinary words here)
    U1 = _dev(sc["U"])
    U = place(U1)
    tfluids.addGravityItems(U, flags, GRAV, dt)
    for b in range(3):
        Ub = U1[b:b + 1].clone()
        tfluids.addGravity(Ub, flags[b:b + 1].clone(), GRAV[b], dt)
        assert torch.equal(U[b:b + 1], Ub), b


def test_item_force_operators_refuse_by_name():
    from fluidnet_amd import TfluidsError, tfluids
    sc = scenes.rough_scene((1, 8, 8), seed=1, B=2)
    flags, U = _dev(sc["flags"]), _dev(sc["U"])
    keep = U.clone()
    with pytest.raises(TfluidsError, match="n_items = 3, the batch holds 2"):
        tfluids.addGravityItems(U, flags, GRAV, 0.1)
    with pytest.raises(TfluidsError, match="n_items = 3, the batch holds 2"):
        tfluids.vorticityConfinementItems(U, flags, AMPS)
    big = scenes.rough_scene((1, 8, 8), seed=1, B=33)
    with pytest.raises(TfluidsError, match="33 items, at most 32"):
        tfluids.addBuoyancyItems(_dev(big["U"]), _dev(big["flags"]), _dev(big["density"]), [[0.0, 1.0, 0.0]] * 33, 0.1)
    assert torch.equal(U, keep)


# ---- 2. the step on items -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=C.CASES, ids=["2d", "3d"])
def step_states(request):
    """(is3D, plans, the S_0 of plans 0, 3, 4, 6 as B = 1 batches): computed once, cloned by every test"""
    from fluidnet_amd import datagen
    is3D, dims = request.param
    plans = C.plans(is3D, dims, C.STEP_PLANS, pcgPrecond="mg")
    return is3D, plans, [datagen.init_state(p, DEV) for p in plans]


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


def _forces(plans):
    from fluidnet_amd import datagen
    return [{k: datagen.mconf_of(p)[k] for k in ("gravity", "buoyancyScale", "gravityScale", "vorticityConfinementAmp")} for p in plans]


def _step_both(plans, states, over, forces, steps=3):
    """`steps` steps of the batch on items and of every item alone (simulate_native); compared after every step"""
    from fluidnet_amd import datagen
    from fluidnet_amd.simulate import simulate_items, simulate_native
    mconf = dict(datagen.mconf_of(plans[0]), **over)
    batch = datagen.join_states([_clone(s) for s in states])
    alone = [_clone(s) for s in states]
    for step in range(steps):
        simulate_items(None, mconf, batch, forces)
        for b, one in enumerate(alone):
            simulate_native(None, dict(mconf, **(forces[b] if forces is not None else {})), one, None)
            for k in STATE:
                assert torch.equal(batch[k][b:b + 1], one[k]), (over, step, b, k)
    assert float(batch["pDiv"].abs().max()) > 0 and not bool(torch.isnan(batch["UDiv"]).any())
    return batch


STEP_VARIANTS = [dict(simMethod="pcg", pcgPrecond="mg"), dict(simMethod="pcg", pcgPrecond="none"), dict(simMethod="jacobi"),
                 dict(simMethod="pcg", pcgPrecond="mg", advectionMethod="maccormackOurs"),
                 dict(simMethod="pcg", pcgPrecond="mg", gravityScale=0.75)]


@pytest.mark.parametrize("over", STEP_VARIANTS, ids=["mg", "none", "jacobi", "ours", "gravity"])
def test_step_on_items_equals_the_step_of_every_item_alone(step_states, over):
    is3D, plans, states = step_states
    forces = _forces(plans)
    if "gravityScale" in over:      # addGravity on two of the four items, each along its own axis
        over = {k: v for k, v in over.items() if k != "gravityScale"}
        for b in (1, 3):
            forces[b] = dict(forces[b], gravityScale=0.75 + b)
    _step_both(plans, states, over, forces)


def test_step_on_items_with_shared_forces(step_states):
    """items = None: every item takes mconf's own forces (those of plan 0 here, gravity included)"""
    is3D, plans, states = step_states
    _step_both(plans, states, dict(pcgPrecond="mg", buoyancyScale=1.25, vorticityConfinementAmp=0.3, gravityScale=0.5), None)


@pytest.mark.parametrize("over", [dict(simMethod="pcg", pcgPrecond="mg"), dict(simMethod="jacobi")], ids=["mg", "jacobi"])
def test_outputdiv_items_step_and_project_items_give_one_items_step(step_states, over):
    from fluidnet_amd import datagen
    from fluidnet_amd.simulate import project_items, simulate_items
    is3D, plans, states = step_states
    forces, mconf = _forces(plans), dict(datagen.mconf_of(plans[0]), **over)
    one = datagen.join_states([_clone(s) for s in states])
    two = datagen.join_states([_clone(s) for s in states])
    for step in range(3):
        simulate_items(None, mconf, one, forces)
        before = two["pDiv"].clone()
        simulate_items(None, mconf, two, forces, outputDiv=True)
        assert torch.equal(two["pDiv"], before) and not torch.equal(two["UDiv"], one["UDiv"])      # p untouched, U divergent
        project_items(None, mconf, two, forces)
        for k in STATE:
            assert torch.equal(one[k], two[k]), (over, step, k)


def test_step_on_items_with_the_sequential_preconditioner():
    """'ic0' does not batch: the items step runs the sequential solver, serial over the items"""
    from fluidnet_amd import datagen
    plans = C.plans(False, (1, 16, 16), (0, 3))
    states = [datagen.init_state(p, DEV) for p in plans]
    _step_both(plans, states, dict(simMethod="pcg", pcgPrecond="ic0"), _forces(plans))


# ---- 3. the generator -----------------------------------------------------------------------------------------------------------------
def _gather_all(store, is3D, dims, n):
    Cv = 3 if is3D else 2
    out = {k: torch.empty((n, Cv if k in ("UDiv", "UTarget") else 1) + tuple(dims), device=DEV) for k in KEYS}
    store.gather(range(n), out)
    return out


def _generate(is3D, dims, nruns, batch_runs, out_dir=None, **over):
    """generate() into a store of its own -> (result without the data set, every tensor of every slot)"""
    from fluidnet_amd import datagen
    from fluidnet_amd.data import FrameStore
    kw = dict(pcgPrecond="mg", divThreshold=None)
    kw.update(over)
    g = C.gconf(is3D, dims, **kw)
    frames = len(datagen.saved_steps(g))
    store = FrameStore(DEV, is3D, *dims, nruns * frames, nruns * frames)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            res = datagen.generate(g, "tr", nruns, C.SEED, out_dir=out_dir, store=store, device=DEV, batch_runs=batch_runs)
        got = _gather_all(store, is3D, dims, nruns * frames)
    finally:
        store.close()
    return dict(runs=res["runs"], report=res["report"], warnings=sorted(str(w.message) for w in caught)), got


def _same_set(a, b, what):
    (ra, ta), (rb, tb) = a, b
    assert ra["runs"] == rb["runs"] and ra["report"] == rb["report"] and ra["warnings"] == rb["warnings"], (what, ra, rb)
    for k in KEYS:
        assert torch.equal(ta[k], tb[k]), (what, k)


@pytest.fixture(scope="module", params=C.CASES, ids=["2d", "3d"])
def serial_set(request):
    is3D, dims = request.param
    return is3D, dims, _generate(is3D, dims, C.RUNS, 1)


@pytest.mark.parametrize("R", [4, 8])
def test_generate_in_waves_holds_the_serial_set(serial_set, R):
    is3D, dims, want = serial_set
    assert [r[0] for r in want[0]["runs"]] == ["%06d" % i for i in range(C.RUNS)] and float(want[1]["densityTarget"].max()) > 0.1
    print("max div(U target) per run, serial:", [r["max_div"] for r in want[0]["report"]])
    _same_set(_generate(is3D, dims, C.RUNS, R), want, (dims, R))


@pytest.mark.parametrize("over", [dict(pcgPrecond="none"), dict(emitterSpeed=0.5)], ids=["none", "ubc"])
def test_generate_in_waves_other_configurations_2d(over):
    is3D, dims = C.CASES[0]
    _same_set(_generate(is3D, dims, C.RUNS, 4, **over), _generate(is3D, dims, C.RUNS, 1, **over), over)


def test_generate_in_waves_partial_wave_and_disk_sink(tmp_path):
    is3D, dims = C.CASES[0]
    a, b = str(tmp_path / "serial"), str(tmp_path / "waves")
    _same_set(_generate(is3D, dims, 5, 4, out_dir=b), _generate(is3D, dims, 5, 1, out_dir=a), "partial wave")
    files = sorted(os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs)
    assert len(files) == 5 * 6 * 2
    match, mismatch, errors = filecmp.cmpfiles(a, b, files, shallow=False)
    assert sorted(match) == files and not mismatch and not errors
    assert sorted(os.path.relpath(os.path.join(d, f), b) for d, _, fs in os.walk(b) for f in fs) == files


def test_generate_in_waves_into_a_scratch_store(tmp_path):
    """without a caller's store the scratch store holds R runs: the files are the serial generator's"""
    from fluidnet_amd import datagen
    is3D, dims = C.CASES[0]
    g = C.gconf(is3D, dims, pcgPrecond="mg", divThreshold=None)
    a, b = str(tmp_path / "serial"), str(tmp_path / "waves")
    ra = datagen.generate(g, "te", 3, C.SEED, out_dir=a, device=DEV, first_run=2)
    rb = datagen.generate(g, "te", 3, C.SEED, out_dir=b, device=DEV, first_run=2, batch_runs=2)
    assert (ra["runs"], ra["report"]) == (rb["runs"], rb["report"]) and ra["runs"][0][0] == "000002"
    files = sorted(os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs)
    match, mismatch, errors = filecmp.cmpfiles(a, b, files, shallow=False)
    assert len(files) == 3 * 6 * 2 and sorted(match) == files and not mismatch and not errors


# ---- 4. a retried run -------------------------------------------------------------------------------------------------------------------
# A measured constant. max div(U target) of the runs of the 2-D case (1x32x32, 'mg', seed 11, 12 steps, every 2nd saved) on an
# MI355X, attempts 0 | 1 | 2:
#   run 0  5.245e-06 | 8.991e-06 | 6.318e-06      run 4  1.1146e-05 | 5.066e-06 | 4.858e-06
#   run 1  5.867e-06 | 7.689e-06 | 5.126e-06      run 5  1.0967e-05 | 1.0870e-05 | 5.230e-06
#   run 2  7.361e-06 | 6.534e-06 | 8.911e-06      run 6  4.113e-06 | 6.765e-06 | 1.1086e-05
#   run 3  3.755e-06 | 1.0252e-05 | 4.962e-06     run 7  4.292e-06 | 7.033e-06 | 2.2173e-05
# The threshold lies between the third largest and the second largest of the first attempts (7.361e-06, 1.0967e-05): the serial
# generator drops runs 4 and 5, keeps run 4 at attempt 1 and run 5 -- whose attempt 1 is above it again -- at attempt 2.
RETRY_THRESHOLD = 9.0e-06


def test_generate_in_waves_retries_what_the_serial_generator_retries():
    """divThreshold between two of the serial set's max_divs, so that the serial generator completes with retried runs: batched
    and serial then give the same report, the same warnings and the same store."""
    is3D, dims = C.CASES[0]
    want = _generate(is3D, dims, C.RUNS, 1, divThreshold=RETRY_THRESHOLD)
    print("report:", want[0]["report"])
    assert any(r["attempt"] == 1 for r in want[0]["report"]) and any(not r["kept"] for r in want[0]["report"])      # a retry really happened
    assert [(r["run"], r["attempt"], r["kept"]) for r in want[0]["report"] if r["run"] in (4, 5)] == \
        [(4, 0, False), (4, 1, True), (5, 0, False), (5, 1, False), (5, 2, True)]
    assert len(want[0]["runs"]) == C.RUNS and len(want[0]["warnings"]) == sum(1 for r in want[0]["report"] if not r["kept"])
    for R in (4, 8):
        _same_set(_generate(is3D, dims, C.RUNS, R, divThreshold=RETRY_THRESHOLD), want, ("retry", R))


# ---- 5. the refusals --------------------------------------------------------------------------------------------------------------------
def _raw_items_call(mconf, batch, n_items, short=0, entry="tfl_simulate_step_items"):
    """the entry itself with a chosen item count and a workspace `short` floats below what the step asks for"""
    from fluidnet_amd import tfluids
    from fluidnet_amd._lib import tfl_sim_item
    from fluidnet_amd.simulate import _native_args
    U = batch["UDiv"]
    lib, ctx = tfluids._context(U)
    prm, st, keep = _native_args(lib, ctx, mconf, batch, None, False)
    nws = int(lib.tfl_simulate_items_workspace_floats(ctx, ctypes.byref(prm), ctypes.byref(st)))
    ws = torch.empty(nws + 8, device=U.device)
    items = (tfl_sim_item * max(n_items, 1))()
    tfluids._call(lib, ctx, getattr(lib, entry)(ctx, ctypes.byref(prm), items, n_items, ctypes.byref(st), ctypes.c_void_p(ws.data_ptr()),
                                                nws - short))
    del keep


def test_items_step_refusals_leave_every_tensor_untouched(step_states):
    from fluidnet_amd import TfluidsError, datagen, tfluids
    from fluidnet_amd.simulate import project_items, simulate_items
    is3D, plans, states = step_states
    batch = datagen.join_states([_clone(s) for s in states])
    keep = _clone(batch)
    mconf, forces = dict(datagen.mconf_of(plans[0]), pcgPrecond="mg"), _forces(plans)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(_bits(batch[k]), _bits(keep[k])) for k in keep)

    with pytest.raises(TfluidsError, match="simulate_step_items: simMethod convnet is not stepped on items"):
        simulate_items(None, dict(mconf, simMethod="convnet"), batch, forces)
    with pytest.raises(TfluidsError, match="simulate_step_items: mconf.simMethod is not a valid option"):
        simulate_items(None, dict(mconf, simMethod="sor"), batch, forces)
    with pytest.raises(TfluidsError, match="simulate_project_items: pcgPrecond 'jacobi' is not a preconditioner"):
        project_items(None, dict(mconf, pcgPrecond="jacobi"), batch, forces)
    with pytest.raises(TfluidsError, match="simulate_step_items: n_items = 3, the batch holds 4"):
        simulate_items(None, mconf, batch, forces[:3])
    with pytest.raises(TfluidsError, match="simulate_step_items: a force field of item 2 is not finite"):
        simulate_items(None, mconf, batch, forces[:2] + [dict(forces[2], buoyancyScale=float("inf"))] + forces[3:])
    with pytest.raises(TfluidsError, match=r"simulate_step_items: the workspace holds \d+ floats, the step needs \d+"):
        _raw_items_call(mconf, batch, 4, short=1)
    with pytest.raises(TfluidsError, match=r"simulate_project_items: the workspace holds \d+ floats, the step needs \d+"):
        _raw_items_call(mconf, batch, 4, short=1, entry="tfl_simulate_project_items")
    assert untouched()
    _raw_items_call(mconf, batch, 4, short=0)      # exact to one float: the full size is taken
    assert not untouched()
    for k in keep:
        batch[k].copy_(keep[k])
    lib, ctx = tfluids._context(batch["UDiv"])
    try:
        assert lib.tfl_set_z_window(ctx, 0, 1, 0, 0) == 0
        with pytest.raises(TfluidsError, match="simulate_step_items: a z-window or stage mask is set on the context"):
            simulate_items(None, mconf, batch, forces)
    finally:
        assert lib.tfl_set_z_window(ctx, 0, 0, 0, 0) == 0
    assert untouched()
    # 33 items
    tiny = datagen.init_state(C.plans(False, (1, 16, 16), (0,), pcgPrecond="mg")[0], DEV)
    many = datagen.join_states([tiny] * 33)
    keep33 = _clone(many)
    with pytest.raises(TfluidsError, match="simulate_step_items: 33 items, at most 32"):
        simulate_items(None, mconf, many, None)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(many[k]), _bits(keep33[k])) for k in keep33)


# ---- 6. determinism, the second flavour --------------------------------------------------------------------------------------------
def test_items_step_twice_the_same_behind_another_solve(step_states):
    from fluidnet_amd import datagen
    is3D, plans, states = step_states
    first = _step_both(plans, states, dict(simMethod="pcg", pcgPrecond="mg"), _forces(plans), steps=2)
    # another solve of another shape in between (the S_0 of a plan of the other case projects its noise field with 'none'): the
    # grow-only scratch buffer and the context's solver state are not what the first pass found
    other_3d, other_dims = C.CASES[0] if is3D else C.CASES[1]
    datagen.init_state(C.plans(other_3d, other_dims, (1,), pcgPrecond="none")[0], DEV)
    second = _step_both(plans, states, dict(simMethod="pcg", pcgPrecond="mg"), _forces(plans), steps=2)
    for k in STATE:
        assert torch.equal(_bits(first[k]), _bits(second[k])), k


def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same kernels: this file in a child process against it"""
    import subprocess
    import sys
    import flavours
    if flavours.is_experiments_process():
        return
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "-k", "operators or step_on_items or partial_wave"], cwd=root,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
