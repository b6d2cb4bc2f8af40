"""solveLinearSystemPCGBatched (fluidnet_amd/csrc/pcg_batched.inc) on the device: every batch item advances in the
same launches, and each item gets the BITS the sequential solver gives it alone. The mixed batches of tests/pcg_batched_cases.py
(held to their conditions by tests/test_pcg_batched_cases_cpu.py) against tfluids.solveLinearSystemPCG item by item, for 'mg'
and 'none', converged and at the rungs of the ladder; the coarse levels that run one launch per operation; the batched iterates
against the fp64 restatement with the bounds the sequential solver is held to (tests/pcg_mg_ref64.py: C_ITERATE, C_RESIDUAL);
the edges (B = 1, an item without fluid, permuted items, determinism); the refusals; calcPUTargets with mconf.pcgBatched."""
import ctypes
import functools

import numpy as np
import pytest

import pcg_batched_cases as C
import pcg_mg_ref64 as M
import pcg_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (tol, maxIter): a converged solve, then the rungs with a tolerance that never fires
SOLVES = ((1e-5, 1000), (R.TOL_NEVER, 0), (R.TOL_NEVER, 1), (R.TOL_NEVER, 3))


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _last_iterations():
    import torch
    from fluidnet_amd import tfluids
    return tfluids.pcgLastIterations(torch.empty(1, device=DEV))


def _sequential(f, div, is3d, tol, max_iter, pc):
    """(p, residuals, iterations) of tfluids.solveLinearSystemPCG on every item alone; p starts from noise (the solver zeroes it)"""
    import torch
    from fluidnet_amd import tfluids
    tf, td = _dev(f), _dev(div)
    p = torch.rand(td.shape, device=DEV)
    res, its = [], []
    for b in range(tf.shape[0]):
        pb = p[b:b + 1].clone()
        res.append(tfluids.solveLinearSystemPCG(pb, tf[b:b + 1].clone(), td[b:b + 1].clone(), is3d, tol, max_iter, pc))
        its.append(_last_iterations())
        p[b:b + 1] = pb
    return p, np.array(res, np.float32), np.array(its, np.int64)


def _batched(f, div, is3d, tol, max_iter, pc):
    import torch
    from fluidnet_amd import tfluids
    p = torch.rand(div.shape, device=DEV)
    res, its = tfluids.solveLinearSystemPCGBatched(p, _dev(f), _dev(div), is3d, tol, max_iter, pc)
    return p, res, its


@functools.lru_cache(maxsize=None)
def _sequential_of_batch(name, tol, max_iter, pc):
    f, _, div, is3d = C.batch(name)
    return _sequential(f, div, is3d, tol, max_iter, pc)


def _assert_same(got, want, what):
    (p, res, its), (ps, rs, is_) = got, want
    assert res.dtype == np.float32 and its.dtype == np.int64 and res.shape == rs.shape and its.shape == is_.shape, what
    print("PCGB %s: iterations %s (sequential %s), residuals %s" % (what, its.tolist(), is_.tolist(), res.tolist()))
    assert np.array_equal(its, is_), (what, its, is_)
    assert np.array_equal(res.view(np.uint32), rs.view(np.uint32)), (what, res, rs)
    same = _bits(p) == _bits(ps)
    assert same.all(), (what, "items that differ:", sorted(set(np.argwhere(~same)[:, 0].tolist())))
    assert _last_iterations() == int(is_.sum()), what


# ---- 1. the bits of the sequential solver -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_iter", SOLVES)
@pytest.mark.parametrize("pc", ["mg", "none"])
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_every_item_gets_the_bits_of_the_sequential_solver(oracle, name, pc, tol, max_iter):
    f, _, div, is3d = C.batch(name)
    want = _sequential_of_batch(name, tol, max_iter, pc)
    got = _batched(f, div, is3d, tol, max_iter, pc)      # (the last solve before _assert_same reads pcgLastIterations)
    _assert_same(got, want, "%s %s tol %g maxIter %d" % (name, pc, tol, max_iter))
    if tol > 0:
        assert (want[1] < 2 * tol).all() and len(set(want[2].tolist())) > 1, want[1:]


# ---- 2. coarse levels that run one launch per operation -------------------------------------------------------------------------
# dims: (the kinds of the two items, level count, first level of k_mg_coarse_b)
WIDE = {(1, 132, 136): (("box", "split"), 7, 2), (24, 36, 40): (("box", "split"), 4, 2),
        (1, 260, 264): (("box", "open"), 8, 3), (1, 8, 2100): (("box", "open"), 2, 2), (6, 6, 1000): (("box", "open"), 2, 2),
        (1, 4, 60): (("box", "open"), 1, 1), (4, 12, 14): (("box", "open"), 1, 1)}


@pytest.mark.parametrize("dims", list(WIDE))
def test_wide_coarse_levels(oracle, dims):
    """level 1 of the first two grids has more than kMgBlockCells = 4096 cells (66 x 68; 12 x 18 x 20): restriction, smoothing and
    prolongation of a level below level 0 as batched launches of their own. The others (pcg_mg_ref64.WIDE_SHAPES) with a closed
    and an open item, so that the launches of a level run with and without w as level 0's right-hand side: two levels below level 0
    as launches (260 x 264), no level for k_mg_coarse_b (the thin grids: first block level == level count), one level only"""
    kinds, count, first_block = WIDE[dims]
    levels = M.mg_levels(*dims, dims[0] > 1)
    cells = [z * y * x for z, y, x in levels]
    fb = M.first_block_level(levels)
    assert (len(levels), fb) == (count, first_block)
    assert all(n > M.BLOCK_CELLS for n in cells[1:fb]) and all(n <= M.BLOCK_CELLS for n in cells[fb:])
    assert count == 1 or cells[1] > 4096
    f, _, div, is3d = C.build_batch(oracle, dims, kinds, vel_cells=0.3)
    want = _sequential(f, div, is3d, 1e-4, 1000, "mg")
    _assert_same(_batched(f, div, is3d, 1e-4, 1000, "mg"), want, "wide %s" % (dims,))
    assert (want[1] < 2e-4).all(), want[1]


# ---- 3. an independent yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_batched_iterates_against_the_fp64_restatement(oracle, name):
    """rungs maxIter = 0, 1, 3 with a tolerance that never fires, with the checks and bounds test_hip_pcg_mg.py holds the sequential
    solver to: every cell within C_ITERATE max|p64| of its component, the solve's residual -- the largest of the items', what the
    sequential entry returns for the batch -- within C_RESIDUAL relative, exact zeros off the solved components. (That the inputs
    allow these bounds is checked on the CPU: test_pcg_batched_cases_cpu.py. The items' own residuals are printed: an item that
    has converged further than the one with the largest residual carries a larger relative error -- measured 3.7e-5 on the open
    item of `flat` at rung 3, whose fp32 restatement is off by 8.8e-6 -- and is held to the sequential solver's bits instead.)"""
    f, _, div, is3d = C.batch(name)
    ref = M.solve(f, div, is3d, "mg", M.DEPTH)
    for k in M.RUNGS:
        p, res, its = _batched(f, div, is3d, R.TOL_NEVER, k, "mg")
        p = p.cpu().numpy()
        err, zero = R.worst_error(p, ref["p"][k], ref)
        dres = abs(float(res.max()) - ref["res"][k]) / ref["res"][k]
        print("PCGB64 %s rung %d err %.2e (bound %.1e) residual %.2e (bound %.1e)" % (name, k, err, M.C_ITERATE, dres, M.C_RESIDUAL))
        for b, sizes in enumerate(ref["sizes"]):
            want = max(ref["res_comp"][(b, c)][k + 1] for c, n in enumerate(sizes) if n > 1)
            print("PCGB64 %s rung %d item %d residual %.6e (fp64 %.6e, off by %.2e relative)"
                  % (name, k, b, res[b], want, abs(float(res[b]) - want) / want))
            assert 0 < its[b] <= (k + 1) * sum(1 for n in sizes if n > 1)
        assert np.isfinite(p).all() and zero, (name, k)
        assert err <= M.C_ITERATE, (name, k, err)
        assert dres <= M.C_RESIDUAL, (name, k, float(res.max()), ref["res"][k])


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_one(oracle):
    f, _, div, is3d = C.batch("flat")
    f, div = f[1:2], div[1:2]
    _assert_same(_batched(f, div, is3d, 1e-5, 1000, "mg"), _sequential(f, div, is3d, 1e-5, 1000, "mg"), "B = 1")


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_an_item_without_fluid(oracle, name):
    """item 1 all obstacle: zeros, -inf and 0 iterations there, the neighbours as in the sequential solve"""
    f, _, div, is3d = C.batch(name)
    f, div = f[:3].copy(), div[:3].copy()
    f[1] = 2.0
    want = _sequential(f, div, is3d, 1e-5, 1000, "mg")
    got = _batched(f, div, is3d, 1e-5, 1000, "mg")
    _assert_same(got, want, "no fluid in item 1, %s" % name)
    assert float(got[0][1].abs().max()) == 0.0 and got[1][1] == -np.inf and got[2][1] == 0
    assert got[2][0] > 0 and got[2][2] > 0 and np.isfinite(got[1][[0, 2]]).all()


@pytest.mark.parametrize("pc", ["mg", "none"])
def test_permuting_the_items_permutes_the_outputs(oracle, pc):
    f, _, div, is3d = C.batch("vol")
    perm = [2, 0, 3, 1]
    p, res, its = _batched(f, div, is3d, 1e-5, 1000, pc)
    q, resq, itsq = _batched(f[perm], div[perm], is3d, 1e-5, 1000, pc)
    assert np.array_equal(_bits(q), _bits(p)[perm]) and np.array_equal(resq.view(np.uint32), res[perm].view(np.uint32))
    assert np.array_equal(itsq, its[perm])


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_the_batched_solve_is_deterministic(oracle, name):
    """two calls give the same bits, and so does one behind an unrelated matmul and an 'ic0' sequential solve through the same
    temp storage"""
    import torch
    from fluidnet_amd import tfluids
    f, _, div, is3d = C.batch(name)
    first = _batched(f, div, is3d, 1e-5, 1000, "mg")
    second = _batched(f, div, is3d, 1e-5, 1000, "mg")
    a = torch.rand(256, 256, device=DEV)
    (a @ a).sum().item()
    tfluids.solveLinearSystemPCG(torch.zeros(div.shape, device=DEV), _dev(f), _dev(div), is3d, 1e-5, 1000, "ic0")
    third = _batched(f, div, is3d, 1e-5, 1000, "mg")
    for other in (second, third):
        assert np.array_equal(_bits(other[0]), _bits(first[0]))
        assert np.array_equal(other[1].view(np.uint32), first[1].view(np.uint32)) and np.array_equal(other[2], first[2])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    import torch
    from fluidnet_amd import tfluids
    f, _, div, is3d = C.batch("flat")
    tf, td = _dev(f[:3]), _dev(div[:3])
    lib, ctx = tfluids._context(td)
    B, dims = 3, C.BATCHES["flat"]
    big = torch.empty(int(lib.tfl_pcg_batched_workspace_floats(B, *dims, b"mg")), device=DEV)
    for pc in ("ic0", "ilu0"):
        p = torch.rand(td.shape, device=DEV)
        with pytest.raises(tfluids.TfluidsError, match=pc):
            tfluids.solveLinearSystemPCGBatched(p, tf, td, is3d, 1e-5, 10, pc)
        rc = lib.tfl_solveLinearSystemPCGBatched(ctx, tfluids._tt(p), tfluids._tt(tf), tfluids._tt(td), 0, pc.encode(), 1e-5, 10,
                                                 ctypes.c_void_p(big.data_ptr()), big.numel(), None, None)
        assert rc == -3 and pc in lib.tfl_last_error(ctx).decode()                # TFL_EUNSUPPORTED, by name
    with pytest.raises(tfluids.TfluidsError, match="precondType is not supported"):
        tfluids.solveLinearSystemPCGBatched(torch.rand(td.shape, device=DEV), tf, td, is3d, 1e-5, 10, "multigrid")
    # the size query: -1 for a name that does not batch, growing with B for the two that do
    for pc in (b"ic0", b"ilu0", b"jacobi", None):
        assert int(lib.tfl_pcg_batched_workspace_floats(B, *dims, pc)) == -1
    sizes = {pc: [int(lib.tfl_pcg_batched_workspace_floats(n, *dims, pc)) for n in (1, 3)] for pc in (b"mg", b"none")}
    assert all(0 < s[0] < s[1] for s in sizes.values()) and sizes[b"none"][1] < sizes[b"mg"][1]
    assert sizes[b"mg"][0] >= int(lib.tfl_pcg_workspace_floats_for(*dims, b"mg"))
    # a short workspace
    need = sizes[b"mg"][1]
    ws = torch.empty(need, device=DEV)
    p = torch.rand(td.shape, device=DEV)
    res, its = np.zeros(B, np.float32), np.zeros(B, np.int64)

    def call(nws, r=res, i=its, flags=tf):
        return lib.tfl_solveLinearSystemPCGBatched(ctx, tfluids._tt(p), tfluids._tt(flags), tfluids._tt(td), 0, b"mg", 1e-5, 1000,
                                                   ctypes.c_void_p(ws.data_ptr()), nws,
                                                   r.ctypes.data_as(ctypes.c_void_p) if r is not None else None,
                                                   i.ctypes.data_as(ctypes.c_void_p) if i is not None else None)
    assert call(need - 1) != 0 and "tfl_pcg_batched_workspace_floats" in lib.tfl_last_error(ctx).decode()
    assert call(need) == 0 and (its > 0).all()
    want = p.clone()
    p.uniform_()
    assert call(need, None, None) == 0 and torch.equal(p, want)                    # either output table may be null
    # a fluid cell on the border of item 2 of 3: refused before any CG launch, p all zero
    fb = f[:3].copy()
    fb[2, 0, 0, 0, 5] = 1.0
    p = torch.rand(td.shape, device=DEV)
    with pytest.raises(tfluids.TfluidsError, match=r"fluid cell found on the domain border \(1 fluid border cells in batch item 2\)"):
        tfluids.solveLinearSystemPCGBatched(p, _dev(fb), td, is3d, 1e-5, 1000, "mg")
    assert float(p.abs().max()) == 0.0
    p.uniform_()
    assert call(need, flags=_dev(fb)) == -1 and float(p.abs().max()) == 0.0        # TFL_EINVAL


# ---- 6. calcPUTargets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_calcPUTargets_with_and_without_pcgBatched(oracle, name):
    """with mconf.pcgBatched the targets are the bits of composing by hand the sequential 'mg' solve (tol 1e-4) with the velocity
    update and the wall BCs; without the key, the bits of the same composition with 'ic0' (what the function does today)"""
    import torch
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import calcPUTargets
    f, U0, _, is3d = C.batch(name)
    f, U0 = f[:3], U0[:3]
    tf = _dev(f)

    def by_hand(pc):
        U = _dev(U0)
        tfluids.setWallBcsForward(U, tf)
        div = torch.empty_like(tf)
        tfluids.velocityDivergenceForward(U, tf, div)
        p = torch.rand(tf.shape, device=DEV)
        if pc == "ic0":
            tfluids.solveLinearSystemPCG(p, tf, div, is3d, 1e-4, 100, "ic0")
        else:
            for b in range(tf.shape[0]):
                pb = p[b:b + 1].clone()
                tfluids.solveLinearSystemPCG(pb, tf[b:b + 1].clone(), div[b:b + 1].clone(), is3d, 1e-4, 100, "mg")
                p[b:b + 1] = pb
        UT = U.clone()
        tfluids.velocityUpdateForward(UT, tf, p)
        tfluids.setWallBcsForward(UT, tf)
        return dict(pTarget=p, UTarget=UT, UDiv=U, div=div)

    for mconf, pc in ((dict(trainTargetSource="pcg", maxIter=100, pcgBatched=True, pcgPrecond="mg"), "mg"),
                      (dict(trainTargetSource="pcg", maxIter=100, pcgBatched=True), "mg"),
                      (dict(trainTargetSource="pcg", maxIter=100), "ic0")):
        batch = dict(UDiv=_dev(U0), flags=tf.clone(), pTarget=torch.rand(tf.shape, device=DEV), UTarget=torch.rand(U0.shape, device=DEV))
        calcPUTargets(None, mconf, batch)
        want = by_hand(pc)
        for k in ("pTarget", "UTarget", "UDiv", "div"):
            assert torch.equal(batch[k], want[k]), (mconf, k)
        assert float(batch["pTarget"].abs().max()) > 0
    assert not torch.equal(by_hand("mg")["pTarget"], by_hand("ic0")["pTarget"])


# ---- 7. the experiments flavour -------------------------------------------------------------------------------------------------------
def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same kernels: this file in a child process against it"""
    import os
    import subprocess
    import sys
    import flavours
    if flavours.is_experiments_process():
        return
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=root,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
