"""The fp64 restatement of the multigrid preconditioner (tests/pcg_mg_ref64.py) held to what the device test relies on, on the
CPU: the V-cycle is symmetric and positive on every component of every case (and the 'mean' mutant is not symmetric), converged
mg-PCG reaches the compiled oracle's 'ic0' solution within the bound of test_hip_parity.py's PCG test, mg takes at most half the
iterations of 'ic0', the iterate bound C_ITERATE is 4 x what fp32 costs the restatement itself, and every mutant is more than 100
bounds away at the first rung. The same for WIDE_CASES, the grids whose coarse levels run one launch per operation: the conditions
on the inputs, one bound per rung pinned to the measurement, and mutants that live on one coarse level."""
import numpy as np
import pytest

import pcg_mg_ref64 as M
import pcg_ref64 as R


def _components(name, dtype=np.float64, mutate=None):
    f, _, is3d = M.case(name)
    for b in range(f.shape[0]):
        comp, sizes = R.label_components(f[b, 0], is3d)
        for c, size in enumerate(sizes):
            if size >= 5:
                yield (b, c), M.MgComponent(f[b, 0], comp, c, is3d, dtype, mutate)


def _asym(apply, u, v):
    a, b = float(u @ apply(v)), float(v @ apply(u))
    return abs(a - b) / max(abs(a), abs(b))


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_the_cycle_is_symmetric_and_positive(oracle, name):
    """u.M^-1 v = v.M^-1 u to 1e-12 relative and u.M^-1 u > 0 on random vectors, for every component: the bare V-cycle on any
    vector, and the preconditioner as CG applies it (on a closed component: the cycle behind the removal of the mean) on vectors
    of its domain, the range of A; restriction as a mean instead of a sum is not symmetric"""
    rng = np.random.RandomState(7)
    seen = 0
    for key, C in _components(name):
        Cm = next(m for k, m in _components(name, mutate="restrict_mean") if k == key)
        for _ in range(3):
            u, v = (rng.randn(C.mask.size) * C.mask for _ in range(2))
            assert _asym(C.cycle, u, v) <= 1e-12 and float(u @ C.cycle(u)) > 0 and float(v @ C.cycle(v)) > 0, (name, key)
            if C.closed:
                u, v = (w - (w.sum() / C.mask.sum()) * C.mask for w in (u, v))
            assert _asym(C.precond, u, v) <= 1e-12 and float(u @ C.precond(u)) > 0, (name, key)
            assert _asym(Cm.cycle, u, v) > 1e-6, (name, key)
        seen += 1
    assert seen >= 1


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_converged_mg_pcg_equals_the_oracles_ic0_solution(oracle, name):
    f, div, is3d = M.case(name)
    tol = 1e-5
    out = M.solve(f, div, is3d, "mg", 200, tol=tol, max_iter=1000)
    p = out["p"][-1]
    pb = np.zeros_like(div)
    rb = oracle.solveLinearSystemPCG(pb, f, div, is3d, tol, 1000, "ic0")
    scale = max(np.abs(pb).max(), 1e-6)
    assert out["res"][-1] < 2 * tol and rb < 2 * tol
    assert np.abs(p - pb).max() < max(5e-5 * scale, 50 * tol), (np.abs(p - pb).max(), scale)
    assert np.all(p[f != 1.0] == 0.0)


@pytest.mark.parametrize("name", M.RATIO_CASES)
def test_mg_takes_at_most_half_of_ic0s_iterations(oracle, name):
    assert M.cells(name) >= 500
    mg, ic = M.iterations(name, "mg"), M.iterations(name, "ic0")
    print("MGRATIO %-18s cells %d: mg %d ic0 %d" % (name, M.cells(name), mg, ic))
    assert 2 * mg <= ic, (mg, ic)


def test_the_iterate_bound_is_four_times_what_fp32_costs_the_restatement(oracle):
    worst = 0.0
    for name in sorted(M.CASES):
        r64, r32 = M.reference(name), M.reference(name, fp32=True)
        for k in M.RUNGS:
            err, zero = R.worst_error(r32["p"][k], r64["p"][k], r64)
            dres = abs(r32["res"][k] - r64["res"][k]) / r64["res"][k]
            print("MGFP32 %-18s rung %d err %.3e residual %.2e" % (name, k, err, dres))
            assert zero and dres <= M.C_RESIDUAL / 2
            worst = max(worst, err)
    print("MGFP32 worst %.3e -> C_ITERATE %.2e" % (worst, 4 * worst))
    assert 0.8 * M.FP32_WORST <= worst <= 1.01 * M.FP32_WORST, (worst, M.FP32_WORST)
    assert 4 * M.FP32_WORST <= M.C_ITERATE <= 4.1 * M.FP32_WORST


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_far_outside_the_iterate_bound(oracle, mutant):
    for name in sorted(M.CASES):
        ref = M.reference(name)
        bad = M.reference(name, mutate=mutant)
        err = R.worst_error(bad["p"][0], ref["p"][0], ref)[0]
        print("MGMUT %-18s %-26s |p - p_mutant| / max|p| = %.2e" % (name, mutant, err))
        assert err > 100 * M.C_ITERATE, (name, mutant, err)


# ---- the cases whose coarse levels run one launch per operation (WIDE_CASES) ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.WIDE_SHAPES))
def test_the_wide_cases_reach_the_schedules_they_are_named_for(oracle, name):
    """the conditions that make WIDE_CASES the right inputs: the level count and the first level of k_mg_coarse (the per-launch
    levels above the block's cell limit, the block's own below it); in the closed variant every component of 5 cells or more is
    closed, in the open variant at least one is open; and no component of 2 to 4 cells in either (CG would solve a closed one
    exactly before rung k: the device test's iteration count (k + 1) x components needs every solved component to run on)"""
    dims = M.WIDE_SHAPES[name]["dims"]
    is3d = dims[0] > 1
    lv = M.mg_levels(*dims, is3d)
    cells = [z * y * x for z, y, x in lv]
    fb = M.first_block_level(lv)
    assert (len(lv), fb) == M.WIDE_SHAPES[name]["levels"]
    assert all(n > M.BLOCK_CELLS for n in cells[1:fb]) and all(n <= M.BLOCK_CELLS for n in cells[fb:])
    for variant, want_open in ((name, False), (name + "_open", True)):
        assert M.WIDE_CASES[variant]["dims"] == dims and bool(M.WIDE_CASES[variant].get("open")) == want_open
        f, div, _ = M.case(variant)
        assert f.shape[0] == 1 and f.size <= 69000
        comp, sizes = R.label_components(f[0, 0], is3d)
        assert not any(2 <= n < 5 for n in sizes), sizes
        closed = [M.MgComponent(f[0, 0], comp, c, is3d).closed for c, n in enumerate(sizes) if n >= 5]
        print("MGWIDE %-28s levels %s first block level %d, components %s, closed %s" % (variant, cells, fb, sizes.tolist(), closed))
        assert closed and (not all(closed) if want_open else all(closed)), (variant, closed)
    # the thin shapes: no level for k_mg_coarse; the wide3 shapes: two levels below level 0 as launches
    if name.startswith("thin"):
        assert fb == len(lv) == 2
    if name.startswith("wide3"):                  # 259 x 263 -> 130 x 132 -> 65 x 66: children outside the grid on levels 0 and 2
        assert fb == 3 and (lv[0][1] % 2 == 1 and lv[0][2] % 2 == 1) == ("odd" in name)
    if name.startswith("one_level"):
        assert len(lv) == 1


def test_the_wide_bounds_are_four_times_what_fp32_costs_the_restatement(oracle):
    """per rung: the iterate bound of WIDE_CASES is 4 x the worst fp32-against-fp64 ratio over WIDE_CASES, rounded up to two digits;
    the residual bound is C_RESIDUAL where the fp32 restatement stays under half of it on every case, else 4 x its worst figure"""
    worst = {k: 0.0 for k in M.RUNGS}
    worst_res = {k: 0.0 for k in M.RUNGS}
    for name in sorted(M.WIDE_CASES):
        r64, r32 = M.reference(name), M.reference(name, fp32=True)
        for k in M.RUNGS:
            err, zero = R.worst_error(r32["p"][k], r64["p"][k], r64)
            dres = abs(r32["res"][k] - r64["res"][k]) / r64["res"][k]
            print("MGFP32W %-28s rung %d err %.3e residual %.3e" % (name, k, err, dres))
            assert zero
            worst[k], worst_res[k] = max(worst[k], err), max(worst_res[k], dres)
    for k in M.RUNGS:
        print("MGFP32W rung %d worst %.3e -> %.2e, residual %.3e" % (k, worst[k], 4 * worst[k], worst_res[k]))
        assert 0.8 * M.FP32_WORST_WIDE[k] <= worst[k] <= 1.01 * M.FP32_WORST_WIDE[k], (k, worst[k])
        assert M.C_ITERATE_WIDE[k] == M.four_times_rounded_up(M.FP32_WORST_WIDE[k]), k
        assert 0.8 * M.FP32_RES_WIDE[k] <= worst_res[k] <= 1.01 * M.FP32_RES_WIDE[k], (k, worst_res[k])
        if M.FP32_RES_WIDE[k] <= M.C_RESIDUAL / 2:
            assert M.C_RESIDUAL_WIDE[k] == M.C_RESIDUAL and worst_res[k] <= M.C_RESIDUAL / 2, k
        else:
            assert M.C_RESIDUAL_WIDE[k] == M.four_times_rounded_up(M.FP32_RES_WIDE[k]), k
    # the rule is C_ITERATE's own
    assert M.four_times_rounded_up(M.FP32_WORST) == M.C_ITERATE


@pytest.mark.parametrize("mutant", M.LEVEL_MUTANTS)
def test_every_level_local_mutant_is_far_outside_the_first_rungs_bound(oracle, mutant):
    """an error that lives on ONE coarse level (a sweep short on the coarsest level or after the prolongation into level 1 or 2,
    the prolongation into level 1 unweighted) moves some cell of level 0 at rung 0 by more than 100 bounds, on every case that
    has the level; on a case that does not have it the mutant is the identity"""
    seen = 0
    for name in sorted(M.WIDE_CASES):
        dims = M.WIDE_CASES[name]["dims"]
        count = len(M.mg_levels(*dims, dims[0] > 1))
        ref = M.reference(name)
        if not M.mutant_applies(mutant, count):
            if count > 1:                                     # (the identity, shown once per mutant on the cheapest such case)
                continue
            bad = M.reference(name, mutate=mutant)
            assert np.array_equal(bad["p"][0], ref["p"][0]), (name, mutant)
            continue
        bad = M.reference(name, mutate=mutant)
        err = R.worst_error(bad["p"][0], ref["p"][0], ref)[0]
        print("MGMUTW %-28s %-26s |p - p_mutant| / max|p| = %.2e (%.0f bounds)" % (name, mutant, err, err / M.C_ITERATE_WIDE[0]))
        assert err > 100 * M.C_ITERATE_WIDE[0], (name, mutant, err)
        seen += 1
    assert seen == (8 if mutant != "coarsest_one_sweep_short" else len(M.WIDE_CASES))


def test_the_constants_mirror_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluidnet_amd", "csrc", "tfl_pcg_mg.hpp")).read()
    val = lambda n: float(re.search(r"constexpr \w+ %s = ([0-9.]+)f?;" % n, src).group(1))
    assert (val("kMgOmega"), val("kMgNu"), val("kMgNuCoarse"), val("kMgAlpha")) == (M.OMEGA, M.NU, M.NU_C, M.ALPHA)
    assert (val("kMgCoarsestExtent"), val("kMgMaxLevels"), val("kMgBlockCells")) == (M.COARSEST, M.MAX_LEVELS, M.BLOCK_CELLS)
