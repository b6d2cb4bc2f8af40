"""The fp64 restatement of the multigrid preconditioner (tests/pcg_mg_ref64.py) held to what the device test relies on, on the
CPU: the V-cycle is symmetric and positive on every component of every case (and the 'mean' mutant is not symmetric), converged
mg-PCG reaches the compiled oracle's 'ic0' solution within the bound of test_hip_parity.py's PCG test, mg takes at most half the
iterations of 'ic0', the iterate bound C_ITERATE is 4 x what fp32 costs the restatement itself, and every mutant is more than 100
bounds away at the first rung."""
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


def test_the_constants_mirror_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluidnet_amd", "csrc", "tfl_pcg_mg.hpp")).read()
    val = lambda n: float(re.search(r"constexpr \w+ %s = ([0-9.]+)f?;" % n, src).group(1))
    assert (val("kMgOmega"), val("kMgNu"), val("kMgNuCoarse"), val("kMgAlpha")) == (M.OMEGA, M.NU, M.NU_C, M.ALPHA)
    assert (val("kMgCoarsestExtent"), val("kMgMaxLevels")) == (M.COARSEST, M.MAX_LEVELS)
