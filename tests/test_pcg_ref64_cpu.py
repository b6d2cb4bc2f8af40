"""The fp64 restatement of solveLinearSystemPCG (tests/pcg_ref64.py) against the fp32 oracle, on the cases, preconditioners and
maxIter rungs that tests/test_hip_pcg_iterates.py holds the device solver to. These are conditions on the reference alone:
the oracle's iterate within 2e-6 max|p64| of the restatement in every cell and its returned residual within 1e-5 relative
(measured on these cases: at most 1.21e-6 and 4.10e-6, profiles/pcg_iterates.md); cells outside the solved components exactly 0 in both; two deliberately wrong
preconditioners more than 100 caps away at the first iterate; and the tolerance stops of the GPU test well posed."""
import numpy as np
import pytest

import pcg_ref64 as R


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_oracle_is_within_the_caps_of_the_restatement(oracle, name):
    f, div, is3d = R.case(name)
    for pc in R.PRECONDS:
        ref = R.reference(name, pc)
        lad = R.oracle_ladder(name, pc)
        worst_p = worst_r = 0.0
        for k in R.RUNGS:
            p, res = lad[k]
            p64, res64 = ref["p"][k], ref["res"][k]
            err, zero = R.worst_error(p, p64, ref)
            assert zero and np.all(p64[~R.solved_mask(ref)] == 0.0), (name, pc, k)
            dres = abs(res - res64) / res64
            worst_p, worst_r = max(worst_p, err), max(worst_r, dres)
            assert err <= R.CAP_P_ORACLE, (name, pc, k, err)
            assert dres <= R.CAP_RES_ORACLE, (name, pc, k, res, res64)
        print("%-20s %-5s oracle: worst |p - p64| / max|p64| = %.2e, residual %.2e" % (name, pc, worst_p, worst_r))


def test_the_cases_reach_what_they_are_meant_to(oracle):
    """component sizes: the pockets of 2, 3, 4 cells and a size-1 component beside a large one; two large components and a
    size-1 pocket in the split cases; a different number of components in the two items of the batch case"""
    for name in ("pockets_9x14x12", "pockets_flat_20x22"):
        sizes = sorted(R.reference(name, "none")["sizes"][0])
        assert sizes[:4] == [1, 2, 3, 4] and sizes[-1] > 100, (name, sizes)
    for name in ("seams_11x67x6", "inner_19x131x8", "flat_70x9"):
        sizes = sorted(R.reference(name, "none")["sizes"][0])
        assert sizes[0] == 1 and sizes[-2] >= 50, (name, sizes)
    ref = R.reference("seams_11x67x6", "none")
    for c, size in enumerate(ref["sizes"][0]):       # each large component crosses the strip seam (row 64 | 65) and the slab seam (plane 8 | 9)
        if size >= 50:
            kk, jj, ii = np.nonzero(ref["comp"][0] == c)
            assert jj.min() <= 64 < jj.max() and kk.min() <= 8 < kk.max(), (c, size)
    f, div, is3d = R.case("seams_11x67x6")
    assert (f == 4.0).any()
    sizes = R.reference("batch_12x20x24", "none")["sizes"]
    assert len(sizes) == 2 and sum(s >= 50 for s in sizes[0]) == 1 and sum(s >= 50 for s in sizes[1]) == 2, sizes
    f, div, is3d = R.case("batch_12x20x24")
    assert not np.array_equal(f[0], f[1])


def test_labelling_is_the_oracles(oracle):
    import ctypes
    for name in sorted(R.CASES):
        f, div, is3d = R.case(name)
        B, _, Z, Y, X = f.shape
        comp = np.zeros((B, Z, Y, X), np.int32)
        ncomp = np.zeros(B, np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        oracle.lib.ora_findConnectedFluidComponents(vp(np.ascontiguousarray(f)), int(is3d), B, Z, Y, X, vp(comp), vp(ncomp))
        assert np.array_equal(comp, R.reference(name, "none")["comp"]), name


@pytest.mark.parametrize("mutant,names", [("slab_seam", ("seams_11x67x6", "inner_19x131x8", "batch_12x20x24")),
                                          ("strip_d", ("seams_11x67x6", "inner_19x131x8"))])
def test_a_wrong_preconditioner_is_far_outside_the_bound(oracle, mutant, names):
    """the z-coupling dropped where the lower neighbour lies across a slab seam (k - 1 a multiple of 8); d of the first strip
    of 64 rows scaled by 1 + 2^-10: at the first iterate each is more than 100 caps from the oracle"""
    for name in names:
        f, div, is3d = R.case(name)
        for pc in ("ilu0", "ic0"):
            ref = R.reference(name, pc)
            bad = R.solve64(f, div, is3d, pc, 1, mutate=mutant)
            err, _ = R.worst_error(R.oracle_ladder(name, pc)[0][0], bad["p"][0], ref)
            print("%-20s %-5s %-9s |p_oracle - p_mutant| / max|p| = %.2e" % (name, pc, mutant, err))
            assert err > 100 * R.CAP_P_ORACLE, (name, pc, mutant, err)


@pytest.mark.parametrize("name,pc,schedule,chunk", R.STOP_CASES)
def test_tolerance_stops_are_well_posed(oracle, name, pc, schedule, chunk):
    """one solved component; ||r_k|| >= 1.5 ||r_{k+1}|| and no earlier residual within sqrt(1.5) of the tolerance; the oracle, given the geometric mean of ||r_k|| and
    ||r_{k+1}|| as its tolerance, stops at iterate k + 1"""
    f, div, is3d = R.case(name)
    ref = R.reference(name, pc, R.STOP_DEPTH)
    assert len(ref["res_comp"]) == 1
    hist = next(iter(ref["res_comp"].values()))
    k, tol = R.pick_stop(hist, chunk)
    assert k % chunk != 0 and hist[k] / hist[k + 1] >= 1.5 and hist[k + 1] < tol < hist[:k + 1].min()
    p = np.zeros_like(div)
    res = oracle.solveLinearSystemPCG(p, f, div, is3d, tol, 1000, pc)
    err, zero = R.worst_error(p, ref["p"][k], ref)
    print("%-20s %-5s stop at k = %d, tol %.3e: oracle %.2e, residual %.2e" % (name, pc, k, tol, err, abs(res - ref["res"][k]) / ref["res"][k]))
    assert zero and err <= R.CAP_P_ORACLE and abs(res - ref["res"][k]) <= R.CAP_RES_ORACLE * ref["res"][k], (k, err, res, ref["res"][k])
    # and it is that iterate, not a neighbour: the iterates before and after are far outside the cap
    for other in (k - 1, k + 1):
        assert R.worst_error(p, ref["p"][other], ref)[0] > 10 * R.CAP_P_ORACLE, other
