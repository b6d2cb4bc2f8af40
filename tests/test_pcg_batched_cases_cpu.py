"""The mixed batches of tests/pcg_batched_cases.py against the conditions that keep them from hiding a failure of the batched
PCG solve, checked with the fp64 restatement (tests/pcg_mg_ref64.py) on the CPU: the items' component counts are not all equal,
closed and open items are both present, a component of one cell and one of fewer than five are present, and at least two items
differ by two or more in the iterations 'mg' takes to 1e-5 (in fp64, seed 11 for all four kinds: 11 / 21 / 20 / 12 at (1, 24, 28)
and 10 / 18 / 18 / 10 at (9, 11, 13))."""
import numpy as np
import pytest

import pcg_batched_cases as C
import pcg_mg_ref64 as M
import pcg_ref64 as R


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_a_mixed_batch_meets_its_conditions(oracle, name):
    f, U0, div, is3d = C.batch(name)
    assert f.shape[0] == len(C.KINDS) == 4 and f.shape[2:] == C.BATCHES[name] and is3d == (C.BATCHES[name][0] > 1)
    assert not (f[:, :, :, 0, :] == 1.0).any() and not (f[:, :, :, :, 0] == 1.0).any()      # no fluid on the border
    sizes = C.component_sizes(f, is3d)
    counts = [len(s) for s in sizes]
    closed = []
    for b in range(f.shape[0]):
        comp, sz = R.label_components(f[b, 0], is3d)
        big = int(np.argmax(sz))
        closed.append(M.MgComponent(f[b, 0], comp, big, is3d).closed)
    its = [M.iterations_to(f[b:b + 1], div[b:b + 1], is3d, "mg", 1e-5) for b in range(f.shape[0])]
    print("BATCHCASE %s: components %s, largest closed %s, mg iterations to 1e-5 %s" % (name, sizes, closed, its))
    assert len(set(counts)) > 1, counts
    assert any(closed) and not all(closed), closed
    flat = [n for s in sizes for n in s]
    assert 1 in flat and any(1 < n < 5 for n in flat) and max(flat) >= 5
    assert max(its) - min(its) >= 2, its
    assert np.isfinite(div).all() and all(np.abs(div[b]).max() > 0 for b in range(f.shape[0]))


def test_the_kinds_are_what_they_say(oracle):
    """box and open: one large component; split: two large ones and a single cell; pockets: components of 2, 3 and 4 cells and a
    single cell beside the large one (the scene's random obstacles may wall off further single cells in any kind)"""
    for name in sorted(C.BATCHES):
        f, _, _, is3d = C.batch(name)
        s = {k: sorted(int(n) for n in v) for k, v in zip(C.KINDS, C.component_sizes(f, is3d))}
        large = {k: [n for n in v if n >= 5] for k, v in s.items()}
        assert len(large["box"]) == 1 and len(large["open"]) == 1 and len(large["pockets"]) == 1
        assert len(large["split"]) == 2 and 1 in s["split"]
        assert all(n in s["pockets"] for n in (1, 2, 3, 4))


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_the_bounds_of_the_sequential_solver_hold_for_these_inputs(oracle, name):
    """C_ITERATE is 4 x the worst fp32-against-fp64 error of the restatement on pcg_mg_ref64.CASES, C_RESIDUAL twice the condition
    on the reference: the GPU test takes both over for the mixed batches, so the batches must lie inside what they were derived
    from -- the fp32 restatement within FP32_WORST per cell and within C_RESIDUAL / 2 on the solve's residual, at every rung"""
    f, _, div, is3d = C.batch(name)
    r64 = M.solve(f, div, is3d, "mg", M.DEPTH)
    r32 = M.solve(f, div, is3d, "mg", M.DEPTH, dtype=np.float32)
    for k in M.RUNGS:
        err, zero = R.worst_error(r32["p"][k], r64["p"][k], r64)
        dres = abs(r32["res"][k] - r64["res"][k]) / r64["res"][k]
        print("BATCHFP32 %s rung %d err %.3e residual %.2e" % (name, k, err, dres))
        assert zero and err <= M.FP32_WORST and dres <= M.C_RESIDUAL / 2, (name, k, err, dres)
