"""Helper of tests/test_hip_pcg_iterates.py: own process, because the library reads TFL_PCG_HYPERPLANES and TFL_WF_MAX_BLOCKS
(and is chosen itself, TFL_LIBRARY) once per process.
`<schedule> <out.npz>`, schedule = default | hyperplanes | chunks: every case of tests/pcg_ref64.py that the schedule runs x
preconditioner x maxIter rung with a tolerance that never fires -> "case/pc/rung" (the returned p) and "case/pc/rung/res" (the
returned residual); rung 5 again with verbose=True (one iteration per host sync) -> "case/pc/verbose"; item 1 of the batch
case solved alone -> "item1/pc/rung"; the tolerance stops of this schedule -> "stop/case/pc" (+ "/res", "/tol")."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

VERBOSE_RUNG = 5
BATCH_CASE = "batch_12x20x24"


def main(schedule, path):
    import numpy as np
    import pcg_ref64 as R
    from flavours import is_experiments_process
    from hip_adapter import HipTfluids
    assert (os.environ.get("TFL_PCG_HYPERPLANES") is not None) == (schedule == "hyperplanes"), schedule
    assert (os.environ.get("TFL_WF_MAX_BLOCKS") == "4") == (schedule == "chunks"), schedule
    assert schedule != "chunks" or is_experiments_process(), "TFL_WF_MAX_BLOCKS is read by the EXPERIMENTS flavour only"
    hip = HipTfluids()
    out = {}

    def solve(f, div, is3d, tol, max_iter, pc, verbose=False):
        p = np.random.RandomState(2).rand(*div.shape).astype(np.float32)     # the solver overwrites every cell
        res = hip.solveLinearSystemPCG(p, np.array(f), np.array(div), is3d, tol, max_iter, pc, verbose)
        return p, np.float64(res)

    names = R.CHUNK_CASES if schedule == "chunks" else sorted(R.CASES)
    for name in names:
        f, div, is3d = R.case(name)
        for pc in R.PRECONDS:
            for k in R.RUNGS:
                out["%s/%s/%d" % (name, pc, k)], out["%s/%s/%d/res" % (name, pc, k)] = solve(f, div, is3d, R.TOL_NEVER, k, pc)
            out["%s/%s/verbose" % (name, pc)], _ = solve(f, div, is3d, R.TOL_NEVER, VERBOSE_RUNG, pc, verbose=True)
            if name == BATCH_CASE:
                for k in R.RUNGS:
                    out["item1/%s/%d" % (pc, k)], _ = solve(f[1:2], div[1:2], is3d, R.TOL_NEVER, k, pc)
    for name, pc, sched, chunk in R.STOP_CASES:
        if sched != schedule:
            continue
        f, div, is3d = R.case(name)
        hist = next(iter(R.reference(name, pc, R.STOP_DEPTH)["res_comp"].values()))
        k, tol = R.pick_stop(hist, chunk)
        key = "stop/%s/%s" % (name, pc)
        out[key], out[key + "/res"] = solve(f, div, is3d, tol, 1000, pc)
        out[key + "/tol"] = np.float64(tol)
    sys.stdout.flush()
    np.savez(path, **out)
    print("\niterates ok: %s, %d arrays" % (schedule, len(out)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
