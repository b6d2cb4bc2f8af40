"""solveLinearSystemPCG (fluidnet_amd/csrc/pcg.hip) held to the fp64 restatement of tests/pcg_ref64.py iterate by iterate. CG
converges with any symmetric positive-definite preconditioner, so a wrong IC(0) / ILU(0) diagonal, a coupling dropped at a
seam of the wavefront sweeps or a stale hand-off pair only costs iterations, and a converged pressure cannot show it; with a
tolerance that never fires, maxIter = k returns iterate k + 1 and its residual, and maxIter = 0 returns alpha_0 M^-1 b.

Every schedule runs the whole ladder in one child process (tests/pcg_iterates_run.py: the library reads its switches once):
  default      pipelined wavefronts on 3-D grids (16 iterations queued per host sync), hyperplane sweeps on 2-D (4), none (32)
  hyperplanes  TFL_PCG_HYPERPLANES=1: one launch per hyperplane on 3-D grids too
  chunks       TFL_WF_MAX_BLOCKS=4 (EXPERIMENTS flavour): at most 4 sub-boxes per launch, which is one slab per launch on the
               3 strips of inner_19x131x8 (seams_11x67x6, 2 x 2 sub-boxes, still runs in one launch)
A wavefront sweep whose sub-box never sees its predecessor makes the library repeat the solve, and the next 16 and more, with
hyperplane sweeps and say so on stderr; a "default" or "chunks" child that printed that line has not tested the wavefronts and
fails.
Bounds, per case, preconditioner and rung: |p - p64| <= 4e-6 max|p64| in every cell, max|p64| per component, and the returned
residual within 2e-5 relative of the restatement's: twice what tests/test_pcg_ref64_cpu.py holds the fp32 oracle to (the
kernels do the oracle's roundings per cell plus one reciprocal, and form their dot products in fp64). A sweep that is wrong
moves the first iterate by 1e-3 or more (tests/test_pcg_ref64_cpu.py, profiles/pcg_iterates.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import flavours
import pcg_ref64 as R
from pcg_iterates_run import BATCH_CASE, VERBOSE_RUNG

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu

SCHEDULES = {"default": {}, "hyperplanes": {"TFL_PCG_HYPERPLANES": "1"}, "chunks": {"TFL_WF_MAX_BLOCKS": "4"}}
WF_FALLBACK = "triangular sweep timed out"      # abi.cpp, tfl_solveLinearSystemPCG: the repeat with hyperplane sweeps
_runs, _failed = {}, []


def run(schedule, tmp_path_factory):
    """the arrays of one schedule's child process; after a child has failed no further one is started"""
    if schedule not in _runs:
        assert not _failed, "the child process of schedule %r failed: no further one is started" % _failed[0]
        env = dict(os.environ)
        for k in ("TFL_PCG_HYPERPLANES", "TFL_WF_MAX_BLOCKS", "TFL_WF_TEST_TIMEOUT"):
            env.pop(k, None)
        env = flavours.child_env(env, SCHEDULES[schedule])
        path = str(tmp_path_factory.mktemp("pcg_iterates") / (schedule + ".npz"))
        try:
            out = subprocess.run([sys.executable, os.path.join(HERE, "pcg_iterates_run.py"), schedule, path], env=env,
                                 capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "iterates ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
            if schedule != "hyperplanes":
                assert WF_FALLBACK not in out.stderr, "the wavefront sweeps fell back to hyperplane sweeps: " + out.stderr[-2000:]
        except BaseException:
            _failed.append(schedule)
            raise
        with np.load(path) as z:
            _runs[schedule] = {k: z[k] for k in z.files}
        _runs[schedule]["stderr"] = out.stderr
    return _runs[schedule]


def cases_of(schedule):
    return R.CHUNK_CASES if schedule == "chunks" else tuple(sorted(R.CASES))


def check(tag, p, res, p64, res64, ref, p_oracle=None):
    """the bounds of the module's docstring on one result; prints the figures first"""
    assert np.isfinite(p).all(), tag
    err, zero = R.worst_error(p, p64, ref)
    dres = abs(float(res) - res64) / res64
    line = "PCGIT %-44s err_hip %.2e residual %.2e" % (tag, err, dres)
    if p_oracle is not None:
        eo = R.worst_error(p_oracle, p64, ref)[0]
        line += " err_oracle %.2e ratio %.2f" % (eo, err / eo)
    print(line)
    assert zero, (tag, "a cell outside the solved components is not 0")
    assert err <= R.CAP_P_HIP, (tag, err)
    assert dres <= R.CAP_RES_HIP, (tag, float(res), res64)
    return err


@pytest.mark.parametrize("schedule,name", [(s, n) for s in SCHEDULES for n in cases_of(s)])
def test_iterates_and_residuals(tmp_path_factory, oracle, schedule, name):
    """every rung of the ladder: the iterate in every cell (pockets of 2 - 4 cells: against the unpreconditioned iterate the
    restatement runs for them), the returned residual, exact zeros outside the solved components"""
    got = run(schedule, tmp_path_factory)
    for pc in R.PRECONDS:
        ref, lad = R.reference(name, pc), R.oracle_ladder(name, pc)
        for k in R.RUNGS:
            check("%s %s %s rung %d" % (schedule, name, pc, k), got["%s/%s/%d" % (name, pc, k)], got["%s/%s/%d/res" % (name, pc, k)],
                  ref["p"][k], ref["res"][k], ref, lad[k][0])


@pytest.mark.parametrize("name,pc,schedule,chunk", R.STOP_CASES)
def test_stop_by_tolerance_inside_a_chunk(tmp_path_factory, oracle, name, pc, schedule, chunk):
    """tolerance = the geometric mean of the restatement's ||r_k|| and ||r_{k+1}||, k inside a queued chunk, maxIter = 1000:
    iterate k + 1 and its residual come back (that the stop is well posed: tests/test_pcg_ref64_cpu.py)"""
    got = run(schedule, tmp_path_factory)
    ref = R.reference(name, pc, R.STOP_DEPTH)
    hist = next(iter(ref["res_comp"].values()))
    k, tol = R.pick_stop(hist, chunk)
    key = "stop/%s/%s" % (name, pc)
    assert float(got[key + "/tol"]) == tol and k % chunk != 0 and (k + 1) % chunk != 0
    check("%s stop %s %s k %d" % (schedule, name, pc, k), got[key], got[key + "/res"], ref["p"][k], ref["res"][k], ref)
    for other in (k - 1, k + 1):       # one iteration fewer or more is far outside the bound
        assert R.worst_error(got[key], ref["p"][other], ref)[0] > 10 * R.CAP_P_HIP, (key, other)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_chunk_length_does_not_change_bits(tmp_path_factory, schedule):
    """verbose=True syncs after every iteration, verbose=False after 16 / 4 / 32 queued ones: the same bits"""
    got = run(schedule, tmp_path_factory)
    for name in cases_of(schedule):
        for pc in R.PRECONDS:
            a, b = got["%s/%s/verbose" % (name, pc)], got["%s/%s/%d" % (name, pc, VERBOSE_RUNG)]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (schedule, name, pc, int((a != b).sum()), got["stderr"][-500:])


@pytest.mark.parametrize("schedule", ["default", "hyperplanes"])
def test_batch_item_solved_alone_gives_the_same_bits(tmp_path_factory, schedule):
    got = run(schedule, tmp_path_factory)
    for pc in R.PRECONDS:
        for k in R.RUNGS:
            a, b = got["item1/%s/%d" % (pc, k)], got["%s/%s/%d" % (BATCH_CASE, pc, k)][1:2]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (schedule, pc, k, int((a != b).sum()), got["stderr"][-500:])


def test_wavefronts_against_hyperplanes(tmp_path_factory):
    """recorded, not bit-equal: the wavefront sweeps multiply by reciprocals where the hyperplane sweeps divide. Both are
    within 4e-6 of the restatement, so within 8e-6 of each other; 2-D grids and `none` run the same kernels in both."""
    wf, hp = run("default", tmp_path_factory), run("hyperplanes", tmp_path_factory)
    for name in sorted(R.CASES):
        f, div, is3d = R.case(name)
        for pc in R.PRECONDS:
            ref = R.reference(name, pc)
            worst = max(R.worst_error(wf["%s/%s/%d" % (name, pc, k)], hp["%s/%s/%d" % (name, pc, k)].astype(np.float64), ref)[0]
                        for k in R.RUNGS)
            print("PCGWH %-20s %-5s wavefronts - hyperplanes %.2e" % (name, pc, worst))
            assert worst <= 2 * R.CAP_P_HIP, (name, pc, worst)
            if not is3d or pc == "none":
                assert worst == 0.0, (name, pc, worst)


def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same kernels: this file in a child process against it"""
    if flavours.is_experiments_process():
        return
    assert not _failed, "the child process of schedule %r failed: no further one is started" % _failed[0]
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
