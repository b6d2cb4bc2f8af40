"""Scratch memory is undefined on entry, and nothing outside it is written: every entry of tests/scratch_cases.py on every case,
held by tests/scratch_history.check_row to

  history independence  the same bits after NaN, after 1e30, after the same entry on another scene, after the same entry on a
                        larger grid and after the operators of a training step as after zeros (the clean run, done twice: the
                        control);
  containment           guards of 4096 floats before and behind a scratch of exactly the size the entry asked for come back
                        word for word;
  alignment             8-byte entries give the same bits at 8 mod 16; 16-byte entries refuse such a pointer, and every entry
                        refuses a scratch one float short, with outputs, scratch and guards unchanged.

Equality is bit equality: the entries are deterministic. These tests do not replace parity -- every case is one an existing
test already holds to the oracle or to an fp64 bound (tests/test_scratch_history_cpu.py checks that), so "equal to the clean
run" means "equal to a checked result". What each entry clears and what it leaves to tags: profiles/scratch_history.md."""
import json
import os
import subprocess
import sys
import time

import pytest

import flavours
import scratch_cases as C
import scratch_history as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def not_trivial(clean):
    """the clean run must have computed something: every float array finite, at least one of them not all zero (equal bits of
    two runs that both gave NaN, or both nothing, would hold nothing)"""
    import numpy as np
    arrays = {k: v for k, v in clean.items() if isinstance(v, np.ndarray) and v.dtype.kind == "f"}
    # (-inf is a legal residual: "nothing to solve")
    out = ["the clean run's %s holds NaN or Inf" % k for k, v in arrays.items() if not np.isfinite(v[v != -np.inf]).all()]
    if not any(v.any() for v in arrays.values()):
        out.append("the clean run computed nothing but zeros")
    return out


def run_row(row):
    log, clean = [], {}
    t0 = time.perf_counter()
    fails = H.check_row(row.target(), H.TorchBackend(C.DEV), log, clean)
    fails += not_trivial(clean)
    print("scratch history %s: %.2f s, %d runs%s" % (row.id, time.perf_counter() - t0, len(log), "" if not fails else ", FAILED"))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("row", C.ROWS, ids=[r.id for r in C.ROWS])
def test_results_do_not_depend_on_what_the_scratch_held(row):
    if row.child is None or all(os.environ.get(k) == v for k, v in row.child.items()):
        fails = run_row(row)
    else:       # a switch the library reads once per process: the row in a child process of its own
        env = flavours.child_env(os.environ, row.child)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), row.id], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "SCRATCH_ROW " in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        fails = json.loads(out.stdout.split("SCRATCH_ROW ", 1)[1].splitlines()[0])
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same entries: this file in a child process against it"""
    if flavours.is_experiments_process():
        return
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("SCRATCH_ROW " + json.dumps(run_row(C.BY_ID[sys.argv[1]])))
