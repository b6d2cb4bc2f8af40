#!/usr/bin/env python3
"""Bits and launches of the PCG solver's host code, for comparing two builds of the library (TFL_LIBRARY=... picks one per process).

For every case of tests/pcg_ref64.py (CASES; CHUNK_CASES when TFL_WF_MAX_BLOCKS is set, the schedule of the EXPERIMENTS flavour):
the three preconditioners at maxIter 0 and 5 with the tolerance that never fires, one converged solve at tol = 1e-4, maxIter 5
again with verbose (one iteration per host sync), item 1 of the batch case solved alone, and one normalizePressureMean. Prints,
per call, the SHA-256 of the returned array, the returned residual's bits and the per-kernel call counts from tfluids.profile.
Two builds that do the same thing print the same lines:

    TFL_LIBRARY=ab/parent.so python tools/pcg_split_check.py parent.txt
    python tools/pcg_split_check.py branch.txt && diff parent.txt branch.txt

The lines go to the file named (the library's own verbose prints stay on stdout), or to stdout without one.
"""
import hashlib
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]

import pcg_ref64 as R  # noqa: E402
from fluidnet_amd import tfluids  # noqa: E402
from fluidnet_amd._lib import TfluidsError  # noqa: E402

DEV = "cuda:0"
BATCH_CASE = "batch_12x20x24"
OUT = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def call(tag, like, fn):
    """run fn under the library's profiler; print what it returned (or the refusal) and its launches"""
    try:
        with tfluids.profile(like) as prof:
            p, res = fn()
        launches = " ".join("%s:%d" % (k, v["calls"]) for k, v in sorted(prof.kernels.items()))
        bits = "none" if res is None else struct.pack("<f", res).hex()
        print("%s p %s residual %s launches %s" % (tag, sha(p), bits, launches), file=OUT, flush=True)
    except TfluidsError as e:
        print("%s refused: %s" % (tag, e), file=OUT, flush=True)


def solves(name, flags, div, is3d):
    def solve(tag, tol, max_iter, pc, verbose=False):
        def fn():
            p = torch.full_like(div, 0.5)       # the solver overwrites every cell
            return p, tfluids.solveLinearSystemPCG(p, flags, div, is3d, tol, max_iter, pc, verbose)
        call("%s %s %s" % (name, pc, tag), flags, fn)

    for pc in R.PRECONDS:
        for k in (0, 5):
            solve("maxIter %d" % k, R.TOL_NEVER, k, pc)
        solve("tol 1e-4", 1e-4, 1000, pc)
        solve("maxIter 5 verbose", R.TOL_NEVER, 5, pc, verbose=True)


def main():
    names = R.CHUNK_CASES if os.environ.get("TFL_WF_MAX_BLOCKS") else sorted(R.CASES)
    for name in names:
        f, div, is3d = R.case(name)
        flags, div = torch.from_numpy(f.copy()).to(DEV), torch.from_numpy(div.copy()).to(DEV)
        solves(name, flags, div, is3d)
        if name == BATCH_CASE:
            solves(name + " item 1", flags[1:2].contiguous(), div[1:2].contiguous(), is3d)

        def npm():
            p = torch.from_numpy(R.np.random.RandomState(3).rand(*f.shape).astype("float32")).to(DEV)
            tfluids.normalizePressureMean(p, flags, is3d)
            return p, None
        call("%s normalizePressureMean" % name, flags, npm)
    torch.cuda.synchronize()
    print("done: %d cases" % len(names), file=OUT, flush=True)


if __name__ == "__main__":
    main()
