"""Times solveLinearSystemPCG with each preconditioner -- none / ilu0 / ic0 / mg -- on the system a step of the data-set generator
solves (tools/datagen_bench.py's scene: plan 0 of the default configuration, 8 steps, then the divergence of an outputDiv step's
velocity) and on the same scene with an open face (the top row of cells empty: a regular system), at 2-D 128^2 and 256^2 and
3-D 64^3 and 128^3, and writes a table (profiles/pcg_mg.md keeps it).
Per grid, scene and preconditioner: the iterations to tol 1e-4 (tfluids.pcgLastIterations; maxIter 1000), the wall-clock ms of
one solve (the call synchronises; median of five after one warm call, min .. max beside it) and the ms of a solve whose tolerance
is met at once ("no iteration": component labelling, the factorisation or the hierarchy, the first queued chunk of iterations
falling through, the write-back; 'none' shows what of it is not the preconditioner's). The launch columns are NOT measured: they
are the launch sequence of the host code (pcg.hip Solve::iteration / precondition, pcg_mg.hip vcycle) worked out for the grid, with
the shape constants read from tfl_pcg_mg.hpp and tfl_pcg_ws.hpp: per iteration 5 launches of CG itself (4 without a
preconditioner), per chunk one more, per component solve 2 (set-up) + 3 (write-back), for a single closed component.
--batched B[,B...] measures solveLinearSystemPCGBatched instead (profiles/pcg_batched.md keeps that table): the closed scene of
the generator's plans 0 .. B - 1 as one batch; per repetition, in turn, the batched 'mg' solve, one call of solveLinearSystemPCG
with 'mg' and one with 'ic0' on the same batch (that entry solves the items one after the other), each synchronised; then, at
the largest B, one calcPUTargets call (trainTargetSource = 'pcg', tol 1e-4, maxIter 100) with and without mconf.pcgBatched.
usage: python tools/pcg_bench.py [--out FILE.md] [--grids 2d128,2d256,3d64,3d128] [--batched 1,4,16]"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fluidnet_amd import datagen, tfluids  # noqa: E402
from fluidnet_amd.simulate import simulate  # noqa: E402

DEV = torch.device("cuda:0")
SEED, TOL, MAX_ITER, REPS = 11, 1e-4, 1000, 5
GRIDS = {"2d128": (False, (1, 128, 128)), "2d256": (False, (1, 256, 256)), "3d64": (True, (64, 64, 64)), "3d128": (True, (128, 128, 128))}


def _constant(header, name):
    src = open(os.path.join(ROOT, "fluidnet_amd", "csrc", header)).read()
    m = re.search(r"\b%s = ([0-9]+)\b" % name, src) or re.search(r"#define %s ([0-9]+)" % name, src)
    return int(m.group(1))


MG_NU, MG_NU_C, MG_COARSEST, MG_MAX_LEVELS, MG_BLOCK_CELLS = (_constant("tfl_pcg_mg.hpp", n) for n in (
    "kMgNu", "kMgNuCoarse", "kMgCoarsestExtent", "kMgMaxLevels", "kMgBlockCells"))
WF_ROWS, WF_PLANES, WF_MAX_BLOCKS = (_constant("tfl_pcg_ws.hpp", n) for n in ("kWfRows", "TFL_WF_PLANES", "kWfMaxBlocks"))


def mg_launches(dims, is3D):
    """(per application, set-up) of pcg_mg.hip for a grid"""
    lv = [dims]
    while len(lv) < MG_MAX_LEVELS:
        z, y, x = lv[-1]
        if x <= MG_COARSEST or y <= MG_COARSEST or (is3D and z <= MG_COARSEST):
            break
        lv.append(((z + 1) // 2 if is3D else z, (y + 1) // 2, (x + 1) // 2))
    cells = [z * y * x for z, y, x in lv]
    fb = len(lv)
    for l in range(len(lv) - 1, 0, -1):
        if cells[l] > MG_BLOCK_CELLS:
            break
        fb = l
    wide, last = min(fb, len(lv)), len(lv) - 1
    n = 1                                                       # the sum of r
    for l in range(wide):
        n += (1 if l > 0 else 0) + (MG_NU_C if l == last else MG_NU)
    n += 1 if fb < len(lv) else 0                               # k_mg_coarse
    n += MG_NU * min(wide, last)
    return n, len(lv), dict(levels=len(lv), first_block_level=fb, level_cells=cells)


def sweep_launches(dims, is3D):
    """(per application, set-up) of the IC(0) / ILU(0) sweeps"""
    Z, Y, X = dims
    planes = (X - 2) + (Y - 2) + (Z - 2 if is3D else 0) - (2 if is3D else 1)
    if not is3D:
        return 2 * planes, planes
    ns, nb = -(-(Y - 2) // WF_ROWS), -(-(Z - 2) // WF_PLANES)
    if ns * nb <= WF_MAX_BLOCKS:
        return 4, planes + 1
    return 2 + 2 * -(-nb // max(1, WF_MAX_BLOCKS // ns)), planes + 1


def scene(is3D, dims, open_face, run=0, with_velocity=False):
    g = datagen.default_gconf(is3D, dims)
    plan = datagen.plan_run(g, SEED, run)
    mconf = datagen.mconf_of(plan)
    batch = datagen.init_state(plan, DEV)
    for _ in range(8):
        simulate(None, mconf, batch, None)
    simulate(None, mconf, batch, None, outputDiv=True)      # advection and forces only: the velocity the step's solve projects
    flags = batch["flags"].clone()
    if open_face:
        Y = dims[1]
        top = flags[:, :, 1:-1, Y - 2, 1:-1] if is3D else flags[:, :, :, Y - 2, 1:-1]
        top[top == 1.0] = 4.0
    U = batch["UDiv"].clone()
    tfluids.setWallBcsForward(U, flags)
    div = torch.empty_like(batch["pDiv"])
    tfluids.velocityDivergenceForward(U, flags, div)
    if with_velocity:
        return flags, div, batch["UDiv"].clone()
    return flags, div


def solve_ms(p, flags, div, is3D, tol, pc):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = tfluids.solveLinearSystemPCG(p, flags, div, is3D, tol, MAX_ITER, pc)
    return (time.perf_counter() - t0) * 1e3, r


def measure(key):
    is3D, dims = GRIDS[key]
    rows = []
    for open_face in (False, True):
        flags, div = scene(is3D, dims, open_face)
        p = torch.zeros_like(div)
        for pc in ("none", "ilu0", "ic0", "mg"):
            solve_ms(p, flags, div, is3D, TOL, pc)
            ts, res = [], 0.0
            for _ in range(REPS):
                t, res = solve_ms(p, flags, div, is3D, TOL, pc)
                ts.append(t)
            its = tfluids.pcgLastIterations(p)
            setup = float(np.median([solve_ms(p, flags, div, is3D, 1e30, pc)[0] for _ in range(REPS)]))
            per_app, setup_launches, extra = (0, 0, {}) if pc == "none" else (mg_launches(dims, is3D) if pc == "mg" else sweep_launches(dims, is3D) + ({},))
            chunk = 32 if pc == "none" else (8 if pc == "mg" else (16 if is3D and per_app == 4 else 4))
            per_solve = 2 + 3 + setup_launches + its * (per_app + (5 if pc != "none" else 4)) + -(-its // chunk)
            rows.append(dict(grid=key, scene="open face" if open_face else "closed", precond=pc, iterations=its, residual=res,
                             ms=float(np.median(ts)), ms_min=min(ts), ms_max=max(ts), setup_ms=setup, launches_per_application=per_app,
                             launches_per_solve=per_solve, rhs_norm=float(div.norm()), **extra))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure_batched(key, sizes):
    """rows of the batched table for one grid: per B the three solves in turn, REPS times after a warm round; then calcPUTargets"""
    from fluidnet_amd.simulate import calcPUTargets
    is3D, dims = GRIDS[key]
    items = [scene(is3D, dims, False, run=b, with_velocity=True) for b in range(max(sizes))]
    rows = []
    for B in sizes:
        flags, div = (torch.cat([it[i] for it in items[:B]]).contiguous() for i in (0, 1))
        pb, pm, pi = (torch.zeros_like(div) for _ in range(3))
        forms = (("batched mg", lambda: tfluids.solveLinearSystemPCGBatched(pb, flags, div, is3D, TOL, MAX_ITER, "mg")[1].sum()),
                 ("sequential mg", lambda: (tfluids.solveLinearSystemPCG(pm, flags, div, is3D, TOL, MAX_ITER, "mg"), tfluids.pcgLastIterations(pm))[1]),
                 ("sequential ic0", lambda: (tfluids.solveLinearSystemPCG(pi, flags, div, is3D, TOL, MAX_ITER, "ic0"), tfluids.pcgLastIterations(pi))[1]))
        ts, its = {n: [] for n, _ in forms}, {}
        for rep in range(REPS + 1):                       # the first round warms every form up
            for n, fn in forms:
                t, its[n] = _timed(fn)
                if rep:
                    ts[n].append(t)
        row = dict(grid=key, B=B, same_bits=bool(torch.equal(pb, pm)), iterations={n: int(v) for n, v in its.items()},
                   ms={n: float(np.median(v)) for n, v in ts.items()}, ms_min={n: min(v) for n, v in ts.items()},
                   ms_max={n: max(v) for n, v in ts.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    B = max(sizes)
    flags = torch.cat([it[0] for it in items[:B]]).contiguous()
    U0 = torch.cat([it[2] for it in items[:B]]).contiguous()
    base = dict(trainTargetSource="pcg", maxIter=100)
    batch = dict(flags=flags, UDiv=U0.clone(), pTarget=torch.zeros_like(flags), UTarget=torch.zeros_like(U0))
    ts = {"pcgBatched": [], "as it is": []}
    for rep in range(REPS + 1):
        for n, mconf in (("pcgBatched", dict(base, pcgBatched=True)), ("as it is", base)):
            batch["UDiv"].copy_(U0)
            t, _ = _timed(lambda: calcPUTargets(None, mconf, batch))
            if rep:
                ts[n].append(t)
    row = dict(grid=key, B=B, calcPUTargets_ms={n: float(np.median(v)) for n, v in ts.items()},
               calcPUTargets_ms_min={n: min(v) for n, v in ts.items()}, calcPUTargets_ms_max={n: max(v) for n, v in ts.items()})
    rows.append(row)
    print(json.dumps(row), flush=True)
    return rows


def batched_table(rows):
    lines = ["%s, HIP %s. tol %g, maxIter %d (calcPUTargets: maxIter 100); ms: median of %d after a warm round, the forms in turn "
             "(min .. max). Iterations: summed over the items." % (torch.cuda.get_device_name(0), torch.version.hip, TOL, MAX_ITER, REPS), "",
             "| grid | B | batched mg ms | sequential mg ms | sequential ic0 ms | sequential mg / batched | sequential ic0 / batched | iterations mg | iterations ic0 | same bits as sequential mg |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda r, n: "%.2f (%.2f .. %.2f)" % (r["ms"][n], r["ms_min"][n], r["ms_max"][n])
    for r in rows:
        if "ms" in r:
            b = r["ms"]["batched mg"]
            lines.append("| %s | %d | %s | %s | %s | %.2f | %.2f | %d | %d | %s |" % (
                r["grid"], r["B"], f(r, "batched mg"), f(r, "sequential mg"), f(r, "sequential ic0"), r["ms"]["sequential mg"] / b,
                r["ms"]["sequential ic0"] / b, r["iterations"]["batched mg"], r["iterations"]["sequential ic0"], "yes" if r["same_bits"] else "NO"))
    lines += ["", "| grid | B | calcPUTargets with pcgBatched ms | calcPUTargets as it is ('ic0') ms | ratio |", "|---|---|---|---|---|"]
    for r in rows:
        if "calcPUTargets_ms" in r:
            m, lo, hi = r["calcPUTargets_ms"], r["calcPUTargets_ms_min"], r["calcPUTargets_ms_max"]
            lines.append("| %s | %d | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.2f |" % (
                r["grid"], r["B"], m["pcgBatched"], lo["pcgBatched"], hi["pcgBatched"], m["as it is"], lo["as it is"], hi["as it is"],
                m["as it is"] / m["pcgBatched"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="2d128,2d256,3d64,3d128")
    ap.add_argument("--batched", default=None, help="batch sizes, e.g. 1,4,16: measure solveLinearSystemPCGBatched instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcg_bench needs an MI355X: nothing is measured without one")
    if a.batched:
        rows = []
        for key in a.grids.split(","):
            rows += measure_batched(key, [int(b) for b in a.batched.split(",")])
        text = batched_table(rows)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    rows = []
    for key in a.grids.split(","):
        rows += measure(key)
    lines = ["%s, HIP %s. tol %g, maxIter %d; ms: median of %d solves after a warm one (min .. max)." % (
        torch.cuda.get_device_name(0), torch.version.hip, TOL, MAX_ITER, REPS), "",
        "| grid | scene | precond | iterations | residual | ms per solve | ms with no iteration | launches per application (from the host code) | launches per solve (from the host code) |",
        "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %d | %.2e | %.2f (%.2f .. %.2f) | %.2f | %d | %d |" % (
            r["grid"], r["scene"], r["precond"], r["iterations"], r["residual"], r["ms"], r["ms_min"], r["ms_max"], r["setup_ms"],
            r["launches_per_application"], r["launches_per_solve"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
