"""The case table of the scratch-memory contract (tests/scratch_history.py): one row per (entry, case). Every case comes from a
table an existing test already holds to the oracle or to an fp64 bound; tests/test_scratch_history_cpu.py looks every one up in
the table its row names (`sources`), and holds the table complete against include/tfluids_hip.h and the getTempStorage call
sites of fluidnet_amd/*.py. What is shared with that table is the shape and, where the table builds a scene from parameters (the
PCG, multigrid, batched, criterion, divergence-norm, gradient, step and z-slab tables, the operator tables' seed and scene
arguments), the scene itself. What a parity test does to its scene afterwards (flag words swapped in, random fields of its own,
more steps) is not repeated here, so for those rows "the same bits as the clean run" means "the same bits as a run of a case
the suite checks", not "as the very array a parity test compared".

Importing this module needs neither a GPU nor the built library: a row only describes its case; Row.target() builds the scenes
and the device tensors when tests/test_hip_scratch_history.py runs it.

Most entries draw their scratch from tfluids.getTempStorage, and those rows are seeded the same way: the pre-filled arena view
stands in tfluids._tmp[(device, scope)] for the duration of a run, with getTempStorage wrapped to record the largest total it
was asked for -- that total is the `need` the arena's interior is cut to, and a run that asked for more would allocate a buffer
of its own, which the wrapper refuses. The refusals (a scratch one float short, a 16-byte entry at 8 mod 16) go through ctypes
with the interior pointer, as scal3_sparse_run.run_stale calls the step; the same ctypes call on the whole, aligned interior
must succeed (the control of the refusals).

The projection ConvNet keeps scratch of its own (ProjectionNet._work per device, the trainer's _bwd_work) and a tape. Those rows
(ModelTarget) do NOT assign views to net._work / trainer._bwd_work: they call the C entries through ctypes on exact-length
interiors, one arena per array, so that each array has guards of its own and can be one float short alone. That holds the
library's contract; how ProjectionNet and the trainer grow and slice their buffers is not under test here. The z-slab rows
(SlabTarget) replace each virtual rank's SlabSimulation.ws, the persistent workspace the step is given, and run through
SlabSimulation's own calls.

Every row's other scene has another flag topology -- more fluid components wherever the case's table offers that (the split
scenes of scenes.pcg_problem, the reversed kinds of a mixed batch, an extra wall, a second plume's obstacles), the closed / open
twin of the same shape for the multigrid cases -- and, where the entry iterates, a tolerance ten times tighter; every row's
larger grid moves every region of the workspace to another offset."""
import ctypes
import functools
import os

import numpy as np

import scratch_history as H

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
EVERY = ("nan", "1e30", "leftover-scene", "leftover-larger", "leftover-foreign")


# ---- rows ---------------------------------------------------------------------------------------------------------------------
class Row:
    """id; entries: the header's functions the row runs; call_sites: (file, function) of the getTempStorage calls it reaches;
    sources: where the case comes from -- ("file.py", "text", literal found in that file) or ("module", "key", TABLE, key);
    make: () -> scratch_history.Target (needs the GPU); child: environment of the child process the row runs in (a switch the
    library reads once per process), None for the test's own process"""

    def __init__(self, id, entries, call_sites, sources, make, prestates=EVERY, child=None):
        self.id, self.entries, self.call_sites, self.sources = id, tuple(entries), tuple(call_sites), tuple(sources)
        self.make, self.prestates, self.child = make, tuple(prestates), child
        self.shared_tmp = bool(call_sites)      # the row runs on the shared getTempStorage buffer: the foreign leftovers apply

    def target(self):
        t = self.make()
        t.prestates = self.prestates
        return t


def in_source(src):
    if src[1] == "text":
        return src[2] in open(os.path.join(HERE, src[0])).read()
    assert src[1] == "key", src
    import importlib
    table = getattr(importlib.import_module(src[0]), src[2])
    if isinstance(table, dict):
        return src[3] in table
    return any((row[0] if isinstance(row, (tuple, list)) else row) == src[3] or row == src[3] for row in table)


# Functions of the header with a `workspace` or `tape` parameter that no row runs, each with its reason.
EXCLUDED = {
    "tfl_model_div": "returns an address inside the workspace and launches nothing: there is nothing to leave or to read",
    "tfl_slab_graph_create": "out of scope: a captured-graph step pins its own scratch scope for as long as the graph lives",
}
# Operators that take their temporaries as tensors (no `workspace` parameter): rows name them all the same.
TMP_ONLY_ENTRIES = ("tfl_advectScalar", "tfl_advectVel", "tfl_vorticityConfinement", "tfl_vorticityConfinementFrom",
                    "tfl_vorticityConfinementItems", "tfl_solveLinearSystemJacobi", "tfl_rectangularBlur")
EXCLUDED_CALL_SITES = {}


# ---- the device side ------------------------------------------------------------------------------------------------------------
def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def down(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def oracle():
    import pcg_ref64
    return pcg_ref64._oracle()


class TmpTarget(H.Target):
    """An entry that draws its scratch from tfluids.getTempStorage. runs: which -> () -> results; direct: (view) -> complaints,
    the entry called through ctypes on `view` (pointer and length) in a way that must be refused."""
    slots = ("ws",)

    def __init__(self, runs, align, direct=None, short=False, scope=None):
        self.runs, self.direct, self.scope = runs, direct, scope
        self.align = {"ws": align}
        self.short = ("ws",) if short else ()
        self._need = {}

    def _with_tmp(self, view, fn):
        """fn() with `view` (None: nothing) as the scratch buffer of the scope; returns (result, largest total asked for)"""
        import torch
        from fluidnet_amd import tfluids
        key = (torch.device(DEV).index, self.scope)
        saved_tmp, saved_get, saved_scope = tfluids._tmp.get(key), tfluids.getTempStorage, tfluids._scratch_scope
        asked = [0]

        def recording(like, sizes):
            total = sum(int(np.prod(s)) for s in sizes)
            asked[0] = max(asked[0], total)
            if view is not None:
                assert total <= view.numel(), "the entry asks for %d floats, the size recorded for this case is %d" % (total, view.numel())
            out = saved_get(like, sizes)
            assert view is None or tfluids._tmp[key] is view
            return out
        tfluids._tmp.pop(key, None)
        if view is not None:
            tfluids._tmp[key] = view
        tfluids._scratch_scope = self.scope
        tfluids.getTempStorage = recording
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            tfluids.getTempStorage, tfluids._scratch_scope = saved_get, saved_scope
            tfluids._tmp.pop(key, None)
            if saved_tmp is not None:
                tfluids._tmp[key] = saved_tmp
        return out, asked[0]

    def need(self, which):
        if which not in self._need:
            _, n = self._with_tmp(None, self.runs[which])
            assert n > 0, "the entry never asked for scratch"
            self._need[which] = n
        return {"ws": self._need[which]}

    def run(self, which, spans):
        out, n = self._with_tmp(spans["ws"].view(), self.runs[which])
        assert n == self._need[which], (which, n, self._need[which])
        return out

    def run_refused(self, spans, accepted=False):
        return self.direct(spans["ws"].view(), accepted)


def refusal(call, outputs, accepted=False, also=None):
    """complaints of a ctypes call that must come back TFL_EINVAL (-1) and leave `outputs` (name -> tensor) as they were; also:
    () -> more complaints of that kind (host-side results). accepted: the control -- the same call must succeed (0)"""
    import torch
    before = {k: v.clone() for k, v in outputs.items()}
    rc = call()
    torch.cuda.synchronize()
    if accepted:
        return [] if rc == 0 else ["the call was not accepted (returned %d)" % rc]
    out = [] if rc == -1 else ["the call was not refused with TFL_EINVAL (returned %d)" % rc]
    for k, v in outputs.items():
        if not torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, before[k].view(torch.int32) if v.dtype == torch.float32 else before[k]):
            out.append("the refused call changed %s" % k)
    return out + (also() if also else [])


def foreign(dims, B):
    """what a training step leaves in the shared scratch: one MacCormack advectScalar and one fluidCriterion at the case's shape"""
    import torch
    import scenes
    from fluidnet_amd import tfluids

    def run():
        a = scenes.make_scene(dims, seed=901, B=B, vel_cells=1.5)
        b = scenes.make_scene(dims, seed=902, B=B, vel_cells=0.4)
        s, U, fl = up(a["density"]), up(a["U"]), up(a["flags"])
        tfluids.advectScalar(0.1, s, U, fl, "maccormackOurs")
        loss = torch.empty(4, dtype=torch.float64, device=DEV)
        gP, gU = torch.empty_like(s), torch.empty_like(U)
        tfluids.fluidCriterion(up(a["p"]), U, up(b["p"]), up(b["U"]), fl, None, 0.7, 1.3, 2.5, True, loss, gP, gU)
        return {}
    return run


def grown(dims):
    """a larger grid of the same dimensionality, no extent a multiple of the case's"""
    Z, Y, X = dims
    return ((Z + 3) if Z > 1 else 1, Y + 5, X + 9)


# ---- solveLinearSystemPCG ---------------------------------------------------------------------------------------------------------
def _pcg_runs(problems, is3d, pc, direct_of=None):
    """problems: which -> (flags, div, tol)"""
    import torch
    from fluidnet_amd import tfluids

    def run_of(f, div, tol):
        def run():
            p = torch.full(div.shape, float("nan"), device=DEV)
            res = tfluids.solveLinearSystemPCG(p, up(f), up(div), is3d, tol, 1000, pc)
            return dict(p=down(p), residual=res, pcgLastIterations=tfluids.pcgLastIterations(p))
        return run
    return {w: run_of(*v) for w, v in problems.items()}


def _pcg_direct(f, div, is3d, pc, tol):
    import torch
    from fluidnet_amd import tfluids

    def direct(view, accepted):
        p, tf, td = torch.full(div.shape, 5.0, device=DEV), up(f), up(div)
        lib, ctx = tfluids._context(p)
        res = ctypes.c_float(3.0)
        out = refusal(lambda: lib.tfl_solveLinearSystemPCG(ctx, tfluids._tt(p), tfluids._tt(tf), tfluids._tt(td), int(is3d), pc.encode(), tol, 1000,
                                                           0, ctypes.c_void_p(view.data_ptr()), view.numel(), ctypes.byref(res)), dict(p=p), accepted,
                      lambda: [] if res.value == 3.0 else ["the refused call wrote the residual"])
        return out
    return direct


def pcg_target(dims, seed, split, B, tol, vel, pc):
    import scenes
    sc, f, _, div = scenes.pcg_problem(oracle(), dims, seed, split=split, B=B, vel_cells=vel)
    _, f2, _, div2 = scenes.pcg_problem(oracle(), dims, seed + 50, split=True, B=B, vel_cells=vel)
    big = grown(dims)
    _, f3, _, div3 = scenes.pcg_problem(oracle(), big, seed + 70, split=True, B=B, vel_cells=vel)
    runs = _pcg_runs({"case": (f, div, tol), "scene": (f2, div2, tol / 10), "larger": (f3, div3, tol)}, sc["is3d"], pc)
    runs["foreign"] = foreign(dims, B)
    return TmpTarget(runs, 8, _pcg_direct(f, div, sc["is3d"], pc, tol), short=True)


PCG_ROWS = [  # (dims, seed, split, B, tol, vel_cells, the literal of the existing table)
    ((1, 24, 28), 3, False, 1, 1e-5, 2.0, "((1, 24, 28), 3, False, 1, 1e-5)"),
    ((9, 11, 13), 4, False, 2, 1e-5, 2.0, "((9, 11, 13), 4, False, 2, 1e-5)"),
    ((20, 24, 40), 13, False, 1, 1e-4, 0.3, "((20, 24, 40), 13, False)"),
]


def mg_target(name):
    import scenes
    import pcg_mg_ref64 as M
    f, div, is3d = M.case(name)
    other = name[:-5] if name.endswith("_open") else name + "_open"       # the same shape, the patch of empty cells added / taken away
    f2, div2, _ = M.case(other)
    dims = M.WIDE_CASES[name]["dims"]
    _, f3, _, div3 = scenes.pcg_problem(oracle(), grown(dims), 77, split=True, vel_cells=2.0)
    runs = _pcg_runs({"case": (f, div, 1e-5), "scene": (f2, div2, 1e-6), "larger": (f3, div3, 1e-5)}, is3d, "mg")
    runs["foreign"] = foreign(dims, f.shape[0])
    return TmpTarget(runs, 8, _pcg_direct(f, div, is3d, "mg", 1e-5), short=True)


MG_CASES = ("one_level_4x12x14", "one_level_4x12x14_open", "wide2_24x36x40", "wide2_24x36x40_open", "wide2_flat_132x136",
            "wide2_flat_132x136_open")


# ---- solveLinearSystemPCGBatched --------------------------------------------------------------------------------------------------
def batched_target(problem, pc):
    """problem: () -> (flags, div, is3d, flags of the other scene, its div, dims)"""
    import torch
    import scenes
    import pcg_batched_cases as PB
    from fluidnet_amd import tfluids
    f, div, is3d, f2, div2, dims = problem()
    B = f.shape[0]
    f3, _, div3, _ = PB.build_batch(oracle(), grown(dims), PB.KINDS[:B] if B <= len(PB.KINDS) else PB.KINDS, seed=PB.SEED + 1)
    f3, div3 = f3[:B], div3[:B]

    def run_of(fl, dv, tol):
        def run():
            p = torch.full(dv.shape, float("nan"), device=DEV)
            res, its = tfluids.solveLinearSystemPCGBatched(p, up(fl), up(dv), is3d, tol, 1000, pc)
            return dict(p=down(p), residuals=res, iterations=its, pcgLastIterations=tfluids.pcgLastIterations(p))
        return run

    def direct(view, accepted):
        p, tf, td = torch.full(div.shape, 5.0, device=DEV), up(f), up(div)
        lib, ctx = tfluids._context(p)
        res, its = np.full(B, 3.0, np.float32), np.full(B, 3, np.int64)
        out = refusal(lambda: lib.tfl_solveLinearSystemPCGBatched(ctx, tfluids._tt(p), tfluids._tt(tf), tfluids._tt(td), int(is3d), pc.encode(), 1e-5,
                                                                  1000, ctypes.c_void_p(view.data_ptr()), view.numel(),
                                                                  res.ctypes.data_as(ctypes.c_void_p), its.ctypes.data_as(ctypes.c_void_p)), dict(p=p), accepted,
                      lambda: [] if (res == 3.0).all() and (its == 3).all() else ["the refused call wrote residuals or iterations"])
        return out
    runs = {"case": run_of(f, div, 1e-5), "scene": run_of(f2, div2, 1e-6), "larger": run_of(f3, div3, 1e-5), "foreign": foreign(dims, B)}
    return TmpTarget(runs, 8, direct, short=True)


def _mixed(name):
    def problem():
        import pcg_batched_cases as PB
        f, _, div, is3d = PB.batch(name)
        f2, _, div2, _ = PB.batch(name, PB.KINDS[::-1])          # every item another topology: pockets and splits where boxes were
        return f, div, is3d, f2, div2, PB.BATCHES[name]
    return problem


def _wide_pair():
    """(24, 36, 40) as a batch of two: the closed and the open case of pcg_mg_ref64.WIDE_CASES, the other scene the two swapped"""
    import pcg_mg_ref64 as M
    a, b = M.case("wide2_24x36x40"), M.case("wide2_24x36x40_open")
    f, div = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    f2, div2 = np.concatenate([b[0], a[0]]), np.concatenate([b[1], a[1]])
    return f, div, a[2], f2, div2, (24, 36, 40)


# ---- normalizePressureMean, velocityDivergenceNorm, fluidCriterion --------------------------------------------------------------------
def normalize_target(dims, seed):
    import torch
    import scenes
    from fluidnet_amd import tfluids

    def problem(d, s, B=2):
        sc, f, _, div = scenes.pcg_problem(oracle(), d, s, split=True, B=B)
        return f, (np.random.RandomState(s).randn(*div.shape) * 3 + 5).astype(np.float32), sc["is3d"]

    def run_of(f, p0, is3d):
        def run():
            p = up(p0)
            tfluids.normalizePressureMean(p, up(f), is3d)
            return dict(p=down(p))
        return run
    case = problem(dims, seed)
    other = problem(dims, seed + 50)
    other[0][:, :, :, other[0].shape[3] // 3, :] = 2.0        # one more wall: more components than the case
    big = problem(grown(dims), seed + 70)

    def direct(view, accepted):
        p, tf = up(case[1]), up(case[0])
        lib, ctx = tfluids._context(p)
        return refusal(lambda: lib.tfl_normalizePressureMean(ctx, tfluids._tt(p), tfluids._tt(tf), int(case[2]), ctypes.c_void_p(view.data_ptr()),
                                                             view.numel()), dict(p=p), accepted)
    runs = {"case": run_of(*case), "scene": run_of(*other), "larger": run_of(*big), "foreign": foreign(dims, 2)}
    return TmpTarget(runs, 8, direct, short=True)


def divnorm_target(name):
    import torch
    import scenes
    import divnorm_ref as D
    from fluidnet_amd import tfluids
    _, dims, B, _ = next(c for c in D.CASES if c[0] == name)

    def run_of(U, f):
        def run():
            return dict(norm=down(tfluids.velocityDivergenceNorm(up(U), up(f))))
        return run
    U, f = D.make_case(name)
    o = scenes.make_scene(dims, seed=940, B=B, vel_cells=0.4, empty_cells=True)
    g = scenes.make_scene(grown(dims), seed=941, B=B, vel_cells=0.4)

    def direct(view, accepted):
        tU, tf = up(U), up(f)
        out_ = torch.full((B,), 3.0, dtype=torch.float64, device=DEV)
        lib, ctx = tfluids._context(tU)
        return refusal(lambda: lib.tfl_velocityDivergenceNorm(ctx, tfluids._tt(tU), tfluids._tt(tf), int(dims[0] > 1), ctypes.c_void_p(out_.data_ptr()),
                                                              ctypes.c_void_p(view.data_ptr()), view.numel()), dict(norm=out_), accepted)
    runs = {"case": run_of(U, f), "scene": run_of(o["U"], o["flags"]), "larger": run_of(g["U"], g["flags"]), "foreign": foreign(dims, B)}
    return TmpTarget(runs, 8, direct, short=True)


def criterion_target(name, module):
    """module: through nn.FluidCriterion and autograd (what the training closure calls) instead of tfluids.fluidCriterion"""
    import torch
    import scenes
    import criterion_ref as R
    from fluidnet_amd import tfluids
    from fluidnet_amd.criterion import FluidCriterion
    _, dims, B, _ = R.case(name)
    lam = R.LAMBDAS["all"]

    def fields(d, s):
        a = scenes.make_scene(d, seed=s, B=B, vel_cells=0.4, empty_cells=True)
        b = scenes.make_scene(d, seed=s + 100, B=B, vel_cells=0.4)
        return a["p"], a["U"], b["p"], b["U"], a["flags"]

    def run_of(pP, UP, pT, UT, fl):
        def plain():
            t = [up(x) for x in (pP, UP, pT, UT, fl)]
            w = tfluids.criterionWeight(t[4], R.BORDER[1], R.BORDER[0])
            loss = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
            gP, gU = torch.full_like(t[0], float("nan")), torch.full_like(t[1], float("nan"))
            tfluids.fluidCriterion(*t, w, lam[0], lam[1], lam[2], True, loss, gP, gU)
            return dict(loss=down(loss), gradP=down(gP), gradU=down(gU))

        def through_module():
            t = [up(x) for x in (pP, UP, pT, UT, fl)]
            t[0].requires_grad_(True)
            t[1].requires_grad_(True)
            crit = FluidCriterion(*lam, borderWeight=R.BORDER[0], borderWidth=R.BORDER[1])
            total = crit((t[0], t[1]), (t[2], t[3], t[4]))
            total.backward()
            return dict(total=down(total), terms=down(torch.stack([crit.pLoss, crit.uLoss, crit.divLoss])), gradP=down(t[0].grad), gradU=down(t[1].grad))
        return through_module if module else plain
    case = R.make_case(name)

    def direct(view, accepted):
        t = [up(x) for x in case]
        loss = torch.full((4,), 3.0, dtype=torch.float64, device=DEV)
        gP, gU = torch.full_like(t[0], 3.0), torch.full_like(t[1], 3.0)
        lib, ctx = tfluids._context(t[0])
        return refusal(lambda: lib.tfl_fluidCriterion(ctx, *[tfluids._tt(x) for x in t], None, lam[0], lam[1], lam[2], 1, int(dims[0] > 1),
                                                      ctypes.c_void_p(loss.data_ptr()), tfluids._tt(gP), tfluids._tt(gU),
                                                      ctypes.c_void_p(view.data_ptr()), view.numel()), dict(loss=loss, gradP=gP, gradU=gU), accepted)
    runs = {"case": run_of(*case), "scene": run_of(*fields(dims, 950)), "larger": run_of(*fields(grown(dims), 951)), "foreign": foreign(dims, B)}
    return TmpTarget(runs, 8, direct, short=True)


# ---- operators with temporaries ----------------------------------------------------------------------------------------------------
def operator_target(op, dims, B, seed, kw=None):
    """op: (scene dict) -> results. The temporaries are tensors carved out of the shared buffer: no alignment promise to hold, no
    size to fall short of"""
    import scenes
    kw = kw or {}

    def run_of(d, s, **more):
        sc = scenes.make_scene(d, seed=s, B=B, **dict(kw, **more))
        return lambda: op(sc)
    runs = {"case": run_of(dims, seed), "scene": run_of(dims, seed + 50, empty_cells=True, stick=True, noise=1.0),
            "larger": run_of(grown(dims), seed + 70), "foreign": foreign(dims, B)}
    return TmpTarget(runs, None)


def op_advect_scalar(sc):
    from fluidnet_amd import tfluids
    s, U, f = up(sc["density"]), up(sc["U"]), up(sc["flags"])
    tfluids.traceErrors(s)
    tfluids.advectScalar(sc["dt"], s, U, f, "maccormackOurs")
    return dict(s=down(s), traceErrors=tfluids.traceErrors(s))


def op_advect_vel(sc):
    from fluidnet_amd import tfluids
    U, f = up(sc["U"]), up(sc["flags"])
    tfluids.traceErrors(U)
    tfluids.advectVel(sc["dt"], U, f, "maccormackOurs")
    return dict(U=down(U), traceErrors=tfluids.traceErrors(U))


def op_vorticity(sc):
    """both forms of the operator: in place (four temporaries, always two launches) and U = USrc + confinement (two launches;
    the fused kernel, which takes no temporary, from 0.6 M cells on or where TFL_VORT_FUSED=1 forces it)"""
    import torch
    from fluidnet_amd import tfluids
    U, f = up(sc["U"]), up(sc["flags"])
    dst = torch.full_like(U, float("nan"))
    tfluids.vorticityConfinement(dst, f, 0.7, USrc=U)
    tfluids.vorticityConfinement(U, f, 0.7)
    return dict(inplace=down(U), from_src=down(dst))


def op_jacobi(sc):
    from fluidnet_amd import tfluids
    U, f = up(sc["U"]), up(sc["flags"])
    tfluids.setWallBcsForward(U, f)
    div = up(np.zeros_like(sc["p"]))
    tfluids.velocityDivergenceForward(U, f, div)
    out = {}
    for iters in (1, 20):      # 2-D grids of up to 16 K cells with a fixed count: the one-launch LDS solve
        p = up(np.full_like(sc["p"], 3.0))
        out["residual%d" % iters] = tfluids.solveLinearSystemJacobi(p, f, div, sc["is3d"], 0.0, iters)
        out["p%d" % iters] = down(p)
    p = up(np.zeros_like(sc["p"]))
    out["residual_tol"] = tfluids.solveLinearSystemJacobi(p, f, div, sc["is3d"], 1e-3, 300)
    out["p_tol"] = down(p)
    return out


def op_blur(sc):
    import torch
    from fluidnet_amd import tfluids
    src = up(sc["U"])
    out = {}
    for rad in (1, 5):
        dst = torch.full_like(src, float("nan"))
        tfluids.rectangularBlur(src, rad, sc["is3d"], dst)
        out["blur%d" % rad] = down(dst)
    return out


def op_vorticity_items(sc):
    from fluidnet_amd import tfluids
    U, f = up(sc["U"]), up(sc["flags"])
    tfluids.vorticityConfinementItems(U, f, (0.4, 9.0, 0.07), on=(1, 0, 1))
    return dict(U=down(U))


# ---- the step --------------------------------------------------------------------------------------------------------------------
STEP_BASE = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.0, gravityScale=0, vorticityConfinementAmp=0)


def _step_direct(entry, mconf, batch_of, model_of):
    """the step through ctypes on a view the library must refuse"""
    def direct(view, accepted):
        from fluidnet_amd import tfluids
        from fluidnet_amd.simulate import _native_args
        batch = batch_of()
        lib, ctx = tfluids._context(batch["UDiv"])
        prm, st, keep = _native_args(lib, ctx, mconf, batch, model_of())
        outs = {k: batch[k] for k in ("pDiv", "UDiv", "density")}
        out = refusal(lambda: getattr(lib, entry)(ctx, ctypes.byref(prm), ctypes.byref(st), ctypes.c_void_p(view.data_ptr()), view.numel()), outs, accepted)
        del keep
        return out
    return direct


def step_target(which, split):
    """two steps of tfl_simulate_step (split: each as tfl_simulate_step with outputDiv + tfl_simulate_project) on the smallest
    grid of tests/test_hip_simulate.py for the projection at hand"""
    import torch
    import test_hip_simulate as T
    from oracle import simulate_np as S
    from fluidnet_amd import FluidNetModel, tfluids
    from fluidnet_amd.simulate import project, simulate_native
    model = None
    if which == "2d_jacobi":
        dims, args, mconf = (1, 40, 44), (0.08, 5.0, 3), dict(STEP_BASE, simMethod="jacobi", maxIter=15)
    elif which == "3d_jacobi":
        dims, args, mconf = (12, 14, 16), (0.15, 1.0, None), dict(STEP_BASE, simMethod="jacobi", maxIter=12, buoyancyScale=0, gravityScale=0.3,
                                                                    gravity=[0.2, 1.0, -0.3])
    elif which == "2d_convnet":
        dims, args, mconf = (1, 36, 40), (0.1, 4.0, None), dict(STEP_BASE, simMethod="convnet", vorticityConfinementAmp=0.4)
        model = FluidNetModel(T._layers2d(), False)
    elif which == "3d_convnet":
        dims, args, mconf = (12, 14, 16), (0.15, 1.0, None), dict(STEP_BASE, simMethod="convnet", buoyancyScale=0, vorticityConfinementAmp=1.5)
        model = FluidNetModel(S.default_3d_layers(seed=5), True)
    elif which in ("2d_pcg_ic0", "2d_pcg_mg"):
        dims, args = (1, 48, 48), (0.08, 4.0, 5)
        mconf = dict(STEP_BASE, maccormackStrength=0.75, vorticityConfinementAmp=0.5, simMethod="pcg", maxIter=400, pcgPrecond=which[-3:].lstrip("_"))
    else:
        assert which in ("3d_pcg_ic0", "3d_pcg_mg"), which
        dims, args = (20, 24, 24), (0.15, 1.0, 5)
        mconf = dict(STEP_BASE, maccormackStrength=0.75, vorticityConfinementAmp=0.5, simMethod="pcg", maxIter=400, pcgPrecond=which[-3:].lstrip("_"))

    def scene(d, rad, usc, obst):
        b = T._plume_batch(d, rad, usc, obstacles_seed=obst)
        if mconf["simMethod"] == "pcg":      # open the top: a well-posed system (test_simulate_pcg_projection)
            Y = d[1]
            top = b["flags"][:, :, 1:-1, Y - 2, 1:-1] if d[0] > 1 else b["flags"][:, :, :, Y - 2, 1:-1]
            top[...] = 4.0
        return b

    def run_of(b):
        def run():
            batch = T._to_dev(b, DEV)
            tfluids.traceErrors(batch["UDiv"])
            for _ in range(2):
                if split:
                    simulate_native(None, mconf, batch, model, outputDiv=True)
                    project(None, mconf, batch, model)
                else:
                    simulate_native(None, mconf, batch, model)
            out = {k: down(batch[k]) for k in ("pDiv", "UDiv", "density")}
            out["traceErrors"] = tfluids.traceErrors(batch["UDiv"])
            if model is not None:
                out["range_errors"] = model.range_errors(batch["UDiv"])
                assert out["range_errors"] == 0
            if mconf["simMethod"] == "pcg":
                out["pcgLastIterations"] = tfluids.pcgLastIterations(batch["UDiv"])
            return out
        return run
    case = scene(dims, *args)
    other = scene(dims, args[0] * 1.5, args[1] * 1.7, 11)      # obstacles where the case may have none, a faster and wider plume
    big = scene(grown(dims), args[0], args[1], args[2])
    entry = "tfl_simulate_project" if split else "tfl_simulate_step"
    runs = {"case": run_of(case), "scene": run_of(other), "larger": run_of(big), "foreign": foreign(dims, 1)}
    return TmpTarget(runs, 16, _step_direct(entry, mconf, lambda: T._to_dev(case, DEV), lambda: model), short=True)


STEP_SOURCES = {
    "2d_jacobi": ("(1, 40, 44), 0.08, 5.0, obstacles_seed=3", "simMethod=\"jacobi\", maxIter=15"),
    "3d_jacobi": ("simMethod=\"jacobi\", maxIter=12, buoyancyScale=0, gravityScale=0.3", "(12, 14, 16), 0.15, 1.0"),
    "2d_convnet": ("(1, 36, 40), 0.1, 4.0", "simMethod=\"convnet\", vorticityConfinementAmp=0.4"),
    "3d_convnet": ("(12, 14, 16), 0.15, 1.0", "simMethod=\"convnet\", buoyancyScale=0, vorticityConfinementAmp=1.5"),
    "2d_pcg_ic0": ("((1, 48, 48), 0.08, 4.0)",), "2d_pcg_mg": ("((1, 48, 48), 0.08, 4.0)",),
    "3d_pcg_ic0": ("((20, 24, 24), 0.15, 1.0)",), "3d_pcg_mg": ("((20, 24, 24), 0.15, 1.0)",),
}


def items_target(case_index, over, split):
    """two steps of tfl_simulate_step_items on R = 2 runs of tests/datagen_batched_cases.py (plans 0 and 3; the other scene:
    plans 4 and 6)"""
    import datagen_batched_cases as DC
    from fluidnet_amd import datagen, tfluids
    from fluidnet_amd.simulate import _item_array, _native_args, project_items, simulate_items
    is3D, dims = DC.CASES[case_index]

    def setup(d, runs):
        plans = DC.plans(is3D, d, runs, pcgPrecond="mg")
        forces = [{k: datagen.mconf_of(p)[k] for k in ("gravity", "buoyancyScale", "gravityScale", "vorticityConfinementAmp")} for p in plans]
        return plans, forces, dict(datagen.mconf_of(plans[0]), **over)

    def run_of(d, runs):
        plans, forces, mconf = setup(d, runs)

        def run():
            batch = datagen.join_states([datagen.init_state(p, DEV) for p in plans])
            tfluids.traceErrors(batch["UDiv"])
            for _ in range(2):
                if split:
                    simulate_items(None, mconf, batch, forces, outputDiv=True)
                    project_items(None, mconf, batch, forces)
                else:
                    simulate_items(None, mconf, batch, forces)
            out = {k: down(batch[k]) for k in ("pDiv", "UDiv", "density")}
            out["traceErrors"] = tfluids.traceErrors(batch["UDiv"])
            out["pcgLastIterations"] = tfluids.pcgLastIterations(batch["UDiv"])
            return out
        return run
    plans, forces, mconf = setup(dims, (0, 3))
    entry = "tfl_simulate_project_items" if split else "tfl_simulate_step_items"

    def direct(view, accepted):
        batch = datagen.join_states([datagen.init_state(p, DEV) for p in plans])
        lib, ctx = tfluids._context(batch["UDiv"])
        prm, st, keep = _native_args(lib, ctx, mconf, batch, None)
        items = _item_array(mconf, forces)
        out = refusal(lambda: getattr(lib, entry)(ctx, ctypes.byref(prm), items, len(forces), ctypes.byref(st), ctypes.c_void_p(view.data_ptr()),
                                                  view.numel()), {k: batch[k] for k in ("pDiv", "UDiv", "density")}, accepted)
        del keep
        return out
    runs = {"case": run_of(dims, (0, 3)), "scene": run_of(dims, (4, 6)), "larger": run_of(grown(dims), (0, 3)), "foreign": foreign(dims, 2)}
    return TmpTarget(runs, 16, direct, short=True)


# ---- the z-slab step ---------------------------------------------------------------------------------------------------------------
class SlabTarget(H.Target):
    """tfl_simulate_step_slab, tfl_slab_divergence_norm and tfl_slab_drain (with the ConvNet projection tfl_model_begin /
    tfl_model_finish inside the step) on two virtual ranks of tests/test_hip_slab_methods.py: one slot per rank, each rank's
    SlabSimulation.ws replaced by the interior of its arena before the first step. A run is: step, step, the divergence norm
    (it finishes the messages the second step left in flight and puts its plane sums into the compute region), a third step,
    drain. The workspace's message buffers carry the p / U halos from one step to the next (the header says so), so the
    pre-state is what the FIRST step of a run finds, when slab.in_flight is 0 and nothing is carried: no region is excluded
    there, and between the steps nothing is seeded. scenes: which -> the un-cut batch (numpy)."""
    STEPS = 3

    def __init__(self, scenes_, conf, layers):
        self.scenes, self.conf, self.layers = scenes_, conf, layers
        self.slots = ("rank0", "rank1")
        self.align = {s: 16 for s in self.slots}
        self.short = self.slots
        self._need = {}

    def _sims(self, which):
        import test_hip_slab_jacobi as J
        import test_hip_slab_methods as SM
        ref = SM._dev(self.scenes[which])
        return SM.sims_for(ref, self.conf, J.uneven_cuts(ref["flags"].size(2), 2), layers=self.layers)

    def need(self, which):
        if which not in self._need:
            sims = self._sims(which)
            self._need[which] = {"rank%d" % r: int(s.ws.numel()) for r, s in enumerate(sims)}
            for s in sims:
                s.close()
        return self._need[which]

    @staticmethod
    def _ranks(sims, work, active=None):
        """work(rank, sim) in one thread per rank of `active` (all by default), as fluidnet_amd.dist.run_virtual_ranks runs the
        steps: an error in one rank, or a rank that ends without its neighbour, breaks the hub's barrier for the other"""
        import threading
        import torch
        errs, out = [], {}
        dev = sims[0].batch["UDiv"].device

        def run(r, sim):
            try:
                torch.cuda.set_device(dev)
                out[r] = work(r, sim)
            except Exception as e:   # noqa: BLE001
                errs.append(e)
            finally:
                if errs or out.get(r) == "left":
                    sim.comm.hub.barrier.abort()
        ts = [threading.Thread(target=run, args=(r, s), daemon=True) for r, s in enumerate(sims) if active is None or r in active]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        if any(t.is_alive() for t in ts):
            sims[0].comm.hub.barrier.abort()
            raise AssertionError("a virtual rank did not come back")
        torch.cuda.synchronize(dev)
        if errs:
            raise errs[0]
        return out

    def run(self, which, spans):
        import torch
        sims = self._sims(which)
        for r, s in enumerate(sims):
            view = spans["rank%d" % r].view()
            assert view.numel() == s.ws.numel(), (which, r, view.numel(), s.ws.numel())
            s.ws = view
            s.comm.bind(view)
        norms = {}

        def work(r, sim):
            sim.step()
            sim.step()
            norms[r] = sim.divergence_norm()
            sim.step()
            assert sim.slab.in_flight & 0xF, "the eager step left no message for tfl_slab_drain to finish"
            sim.drain()
        try:
            self._ranks(sims, work)
            out = {}
            for r, s in enumerate(sims):
                for k in ("pDiv", "UDiv", "density"):
                    out["rank%d_%s" % (r, k)] = down(s.lay.owned(s.batch[k]))
                out["rank%d_norm" % r] = down(norms[r])
                assert out["rank%d_pDiv" % r].any() and float(norms[r].max()) > 0, "rank %d: the steps projected nothing" % r
            assert torch.equal(norms[0], norms[1])
        finally:
            for s in sims:
                s.close()
        return out

    def run_refused(self, spans, accepted=False):
        """the three entries through ctypes, in each rank's thread. Only a rank whose scratch is short or misaligned calls (its
        neighbour would be accepted and wait for it in the first exchange); accepted: both ranks, every call must succeed"""
        import torch
        sims = self._sims("case")
        need = self.need("case")
        bad = {r for r, s in enumerate(self.slots) if spans[s].n < need[s] or spans[s].view().data_ptr() % 16}
        assert bool(bad) != accepted, (bad, accepted)
        complaints = []

        def work(r, sim):
            view = spans["rank%d" % r].view()
            sim.comm.bind(view)
            lib, ctx = sim._context()
            norm = torch.full((sim.batch["UDiv"].size(0),), 3.0, dtype=torch.float64, device=DEV)
            tail = (ctypes.byref(sim.slab), ctypes.byref(sim.comm.struct), ctypes.c_void_p(view.data_ptr()), view.numel())
            outs = dict({k: sim.batch[k] for k in ("pDiv", "UDiv", "density")}, norm=norm)
            calls = [("tfl_simulate_step_slab", lambda: lib.tfl_simulate_step_slab(ctx, ctypes.byref(sim.prm), ctypes.byref(sim.st), *tail)),
                     ("tfl_slab_divergence_norm", lambda: lib.tfl_slab_divergence_norm(ctx, ctypes.byref(sim.st), *tail, ctypes.c_void_p(norm.data_ptr()))),
                     ("tfl_slab_drain", lambda: lib.tfl_slab_drain(ctx, ctypes.byref(sim.st), *tail))]
            for name, call in calls:
                got = refusal(call, outs, accepted)
                complaints.extend("rank %d, %s: %s" % (r, name, c) for c in got)
                if got and accepted:
                    return "left"         # the neighbour must not wait for this rank
            if not accepted and (sim.slab.in_flight & 0xF):
                return "left"             # a step that was taken after all: likewise
        try:
            self._ranks(sims, work, None if accepted else bad)
        finally:
            for s in sims:
                s.close()
        return complaints


def slab_target(sim):
    """tests/test_hip_slab_methods.py, two ranks on uneven cuts: test_methods_jacobi_slabs_equal_uncut's scene and mconf
    (maccormackOurs), or test_methods_convnet_slabs_equal_uncut's with its model. The other scene: two batch items' worth of
    obstacles folded into one (the second plume's boxes added) and another jet; the larger grid: four more planes, other Y / X"""
    import test_hip_slab_methods as SM
    from oracle import simulate_np as S
    Y, X = (20, 24) if sim == "jacobi" else (24, 32)
    case = SM.scene(22, Y, X)
    other = SM.scene(22, Y, X, jet=0.5)
    import test_hip_slab_jacobi as J
    more = J.scene(22, Y, X, B=2)["flags"][1:2]
    other["flags"] = np.ascontiguousarray(np.maximum(other["flags"], np.where(more == 2.0, 2.0, 0.0)).astype(np.float32))
    big = SM.scene(26, Y + 4, X + 8)
    layers = S.default_3d_layers(seed=2) if sim == "convnet" else None
    return SlabTarget({"case": case, "scene": other, "larger": big}, SM.mconf("maccormackOurs", sim), layers)


# ---- the projection ConvNet: its own scratch (ProjectionNet._work, the trainer's _bwd_work) and the tape ------------------------------
class ModelTarget(H.Target):
    """tfl_model_forward, or tfl_model_forward_train + tfl_model_backward [+ tfl_model_backward_input], through ctypes on the
    interior pointers with exactly the floats the size functions return. The header promises 8 bytes for every one of these
    arrays (tfl_model.hpp check_buffer), so all of them move to 8 mod 16 together. inputs: which -> (pDiv, UDiv, flags[, gradP, gradU])"""

    def __init__(self, model, inputs, train, with_input_grad):
        import torch
        from fluidnet_amd import tfluids
        from fluidnet_amd.train import ProjectionNet
        self.inputs, self.train, self.with_input_grad = inputs, train, train and with_input_grad
        self.net = ProjectionNet(model, device=DEV, multires=train and any(p > 1 for p in (model.pool or []))) if train else None
        self.model = model
        self.slots = ("work",) + (("tape", "bwd") + (("bwd_input",) if self.with_input_grad else ()) if train else ())
        self.align = {s: 8 for s in self.slots}
        self.short = self.slots
        like = torch.empty(1, device=DEV)
        self.lib, self.ctx = tfluids._context(like)
        self.h = (self.net or self.model)._handle(self.lib, self.ctx, like.device.index)

    def need(self, which):
        B, _, Z, Y, X = self.inputs[which][2].shape
        lib, h = self.lib, self.h
        out = {"work": int(lib.tfl_model_workspace_floats(h, B, Z, Y, X))}
        if self.train:
            out["tape"] = int(lib.tfl_model_tape_floats(h, B, Z, Y, X))
            out["bwd"] = int(lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X))
            if self.with_input_grad:
                out["bwd_input"] = int(lib.tfl_model_backward_input_workspace_floats(h, B, Z, Y, X))
        assert all(v > 0 for v in out.values()), out
        return out

    def _calls(self, which, spans, fill, only=None):
        """the entry's calls one after the other: [(name, rc)], and the outputs by name (pre-filled with `fill`); only: the
        calls to make (None: all)"""
        import torch
        from fluidnet_amd import tfluids
        from fluidnet_amd.train import _ptr_array
        lib, ctx, h, tt = self.lib, self.ctx, self.h, tfluids._tt
        ins = [up(a) for a in self.inputs[which]]
        pDiv, UDiv, flags = ins[:3]
        ptr = lambda s: ctypes.c_void_p(spans[s].view().data_ptr())      # noqa: E731
        p, U = torch.full_like(pDiv, fill), torch.full_like(UDiv, fill)
        outs, rcs = dict(p=p, U=U), []
        want = lambda name: only is None or name in only      # noqa: E731
        if not self.train:
            from fluidnet_amd.simulate import wall_plan
            wall_plan(lib, ctx, flags)
            rcs.append(("forward", lib.tfl_model_forward(ctx, h, tt(pDiv), tt(UDiv), tt(flags), tt(p), tt(U), ptr("work"), spans["work"].n, None, None,
                                                         0, 0.0, 0.0)))
            return rcs, outs
        gP, gU = ins[3:5]
        if want("forward_train"):
            rcs.append(("forward_train", lib.tfl_model_forward_train(ctx, h, tt(pDiv), tt(UDiv), tt(flags), tt(p), tt(U), ptr("work"),
                                                                     spans["work"].n, ptr("tape"), spans["tape"].n)))
        # the gradient outputs of an accumulate = 0 call: whatever they held must not show
        gw, gb = [torch.full_like(w, fill) for w in self.net.weights], [torch.full_like(b, fill) for b in self.net.biases]
        if want("backward"):
            rcs.append(("backward", lib.tfl_model_backward(ctx, h, tt(flags), tt(gP), tt(gU), ptr("tape"), spans["tape"].n, ptr("bwd"),
                                                           spans["bwd"].n, _ptr_array(gw), _ptr_array(gb), 0)))
        outs.update({"gradWeight%d" % i: t for i, t in enumerate(gw)})
        outs.update({"gradBias%d" % i: t for i, t in enumerate(gb)})
        if self.with_input_grad and want("backward_input"):
            gw2, gb2 = [torch.full_like(w, fill) for w in self.net.weights], [torch.full_like(b, fill) for b in self.net.biases]
            gp, gu = torch.full_like(pDiv, fill), torch.full_like(UDiv, fill)
            rcs.append(("backward_input", lib.tfl_model_backward_input(ctx, h, tt(flags), tt(pDiv), tt(UDiv), tt(U), tt(gP), tt(gU), ptr("tape"),
                                                                       spans["tape"].n, ptr("bwd_input"), spans["bwd_input"].n, _ptr_array(gw2),
                                                                       _ptr_array(gb2), 0, tt(gp), tt(gu))))
            outs.update({"in_gradWeight%d" % i: t for i, t in enumerate(gw2)})
            outs.update({"in_gradBias%d" % i: t for i, t in enumerate(gb2)})
            outs.update(gradPDiv=gp, gradUDiv=gu)
        return rcs, outs

    def run(self, which, spans):
        import torch
        from fluidnet_amd import TfluidsError
        rcs, outs = self._calls(which, spans, float("nan"))
        torch.cuda.synchronize()
        for name, rc in rcs:
            if rc != 0:
                raise TfluidsError("%s: %s" % (name, self.lib.tfl_last_error(self.ctx).decode()))
        out = {k: down(v) for k, v in outs.items()}
        out["range_errors"] = (self.net or self.model).range_errors(outs["p"])
        assert out["range_errors"] == 0      # after every run
        return out

    USES = {"forward": ("work",), "forward_train": ("work", "tape"), "backward": ("tape", "bwd"), "backward_input": ("tape", "bwd_input")}

    def run_refused(self, spans, accepted=False):
        """the calls that take a short slot must be refused; the others are not made (a backward entry on a tape that no
        forward_train wrote would be accepted, and compute on whatever the tape holds). accepted: every call, all must succeed"""
        import torch
        need = self.need("case")
        short = {s for s in self.slots if spans[s].n < need[s]}
        assert bool(short) != accepted, (short, accepted)
        rcs, outs = self._calls("case", spans, 3.0, None if accepted else {c for c, uses in self.USES.items() if short & set(uses)})
        torch.cuda.synchronize()
        assert rcs, "no call takes the short slot"
        if accepted:
            return ["%s was not accepted (returned %d)" % (name, rc) for name, rc in rcs if rc != 0]
        bad = ["%s was not refused with TFL_EINVAL (returned %d)" % (name, rc) for name, rc in rcs if rc != -1]
        return bad + ["the refused call changed %s" % k for k, v in outs.items() if not bool((v == 3.0).all())]


def _rough_inputs(dims, B, seed, grads, frac=0.08):
    import scenes
    sc = scenes.rough_scene(dims, seed=seed, B=B, obstacle_frac=frac)
    out = [sc["p"], sc["U"], sc["flags"]]
    if grads:
        rng = np.random.RandomState(seed + 1)
        out += [(rng.randn(*sc["p"].shape) + 0.5).astype(np.float32), rng.randn(*sc["U"].shape).astype(np.float32)]
    return tuple(out)


def _conv_env(path):
    """the model is created under TFL_CONV_PATH = path (read at model creation)"""
    import contextlib

    @contextlib.contextmanager
    def env():
        old = os.environ.get("TFL_CONV_PATH")
        if path:
            os.environ["TFL_CONV_PATH"] = path
        else:
            os.environ.pop("TFL_CONV_PATH", None)
        try:
            yield
        finally:
            if old is None:
                os.environ.pop("TFL_CONV_PATH", None)
            else:
                os.environ["TFL_CONV_PATH"] = old
    return env()


def forward_target(build, path, dims, B, larger):
    """build: (FluidNetModel class) -> model; the scenes are test_hip_conv_bound's rough kind (white noise, salt-and-pepper obstacles)"""
    from fluidnet_amd import FluidNetModel
    with _conv_env(path):
        model = build(FluidNetModel)
        # (the larger grid: 8 more cells along every axis keeps any model's downsampling factor)
        larger = larger or ((dims[0] + 8) if dims[0] > 1 else 1, dims[1] + 8, dims[2] + 8)
        inputs = {"case": _rough_inputs(dims, B, 100, False, 0.1), "scene": _rough_inputs(dims, B, 171, False, 0.3),
                  "larger": _rough_inputs(larger, B, 172, False, 0.1)}
        return ModelTarget(model, inputs, False, False)      # (the handle is created here, under the path)


def _default_2d(F):
    import test_hip_simulate as T
    return F(T._layers2d(), False)


def _other(name):
    def build(F):
        import test_hip_conv_bound as CB
        return CB.OTHER[name][0](F)
    return build


FORWARD_OTHER = {"tog3d": (4, 8, 32), "tog2d": (1, 16, 66), "yang3d": (5, 9, 33), "mres_concat_affine": (4, 8, 32), "tog_banks_max": (8, 16, 32)}


def train_target(module, name):
    """module: the gradient tests' table (model_grad_ref | model_bank_grad_ref | model_multires_grad_ref) that holds `name`"""
    import importlib
    M = importlib.import_module(module)
    c = M.case(name)
    B, Z, Y, X = c[-1]
    if module == "model_grad_ref":
        model, input_grad = M.make_model(c[1], c[2], c[3]), True
    elif module == "model_bank_grad_ref":
        model, input_grad = M.make_model(name), False          # (graph models: tfl_model_backward_input is TFL_EUNSUPPORTED)
    else:
        model, input_grad = M.make_model(c[1], c[2]), False    # (pooling / upsampling layers: likewise)
    dims = (Z, Y, X)
    big = ((Z + 4) if Z > 1 else 1, Y + 8, X + 8)              # (banks and pooling: the extents stay divisible by 4)
    inputs = {"case": M.make_inputs(name), "scene": _rough_inputs(dims, B, 181, True, 0.3), "larger": _rough_inputs(big, B, 182, True)}
    return ModelTarget(model, inputs, True, input_grad)


TRAIN_ROWS = [("model_grad_ref", "default3d-b"), ("model_grad_ref", "default2d-c"), ("model_grad_ref", "k5-skip3d"), ("model_grad_ref", "sigmoid"),
              ("model_bank_grad_ref", "mres2-concat-3d"), ("model_multires_grad_ref", "tog3d-b"), ("model_multires_grad_ref", "tog2d-b")]
NOT_SHARED = ("nan", "1e30", "leftover-scene", "leftover-larger")


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _rows():
    rows = []
    P = "test_hip_parity.py"
    site = lambda f: (("tfluids.py", f),)      # noqa: E731
    for dims, seed, split, B, tol, vel, lit in PCG_ROWS:
        for pc in ("none", "ic0", "ilu0"):
            rows.append(Row("pcg-%s-%s" % (pc, "x".join(map(str, dims))), ["tfl_solveLinearSystemPCG"], site("solveLinearSystemPCG"), [(P, "text", lit)],
                            functools.partial(pcg_target, dims, seed, split, B, tol, vel, pc)))
    # the one-launch-per-hyperplane sweeps of 3-D grids: the switch is read once per process (test_pcg_triangular_solves_both_schedules)
    rows.append(Row("pcg-ic0-9x11x13-hyperplanes", ["tfl_solveLinearSystemPCG"], site("solveLinearSystemPCG"),
                    [(P, "text", "((9, 11, 13), 4, False, 2, 1e-5)"), (P, "text", 'env["TFL_PCG_HYPERPLANES"] = "1"')],
                    functools.partial(pcg_target, (9, 11, 13), 4, False, 2, 1e-5, 2.0, "ic0"), child={"TFL_PCG_HYPERPLANES": "1"}))
    for name in MG_CASES:
        rows.append(Row("pcg-mg-" + name, ["tfl_solveLinearSystemPCG"], site("solveLinearSystemPCG"), [("pcg_mg_ref64", "key", "WIDE_CASES", name)],
                        functools.partial(mg_target, name)))
    for pc in ("mg", "none"):
        for name in ("flat", "vol"):
            rows.append(Row("pcg-batched-%s-%s" % (pc, name), ["tfl_solveLinearSystemPCGBatched"], site("solveLinearSystemPCGBatched"),
                            [("pcg_batched_cases", "key", "BATCHES", name)], functools.partial(batched_target, _mixed(name), pc)))
        rows.append(Row("pcg-batched-%s-24x36x40" % pc, ["tfl_solveLinearSystemPCGBatched"], site("solveLinearSystemPCGBatched"),
                        [("pcg_mg_ref64", "key", "WIDE_CASES", "wide2_24x36x40"), ("pcg_mg_ref64", "key", "WIDE_CASES", "wide2_24x36x40_open")],
                        functools.partial(batched_target, _wide_pair, pc)))
    for dims, seed in (((1, 30, 34), 5), ((8, 10, 16), 6)):
        rows.append(Row("normalize-" + "x".join(map(str, dims)), ["tfl_normalizePressureMean"], site("normalizePressureMean"),
                        [(P, "text", "(%r, %d, True)" % (dims, seed))], functools.partial(normalize_target, dims, seed)))
    for name in ("3d-16x24x32", "2d-ragged-33x47"):
        rows.append(Row("divnorm-" + name, ["tfl_velocityDivergenceNorm"], site("velocityDivergenceNorm"), [("divnorm_ref", "key", "CASES", name)],
                        functools.partial(divnorm_target, name)))
    for name in ("3d-16x24x32", "2d-ragged-33x47-b2"):
        for module in (False, True):
            rows.append(Row("criterion-%s%s" % (name, "-module" if module else ""), ["tfl_fluidCriterion"], site("fluidCriterion"),
                            [("criterion_ref", "key", "CASES", name)], functools.partial(criterion_target, name, module)))
    # (dims, B, seed and scene arguments as the parity test that holds the case builds it: `lit` is its parameter tuple. The
    # advection rows on (1, 24, 33) take the Jacobi table's scene of that shape; the blur's table has random fields, no scene:
    # only its shapes are shared)
    J2 = dict(vel_cells=1.0)
    V = dict(vel_cells=2.0, empty_cells=True)
    ops = [
        ("advectScalar", op_advect_scalar, ["tfl_advectScalar"], "advectScalar", (5, 13, 129), 2, 72, "((5, 13, 129), 72, 0.9, 2)", dict(vel_cells=0.9)),
        ("advectScalar", op_advect_scalar, ["tfl_advectScalar"], "advectScalar", (1, 24, 33), 2, 9, "(1, 24, 33)", J2),
        ("advectVel", op_advect_vel, ["tfl_advectVel"], "advectVel", (5, 13, 129), 2, 72, "((5, 13, 129), 72, 0.9, 2)", dict(vel_cells=0.9)),
        ("advectVel", op_advect_vel, ["tfl_advectVel"], "advectVel", (1, 24, 33), 2, 9, "(1, 24, 33)", J2),
        ("vorticityConfinement", op_vorticity, ["tfl_vorticityConfinement", "tfl_vorticityConfinementFrom"], "vorticityConfinement", (3, 8, 8), 1, 94,
         "((3, 8, 8), 94, 1)", V),
        ("vorticityConfinement", op_vorticity, ["tfl_vorticityConfinement", "tfl_vorticityConfinementFrom"], "vorticityConfinement", (20, 36, 68), 1, 91,
         "((20, 36, 68), 91, 1)", V),
        ("jacobi", op_jacobi, ["tfl_solveLinearSystemJacobi"], "solveLinearSystemJacobi", (1, 24, 33), 2, 9, "(1, 24, 33)", J2),
        ("jacobi", op_jacobi, ["tfl_solveLinearSystemJacobi"], "solveLinearSystemJacobi", (24, 20, 28), 2, 9, "(24, 20, 28)", J2),
        ("rectangularBlur", op_blur, ["tfl_rectangularBlur"], "rectangularBlur", (13, 19, 70), 2, 8, "(2, 3, 13, 19, 70)", None),
        ("rectangularBlur", op_blur, ["tfl_rectangularBlur"], "rectangularBlur", (1, 37, 131), 2, 8, "(2, 3, 1, 37, 131)", None),
    ]
    for name, op, entries, fn, dims, B, seed, lit, kw in ops:
        # (20, 36, 68) is far below the size from which tfl_vorticityConfinementFrom takes its fused kernel by itself: that row
        # runs in a child process with the fused route forced, as test_fused_vorticity_kernel_variants runs its cases
        fused = name == "vorticityConfinement" and dims == (20, 36, 68)
        rows.append(Row("%s-%s%s" % (name, "x".join(map(str, dims)), "-fused" if fused else ""), entries, site(fn),
                        [(P, "text", lit)] + ([(P, "text", '{"TFL_VORT_FUSED": "1", "TFL_VORT_PIPE": "1"}')] if fused else []),
                        functools.partial(operator_target, op, dims, B, seed, kw), child={"TFL_VORT_FUSED": "1"} if fused else None))
    rows.append(Row("vorticityConfinementItems-6x8x12", ["tfl_vorticityConfinementItems"], site("vorticityConfinementItems"),
                    [("test_hip_datagen_batched.py", "text", "((6, 8, 12), False)")], functools.partial(operator_target, op_vorticity_items, (6, 8, 12), 3, 5)))
    S = "test_hip_simulate.py"
    for which, lits in STEP_SOURCES.items():
        src = [(S, "text", lit) for lit in lits]
        if which.endswith("mg"):
            src.append(("test_hip_pcg_mg.py", "text", 'pcgPrecond="mg"'))
        rows.append(Row("step-" + which, ["tfl_simulate_step"], (("simulate.py", "simulate_native"),), src, functools.partial(step_target, which, False)))
    for which in ("2d_jacobi", "3d_pcg_mg", "3d_convnet"):
        rows.append(Row("project-" + which, ["tfl_simulate_step", "tfl_simulate_project"], (("simulate.py", "simulate_native"), ("simulate.py", "project")),
                        [(S, "text", lit) for lit in STEP_SOURCES[which]], functools.partial(step_target, which, True)))
    for pc in ("mg", "none"):
        rows.append(Row("items-2d-" + pc, ["tfl_simulate_step_items"], (("simulate.py", "_items_call"),),
                        [("datagen_batched_cases", "key", "CASES", False), ("test_hip_datagen_batched.py", "text", 'dict(simMethod="pcg", pcgPrecond="%s")' % pc)],
                        functools.partial(items_target, 0, dict(simMethod="pcg", pcgPrecond=pc), False)))
    rows.append(Row("items-3d-mg-project", ["tfl_simulate_step_items", "tfl_simulate_project_items"], (("simulate.py", "_items_call"),),
                    [("datagen_batched_cases", "key", "CASES", True), ("test_hip_datagen_batched.py", "text", 'dict(simMethod="pcg", pcgPrecond="mg")')],
                    functools.partial(items_target, 1, dict(simMethod="pcg", pcgPrecond="mg"), True)))
    SM = "test_hip_slab_methods.py"
    slab = ["tfl_simulate_step_slab", "tfl_slab_divergence_norm", "tfl_slab_drain"]
    rows.append(Row("slab-jacobi-2-ranks", slab, (), [(SM, "text", "ref = _dev(scene(9 * world + 4))"), (SM, "text", 'uneven_cuts(ref["flags"].size(2), world)'),
                                                     (SM, "text", '"maccormackOurs"]')], functools.partial(slab_target, "jacobi"), NOT_SHARED))
    rows.append(Row("slab-convnet-2-ranks", slab + ["tfl_model_begin", "tfl_model_finish"], (),
                    [(SM, "text", "ref = _dev(scene(9 * world + 4, 24, 32))"), (SM, "text", "layers = S.default_3d_layers(seed=2)"),
                     (SM, "text", 'uneven_cuts(ref["flags"].size(2), world)')], functools.partial(slab_target, "convnet"), NOT_SHARED))
    CB = "test_hip_conv_bound.py"
    fwd = ["tfl_model_forward"]
    for path in (None, "mfma", "winograd", "direct"):
        rows.append(Row("forward-default3d-%s" % (path or "mfma16"), fwd, (),
                        [(CB, "text", '((5, 9, 33), 3, "rough")'), (CB, "text", '((9, 17, 63), 1, "smooth")'), (CB, "text", '[None, "mfma", "winograd", "direct"]')],
                        functools.partial(forward_target, lambda F: F.default_3d(seed=3), path, (5, 9, 33), 3, (9, 17, 63)), NOT_SHARED))
    for path in (None, "direct"):
        rows.append(Row("forward-default2d-%s" % (path or "mfma"), fwd, (), [(CB, "text", '((1, 17, 130), 3, "rough")'), (CB, "text", '[None, "direct"]')],
                        functools.partial(forward_target, _default_2d, path, (1, 17, 130), 3, None), NOT_SHARED))
    for name, dims in FORWARD_OTHER.items():
        rows.append(Row("forward-" + name, fwd, (), [(CB, "text", '"%s": (lambda F' % name), (CB, "text", "%r),\n" % (dims,))],
                        functools.partial(forward_target, _other(name), None, dims, 3, None), NOT_SHARED))
    for module, name in TRAIN_ROWS:
        entries = ["tfl_model_forward_train", "tfl_model_backward"] + (["tfl_model_backward_input"] if module == "model_grad_ref" else [])
        rows.append(Row("train-" + name, entries, (), [(module, "key", "CASES", name)], functools.partial(train_target, module, name), NOT_SHARED))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
