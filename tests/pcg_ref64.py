"""solveLinearSystemPCG restated in fp64 (numpy only) and the case table of tests/test_pcg_ref64_cpu.py and
tests/test_hip_pcg_iterates.py.

With a tolerance that never fires, maxIter = k ends the solve after exactly k + 1 iterations (the loop is
`while (r.r > tol^2 && iter <= maxIter)`, oracle/tfluids_oracle.c:1404), in the library and in the oracle alike, and returns
x_{k+1} with the component's mean removed and ||r_{k+1}||: every iterate is visible through the public operator, and at
k = 0 the result is alpha_0 M^-1 b, one application of the preconditioner cell by cell.

solve64 follows oracle/tfluids_oracle.c:1336-1439: components in scan order of their first cell, a size-1 component skipped,
a component of fewer than 5 cells unpreconditioned, diag = number of non-obstacle neighbours, -1 to every fluid neighbour.
On this stencil IC(0) and ILU(0) touch only the diagonal (every fill-in position is outside the pattern) and are the same
operator M = (D + L) D^-1 (D + L^T) with d_i = diag_i - sum over lower fluid neighbours k of 1 / d_k, L the strictly lower
part of A. The factor and the two triangular solves run hyperplane by hyperplane (i + j + k = const: independent cells)."""
import functools

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
PRECONDS = ("none", "ilu0", "ic0")
RUNGS = (0, 1, 2, 5, 12)            # maxIter of the ladder; the deepest rung is 13 iterations
DEPTH = max(RUNGS) + 1
STOP_DEPTH = 24                     # iterations the tolerance-stop cases are followed for
# `rr > tol * tol` in fp32 never fails for a positive rr once tol * tol underflows to 0; neither the library nor the oracle
# rejects any tolerance, so the ladder uses the smallest non-negative one
TOL_NEVER = 0.0
# conditions on the reference alone (oracle against restatement), and the device bounds: twice those
CAP_P_ORACLE, CAP_RES_ORACLE = 2e-6, 1e-5
CAP_P_HIP, CAP_RES_HIP = 4e-6, 2e-5
WF_ROWS, WF_PLANES = 64, 8          # interior rows / planes of a wavefront sub-box (pcg.hip kWfRows, kWfPlanes)


def _clamp(v):                      # clampToEpsilon, oracle/tfluids_oracle.c:1206
    if abs(v) < FLT_MIN:
        return min(v, -FLT_MIN) if v < 0 else max(v, FLT_MIN)
    return v


def label_components(flags3, is3d):
    """comp [Z, Y, X] (-1: no fluid bit) numbered in scan order of each component's first cell, and their sizes"""
    fluid = (flags3.astype(np.int64) & 1) != 0
    big = fluid.size
    lab = np.where(fluid, np.arange(big).reshape(fluid.shape), big)
    axes = (0, 1, 2) if is3d else (1, 2)
    while True:
        new = lab.copy()
        for ax in axes:
            for sh in (1, -1):
                nb = np.full_like(lab, big)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[ax] = slice(0, -1) if sh == 1 else slice(1, None)
                dst[ax] = slice(1, None) if sh == 1 else slice(0, -1)
                nb[tuple(dst)] = lab[tuple(src)]
                new = np.minimum(new, nb)
        new = np.where(fluid, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[fluid])
    comp = np.full(fluid.shape, -1, np.int64)
    comp[fluid] = np.searchsorted(roots, lab[fluid])
    sizes = np.bincount(comp[fluid], minlength=len(roots)) if len(roots) else np.zeros(0, np.int64)
    return comp, sizes


class _Component:
    """one fluid component of one batch item: the matrix, the factor and the sweeps on flat grid-shaped fp64 vectors"""

    def __init__(self, flags3, comp, c, is3d, factor=True, mutate=None):
        Z, Y, X = flags3.shape
        self.is3d, self.shape = is3d, (Z, Y, X)
        self.sy, self.sz = X, X * Y
        fi = flags3.astype(np.int64)
        mask = comp == c
        kk, jj, ii = np.nonzero(mask)
        if ii.min() < 1 or ii.max() > X - 2 or jj.min() < 1 or jj.max() > Y - 2 or (is3d and (kk.min() < 1 or kk.max() > Z - 2)):
            raise ValueError("fluid cell found on the domain border")
        self.idx = np.flatnonzero(mask.ravel())
        self.offs = (1, self.sy, self.sz) if is3d else (1, self.sy)
        notobst = ((fi & 2) == 0).ravel()
        diag = np.zeros(mask.size)
        for o in self.offs:
            diag[self.idx] += notobst[self.idx - o].astype(np.float64) + notobst[self.idx + o]
        self.diag = diag
        self.mask = mask.ravel().astype(np.float64)
        h = ii + jj + kk
        order = np.argsort(h, kind="stable")
        cuts = np.flatnonzero(np.diff(h[order])) + 1
        self.levels = np.split(self.idx[order], cuts)
        # coupling weights of the sweeps (1 everywhere; a mutant drops some): low[q][n] multiplies the lower neighbour n - offs[q]
        # of cell n in the forward sweep, up[q][n] the upper neighbour n + offs[q] in the backward sweep
        self.low = [np.ones(mask.size) for _ in self.offs]
        self.up = [np.ones(mask.size) for _ in self.offs]
        if mutate == "slab_seam" and is3d:
            kgrid = np.broadcast_to(np.arange(Z)[:, None, None], (Z, Y, X)).ravel()
            self.low[2][(kgrid > 1) & ((kgrid - 1) % WF_PLANES == 0)] = 0.0         # k - 1 a multiple of 8: the neighbour k - 1 is across a seam
            self.up[2][(kgrid + 1 > 1) & (kgrid % WF_PLANES == 0)] = 0.0
        self.invd = np.zeros(mask.size)
        for lv in (self.levels if factor else ()):
            d = self.diag[lv].copy()
            for o in self.offs:
                d -= self.invd[lv - o]
            self.invd[lv] = 1.0 / d
        if mutate == "strip_d":
            jgrid = np.broadcast_to(np.arange(Y)[None, :, None], (Z, Y, X)).ravel()
            self.invd[(jgrid >= 1) & ((jgrid - 1) // WF_ROWS == 0)] /= 1.0 + 2.0 ** -10

    def apply(self, s):
        w = self.diag * s
        for o in self.offs:
            w[o:] -= s[:-o]
            w[:-o] -= s[o:]
        return w * self.mask

    def precond(self, r):
        """z = M^-1 r: (D + L) u = r, then (D + L^T) z = D u"""
        u = np.zeros_like(r)
        for lv in self.levels:
            acc = r[lv].copy()
            for q, o in enumerate(self.offs):
                acc += self.low[q][lv] * u[lv - o]
            u[lv] = acc * self.invd[lv]
        z = np.zeros_like(r)
        for lv in reversed(self.levels):
            acc = np.zeros(len(lv))
            for q, o in enumerate(self.offs):
                acc += self.up[q][lv] * z[lv + o]
            z[lv] = u[lv] + acc * self.invd[lv]
        return z


def solve64(flags, div, is3d, precond, iters, tol=None, mutate=None):
    """flags, div: [B, 1, Z, Y, X]. Returns a dict:
    p    [iters, B, 1, Z, Y, X] fp64: what the solver returns after 1 .. iters iterations (component mean removed)
    res  [iters]: the residual it returns (max over items and components of ||r||)
    comp [B, Z, Y, X]: the component of every cell (-1: no fluid bit); sizes: per item the cells of each component
    res_comp {(b, c): [iters + 1]}: ||r_0|| .. ||r_iters|| of every solved component
    tol=None: no tolerance test (only the loop's own `r.r > 0`); a number: the loop's test with that tolerance, per component.
    mutate: "slab_seam" / "strip_d": a deliberately wrong preconditioner (tests/test_pcg_ref64_cpu.py)."""
    assert precond in PRECONDS
    flags = np.asarray(flags)
    B, _, Z, Y, X = flags.shape
    tol2 = 0.0 if tol is None else float(tol) * float(tol)
    P = np.zeros((iters, B, 1, Z, Y, X))
    res = np.full(iters, -np.inf)
    comps = np.zeros((B, Z, Y, X), np.int64)
    sizes_all, res_comp = [], {}
    for b in range(B):
        comp, sizes = label_components(flags[b, 0], is3d)
        comps[b] = comp
        sizes_all.append(sizes)
        rhs_grid = np.asarray(div[b, 0], np.float64).ravel()
        for c, size in enumerate(sizes):
            if size == 1:
                continue
            pc = precond != "none" and size >= 5
            C = _Component(flags[b, 0], comp, c, is3d, factor=pc, mutate=mutate if pc else None)
            x = np.zeros(rhs_grid.size)
            r = rhs_grid * C.mask
            rr1, rr0, prev_num = float(r @ r), 0.0, 0.0
            s = z = None
            hist = [np.sqrt(rr1)]
            for it in range(1, iters + 1):
                if rr1 > tol2:
                    if pc:
                        z = C.precond(r)
                    if it == 1:
                        s = (z if pc else r).copy()
                    elif pc:
                        s = (float(r @ z) / _clamp(prev_num)) * s + z
                    else:
                        s = (rr1 / _clamp(rr0)) * s + r
                    w = C.apply(s)
                    num = float(r @ z) if pc else rr1
                    alpha = num / _clamp(float(s @ w))
                    x = alpha * s + x
                    prev_num = num
                    r = -alpha * w + r
                    rr0, rr1 = rr1, float(r @ r)
                hist.append(np.sqrt(rr1))
                P[it - 1, b, 0].ravel()[C.idx] = x[C.idx] - x[C.idx].sum() / size
                res[it - 1] = max(res[it - 1], np.sqrt(rr1))
            res_comp[(b, c)] = np.array(hist)
    return dict(p=P, res=res, comp=comps, sizes=sizes_all, res_comp=res_comp)


# ---- the cases ----------------------------------------------------------------------------------------------------------
# the smallest grids that reach each piece of the device schedule: wavefront sub-boxes are 64 interior rows x 8 interior planes
# x all of x and run NT steps, (X - 2) + 63 + 2 * 7 rounded up to a multiple of 16 (pcg.hip wf_geom)
CASES = {
    # one partial sub-box. (Not (6, 9, 7): on its 136 cells preconditioned CG is below eps32 ||b|| after 13 iterations, where the
    # oracle's own recursively updated residual is rounding noise, 5e-3 relative, and the condition on the reference cannot hold.)
    "partial_9x11x13": dict(dims=(9, 11, 13), seed=31),
    "one_box_10x66x5": dict(dims=(10, 66, 5), seed=32),                                  # exactly one full sub-box, NT = 80 unpadded
    "seams_11x67x6": dict(dims=(11, 67, 6), seed=33, split=True, empty_patch=True),      # 2 x 2 sub-boxes, second strip / slab 1 wide
    "inner_19x131x8": dict(dims=(19, 131, 8), seed=46, split=True),                      # 3 strips x 3 slabs: an interior sub-box
    "batch_12x20x24": dict(dims=(12, 20, 24), seed=35, B=2, item_wall=True),             # per-item geometry, label / z reuse
    "flat_24x28": dict(dims=(1, 24, 28), seed=36),                                       # 2-D: hyperplane sweeps, 5-point pattern
    "flat_70x9": dict(dims=(1, 70, 9), seed=37, split=True),
    "pockets_9x14x12": dict(dims=(9, 14, 12), seed=38, pockets=True),                    # walled pockets of 2, 3, 4 cells
    "pockets_flat_20x22": dict(dims=(1, 20, 22), seed=39, pockets=True),
}
# the cases the TFL_WF_MAX_BLOCKS=4 schedule runs: slabs per launch = 4 / strips, so inner_19x131x8 (3 strips) runs one slab per
# launch, three launches a sweep; seams_11x67x6 (2 strips x 2 slabs) still fits one launch and runs as in the default schedule
CHUNK_CASES = ("inner_19x131x8", "seams_11x67x6")
# tolerance stops inside a queued chunk: (case, preconditioner, schedule, iterations the host queues per sync)
STOP_CASES = (("one_box_10x66x5", "ic0", "default", 16), ("one_box_10x66x5", "ilu0", "hyperplanes", 4),
              ("partial_9x11x13", "none", "default", 32))


def _add_pockets(f, is3d):
    """walled pockets of 2, 3 and 4 fluid cells in the corner of the domain near the origin (an obstacle block with the
    pocket's cells carved out of it), beside the large component. Each pocket has one empty cell in its wall: a pocket
    walled all round has a singular matrix, and with a tolerance that never fires the oracle itself breaks down on it within
    the first rungs (s.A s = 0 once r is the constant vector, alpha = r.r / FLT_MIN: an iterate off by O(1), then NaN)."""
    B, _, Z, Y, X = f.shape
    ks = slice(1, 4) if is3d else slice(0, 1)
    k = 2 if is3d else 0
    f[:, :, ks, 1:8, 1:10] = 2.0
    f[:, :, k, 2, 2:4] = 1.0                    # 2 cells along x
    f[:, :, k, 4:7, 2] = 1.0                    # 3 cells along y
    f[:, :, k, 4:6, 5:7] = 1.0                  # 4 cells, a square
    f[:, :, k, 2, 6] = 1.0                      # and a size-1 component
    for j, i in ((2, 4), (5, 3), (6, 6)):       # the empty cells: next to one cell of a pocket, obstacles on their other sides
        f[:, :, k, j, i] = 4.0


def build_case(tf, name):
    """(flags, div, is3d) of a case; tf = any object with setWallBcsForward / velocityDivergenceForward (the oracle)"""
    import scenes
    c = CASES[name]
    kw = {k: c[k] for k in ("B",) if k in c}
    sc, f, U, div = scenes.pcg_problem(tf, c["dims"], c["seed"], vel_cells=2.0, split=c.get("split", False), **kw)
    is3d = sc["is3d"]
    if c.get("pockets") or c.get("item_wall") or c.get("empty_patch"):
        if c.get("empty_patch"):                # a few empty cells (a Dirichlet condition for their neighbours) in either component
            patch = f[:, :, 2:4, 30:33, 1:-1]
            patch[patch == 1.0] = 4.0
        if c.get("pockets"):
            _add_pockets(f, is3d)
        if c.get("item_wall"):                  # item 1 alone gets a wall across y: two large components there, one in item 0
            Y = f.shape[3]
            f[1, :, :, Y // 2, :] = 2.0
        U = sc["U"].copy()
        tf.setWallBcsForward(U, f)
        div = np.zeros_like(sc["p"])
        tf.velocityDivergenceForward(U, f, div)
    return np.ascontiguousarray(f), np.ascontiguousarray(div), is3d


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import OracleTfluids
    return OracleTfluids()


@functools.lru_cache(maxsize=None)
def case(name):
    f, div, is3d = build_case(_oracle(), name)
    for a in (f, div):
        a.setflags(write=False)
    return f, div, is3d


@functools.lru_cache(maxsize=None)
def reference(name, precond, depth=DEPTH):
    """solve64 of a case to `depth` iterations, computed once per process and shared (read-only)"""
    f, div, is3d = case(name)
    out = solve64(f, div, is3d, precond, depth)
    for k in ("p", "res", "comp"):
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_ladder(name, precond):
    """{rung: (p, residual)} of the fp32 oracle"""
    f, div, is3d = case(name)
    out = {}
    for k in RUNGS:
        p = np.zeros_like(div)
        r = _oracle().solveLinearSystemPCG(p, f, div, is3d, TOL_NEVER, k, precond)
        p.setflags(write=False)
        out[k] = (p, r)
    return out


def solved_mask(ref):
    """cells of components the solver solves (size > 1)"""
    m = np.zeros(ref["comp"].shape, bool)
    for b, sizes in enumerate(ref["sizes"]):
        for c, size in enumerate(sizes):
            if size > 1:
                m[b] |= ref["comp"][b] == c
    return m[:, None]


def worst_error(p, p64, ref):
    """max over solved components of max|p - p64| / max|p64| (both over the component's cells); and the exact-zero check of
    every other cell"""
    worst = 0.0
    p = np.asarray(p)
    for b, sizes in enumerate(ref["sizes"]):
        for c, size in enumerate(sizes):
            if size == 1:
                continue
            m = ref["comp"][b] == c
            scale = np.abs(p64[b, 0][m]).max()
            worst = max(worst, float(np.abs(p[b, 0][m] - p64[b, 0][m]).max() / scale))
    untouched_zero = bool(np.all(p[~solved_mask(ref)] == 0.0))
    return worst, untouched_zero


def pick_stop(hist, chunk, lo=5, hi=STOP_DEPTH - 2):
    """the iteration k of a tolerance stop: the smallest k >= lo with neither k nor k + 1 a multiple of the chunk,
    ||r_k|| >= 1.5 ||r_{k+1}||, and every ||r_m||, m <= k, at least sqrt(1.5) times the tolerance (the margin ||r_k|| itself
    has). Returns (k, tol = geometric mean of ||r_k|| and ||r_{k+1}||): the solve ends at iterate k + 1."""
    for k in range(lo, hi):
        tol = float(np.sqrt(hist[k] * hist[k + 1]))
        if k % chunk and (k + 1) % chunk and hist[k] >= 1.5 * hist[k + 1] and hist[:k + 1].min() >= np.sqrt(1.5) * tol:
            return k, tol
    raise AssertionError("no well-posed tolerance stop in %r" % (hist,))
