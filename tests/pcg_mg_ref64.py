"""The multigrid preconditioner of solveLinearSystemPCG (precondType = "mg", fluidnet_amd/csrc/pcg_mg.hip) restated in numpy,
in fp64 or fp32 by argument, inside the component loop and the CG recurrence of tests/pcg_ref64.py (components in scan order,
a size-1 component skipped, fewer than 5 cells unpreconditioned, the clampToEpsilon guards, the loop test, the mean removal).

The scheme (fluidnet_amd/csrc/tfl_pcg_mg.hpp states it too; the constants below mirror that header): one symmetric V-cycle of
aggregation multigrid per CG iteration, for one fluid component.
  level 0   diag = number of non-obstacle neighbours on the component, coupling 1 to every face neighbour in the component,
            kept as one plus-face coupling per axis;
  coarser   2x per pooled axis (y, x in 2-D; z, y, x in 3-D), extent = ceil(fine / 2), a coarse cell active if any child is;
            the exact Galerkin product of piecewise-constant P: diag_c = sum of the children's diag - 2 * the couplings inside
            the aggregate, plus-face coupling = sum of the children's couplings across that face; 1 / diag taken as 0 where diag = 0;
  levels    coarsen while every pooled axis is longer than COARSEST, at most MAX_LEVELS levels;
  cycle     from z = 0: NU damped-Jacobi sweeps (weight OMEGA; the first is z = OMEGA r / diag), r_c = P^T (r - A z) summed over
            the children, recurse, z += ALPHA P z_c on active cells, NU sweeps; NU_C sweeps from 0 on the coarsest level;
  closed    a component none of whose cells has an empty neighbour has a singular matrix (null space: the constants). Its cycle
            runs on r minus the mean of r over the component (the mean in fp64, rounded to the format): the identity on the
            range of A, where CG's r lives but for rounding, and what keeps that rounding residue from being amplified by a
            preconditioner that approximates the inverse of a singular matrix well. MgComponent.cycle is the bare V-cycle.

As in tests/pcg_ref64.py, a tolerance that never fires makes maxIter = k return iterate k + 1: the ladder RUNGS.

The iterate bound C_ITERATE. The device forms the same quantities in fp32 with its dot products in fp64, in another order. What
fp32 costs is measured on the restatement itself: solve(dtype=float32) (vectors, the hierarchy and alpha / beta in fp32, dot
products accumulated in fp64 as on the device) against solve(dtype=float64) on CASES at RUNGS, worst cell per component relative
to max|p64| of the component. The largest ratio is 7.19e-7 (flat_split_30x34, rung 1; per case and rung in profiles/pcg_mg.md);
C_ITERATE is 4 x that, rounded up to two digits (2.9e-6): the margin covers the device's different order in the reductions that feed
alpha. The mutants of MUTANTS move the first rung by more than 100 x C_ITERATE (tests/test_pcg_mg_ref_cpu.py).

WIDE_CASES (below) are the grids on which the device runs coarse levels one launch per operation; they have bounds of their own,
one per rung, by the same rule, and mutants that live on one coarse level (LEVEL_MUTANTS)."""
import functools

import numpy as np

import pcg_ref64 as R

OMEGA, NU, NU_C, ALPHA = 0.8, 2, 8, 1.6           # kMgOmega, kMgNu, kMgNuCoarse, kMgAlpha
COARSEST, MAX_LEVELS = 4, 10                      # kMgCoarsestExtent, kMgMaxLevels
RUNGS = (0, 1, 3)
DEPTH = max(RUNGS) + 1
FP32_WORST = 7.19e-7                              # measured: fp32 restatement against fp64 restatement, see the docstring
C_ITERATE = 2.9e-6                                # 4 x FP32_WORST
C_RESIDUAL = 2e-5                                 # the returned residual, relative: tests/pcg_ref64.py CAP_RES_HIP
MUTANTS = ("no_post_smoothing", "galerkin_drops_a_coupling", "restrict_mean")

# dims, seed and extras of scenes.pcg_problem
CASES = {
    "flat_24x28": dict(dims=(1, 24, 28), seed=3),
    "flat_split_30x34": dict(dims=(1, 30, 34), seed=5, split=True),
    "flat_odd_33x47": dict(dims=(1, 33, 47), seed=7),
    "batch_9x11x13": dict(dims=(9, 11, 13), seed=4, B=2, item_wall=True),
    "split_8x10x16": dict(dims=(8, 10, 16), seed=6, split=True),
    "odd_12x17x20": dict(dims=(12, 17, 20), seed=8),
}
# "mg takes at most half of ic0's iterations" is a condition on the inputs. split_8x10x16 has 593 fluid cells in two components of
# 305 and 287: systems that small leave 'ic0' too few iterations to halve (19 against 33 in fp64), so that test alone takes the
# same scene one size up in its place.
EXTRA_CASES = {"split_10x14x20": dict(dims=(10, 14, 20), seed=6, split=True)}
RATIO_CASES = tuple(n for n in sorted(CASES) if n != "split_8x10x16") + ("split_10x14x20",)


# ---- the levels that run one launch per operation ----------------------------------------------------------------------------
# Levels of more than BLOCK_CELLS cells run one launch per operation (k_mg_restrict / k_mg_first / k_mg_sweep), all smaller ones
# inside one launch of k_mg_coarse; the host picks from the grid size alone. In every case of CASES level 1 has at most 17 x 24
# cells: level 0 is the only level that runs as launches. WIDE_SHAPES are the smallest grids that reach the other schedules;
# `levels` = (level count, first level k_mg_coarse owns: == count when it owns none), held by tests/test_pcg_mg_ref_cpu.py.
# Each shape is a case twice, closed (the box as scenes.pcg_problem builds it: the mean of r removed, k_mg_rsum / k_mg_first0) and
# open (NAME_open: pcg_batched_cases.open_patch, the cycle straight from CG's r with k_mg_first).
BLOCK_CELLS = 4096                                # kMgBlockCells
WIDE_SHAPES = {
    # level 1 = 66 x 68 as launches. (Not seed 11: its obstacles wall off a closed pocket of two cells, which CG solves exactly in
    # one iteration -- r = 0 in any precision -- so that the solve does not run k + 1 iterations on every component.)
    "wide2_flat_132x136": dict(dims=(1, 132, 136), seed=19, split=True, levels=(7, 2)),
    # levels 1 (130 x 132) and 2 (65 x 66 = 4290) as launches: prolongation launch to launch, a stacked offset > 0
    "wide3_flat_260x264": dict(dims=(1, 260, 264), seed=12, levels=(8, 3)),
    "wide3_flat_odd_259x263": dict(dims=(1, 259, 263), seed=13, levels=(8, 3)),           # 259 x 263, 130 x 132, 65 x 66: odd
    "wide2_24x36x40": dict(dims=(24, 36, 40), seed=14, split=True, levels=(4, 2)),        # level 1 = 12 x 18 x 20 = 4320
    "thin_flat_8x2100": dict(dims=(1, 8, 2100), seed=15, levels=(2, 2)),                  # no level for k_mg_coarse: the coarsest
    "thin_6x6x1000": dict(dims=(6, 6, 1000), seed=16, levels=(2, 2)),                     # level's sweeps as launches
    "one_level_flat_4x60": dict(dims=(1, 4, 60), seed=17, levels=(1, 1)),                 # NU_C sweeps of level 0, nothing else
    "one_level_4x12x14": dict(dims=(4, 12, 14), seed=18, levels=(1, 1)),
}
WIDE_CASES = {}
for _n, _c in WIDE_SHAPES.items():
    WIDE_CASES[_n] = {k: v for k, v in _c.items() if k != "levels"}
    WIDE_CASES[_n + "_open"] = dict(WIDE_CASES[_n], open=True)
COUNT_CASES = tuple(n for n in sorted(WIDE_CASES) if n.startswith(("wide", "thin")))       # iteration counts at COUNT_TOL
COUNT_TOL = 1e-4
# The bounds of the device test on WIDE_CASES, one per rung, by C_ITERATE's rule: 4 x the worst fp32-restatement-against-fp64-
# restatement ratio over WIDE_CASES at that rung (worst cell per component relative to max|p64| of the component), rounded up to
# two digits. Per case and rung: profiles/pcg_mg.md. tests/test_pcg_mg_ref_cpu.py pins each constant to the measurement.
FP32_WORST_WIDE = {0: 5.327e-7, 1: 3.177e-6, 3: 6.585e-6}       # measured, by rung: wide3_flat_260x264 at each
C_ITERATE_WIDE = {0: 2.2e-6, 1: 1.3e-5, 3: 2.7e-5}
# The returned residual: C_RESIDUAL at the rungs where the fp32 restatement stays under C_RESIDUAL / 2 on every case of WIDE_CASES
# (rungs 0 and 1), elsewhere 4 x the fp32 restatement's worst relative error at that rung, rounded up to two digits (rung 3:
# 1.452e-5 on one_level_flat_4x60_open, whose residual has fallen from 2.1 to 1.7e-3 by then; 1.17e-5 on wide3_flat_260x264).
FP32_RES_WIDE = {0: 4.824e-7, 1: 2.081e-6, 3: 1.452e-5}
C_RESIDUAL_WIDE = {0: C_RESIDUAL, 1: C_RESIDUAL, 3: 5.9e-5}


def four_times_rounded_up(worst):
    """4 x worst rounded up to two significant digits: the rule C_ITERATE and the bounds of WIDE_CASES follow"""
    import decimal
    d = decimal.Decimal(repr(4.0 * worst))
    return float(d.quantize(decimal.Decimal((0, (1,), d.adjusted() - 1)), rounding=decimal.ROUND_CEILING))


# Mutants local to one coarse level (the three of MUTANTS change every level at once). One that names a level a case does not
# have is the identity there: mutant_applies.
LEVEL_MUTANTS = ("coarsest_one_sweep_short", "alpha_one_into_level1", "level1_one_post_sweep", "level2_one_post_sweep")


def mutant_applies(mutant, count):
    """whether a mutant of LEVEL_MUTANTS changes the cycle of a hierarchy of `count` levels"""
    # a prolongation into level l, and post-smoothing on it, exist when level l is not the last one
    return {"coarsest_one_sweep_short": True, "alpha_one_into_level1": count >= 3, "level1_one_post_sweep": count >= 3,
            "level2_one_post_sweep": count >= 4}[mutant]


def mg_levels(Z, Y, X, is3d):
    """[(Z, Y, X)] per level, level 0 first (tfl_pcg_mg.hpp mg_levels)"""
    lv = [(Z, Y, X)]
    while len(lv) < MAX_LEVELS:
        z, y, x = lv[-1]
        if x <= COARSEST or y <= COARSEST or (is3d and z <= COARSEST):
            break
        lv.append(((z + 1) // 2 if is3d else z, (y + 1) // 2, (x + 1) // 2))
    return lv


def first_block_level(levels):
    """the first level k_mg_coarse owns (tfl_pcg_mg.hpp MgLevels::first_block_level): >= 1, == len(levels) when it owns none"""
    fb = len(levels)
    for l in range(len(levels) - 1, 0, -1):
        if levels[l][0] * levels[l][1] * levels[l][2] > BLOCK_CELLS:
            break
        fb = l
    return fb


def _blocks(a, cshape, is3d):
    """a fine array padded with zeros to twice the coarse extents and viewed as [Zc, fz, Yc, 2, Xc, 2] (fz = 2 in 3-D, else 1)"""
    Zc, Yc, Xc = cshape
    fz = 2 if is3d else 1
    pad = np.zeros((Zc * fz, Yc * 2, Xc * 2), a.dtype)
    pad[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return pad.reshape(Zc, fz, Yc, 2, Xc, 2)


class _Level:
    pass


class MgComponent(R._Component):
    """A component with the multigrid hierarchy as its preconditioner. dtype: the number format of the hierarchy and the cycle."""

    def __init__(self, flags3, comp, c, is3d, dtype=np.float64, mutate=None):
        super().__init__(flags3, comp, c, is3d, factor=False)
        self.dtype, self.mutate = dtype, mutate
        Z, Y, X = self.shape
        act = (comp == c)
        lv = _Level()
        lv.active = act
        lv.diag = (self.diag.reshape(Z, Y, X) * act).astype(dtype)
        lv.c = []                                    # plus-face couplings along x, y[, z]: axis 2, 1[, 0]
        for ax in ((2, 1, 0) if is3d else (2, 1)):
            cc = np.zeros((Z, Y, X), dtype)
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            cc[tuple(lo)] = (act[tuple(lo)] & act[tuple(hi)]).astype(dtype)
            lv.c.append((ax, cc))
        self.lv = [lv]
        for cshape in mg_levels(Z, Y, X, is3d)[1:]:
            self.lv.append(self._coarsen(self.lv[-1], cshape))
        # closed: every non-obstacle neighbour of every cell is in the component (row sums of A are zero)
        self.closed = float(self.lv[0].diag.sum(dtype=np.float64)) == 2.0 * sum(float(cc.sum(dtype=np.float64)) for _, cc in self.lv[0].c)
        for lv in self.lv:
            with np.errstate(divide="ignore"):
                lv.invd = np.where(lv.diag > 0, dtype(1) / lv.diag, dtype(0)).astype(dtype)

    def _coarsen(self, f, cshape):
        is3d, dtype = self.is3d, self.dtype
        c = _Level()
        c.active = _blocks(f.active, cshape, is3d).any(axis=(1, 3, 5))
        diag = _blocks(f.diag, cshape, is3d).sum(axis=(1, 3, 5), dtype=dtype)
        c.c = []
        for ax, cc in f.c:
            blk = _blocks(cc, cshape, is3d)
            sub = {2: 5, 1: 3, 0: 1}[ax]             # the [.., 2] axis of the blocks that runs along `ax`
            inner = np.take(blk, 0, axis=sub)        # children on the lower side: their plus face is inside the aggregate
            cross = np.take(blk, 1, axis=sub)
            # after np.take the array is [Zc, fz, Yc, 2, Xc] / [Zc, fz, Yc, Xc, 2] / [Zc, Yc, 2, Xc, 2]: sum the block axes left
            red = {2: (1, 3), 1: (1, 4), 0: (2, 4)}[ax]
            if self.mutate == "galerkin_drops_a_coupling" and ax == 2:
                cross = cross.copy()
                cross[:, :, :, 1] = 0                # x-crossing coupling of the children in the upper y row left out
            diag = diag - 2 * inner.sum(axis=red, dtype=dtype)
            c.c.append((ax, cross.sum(axis=red, dtype=dtype).astype(dtype)))
        c.diag = diag.astype(dtype)
        return c

    @staticmethod
    def _apply(lv, z):
        w = lv.diag * z
        for ax, cc in lv.c:
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            w[lo] -= cc[lo] * z[hi]
            w[hi] -= cc[lo] * z[lo]
        return w

    def _smooth(self, lv, r, z, sweeps):
        om = self.dtype(OMEGA)
        for _ in range(sweeps):
            z = (om * lv.invd * r) if z is None else z + om * lv.invd * (r - self._apply(lv, z))
        return z

    def _cycle(self, l, r):
        lv = self.lv[l]
        if l == len(self.lv) - 1:
            return self._smooth(lv, r, None, NU_C - 1 if self.mutate == "coarsest_one_sweep_short" else NU_C)
        z = self._smooth(lv, r, None, NU)
        cl = self.lv[l + 1]
        res = _blocks(r - self._apply(lv, z), cl.diag.shape, self.is3d)
        rc = res.sum(axis=(1, 3, 5), dtype=self.dtype)
        if self.mutate == "restrict_mean":
            cnt = _blocks(lv.active.astype(self.dtype), cl.diag.shape, self.is3d).sum(axis=(1, 3, 5))
            rc = rc / np.maximum(cnt, 1)
        zc = self._cycle(l + 1, rc.astype(self.dtype))
        up = zc
        for ax in ((0, 1, 2) if self.is3d else (1, 2)):
            up = np.repeat(up, 2, axis=ax)
        up = up[:z.shape[0], :z.shape[1], :z.shape[2]]
        alpha = 1.0 if (self.mutate == "alpha_one_into_level1" and l == 1) else ALPHA
        z = z + self.dtype(alpha) * up * lv.active
        if self.mutate == "no_post_smoothing":
            return z
        short = self.mutate == "level%d_one_post_sweep" % l and l >= 1
        return self._smooth(lv, r, z, NU - 1 if short else NU)

    def cycle(self, r):
        """the bare V-cycle on flat grid-shaped vectors"""
        return self._cycle(0, np.asarray(r, self.dtype).reshape(self.shape)).ravel()

    def precond(self, r):
        """z = M^-1 r on flat grid-shaped vectors: the V-cycle, on a closed component of r minus its mean"""
        r = np.asarray(r, self.dtype).reshape(self.shape)
        if self.closed:
            act = self.lv[0].active
            r = r - self.dtype(r.sum(dtype=np.float64) / act.sum()) * act
        return self._cycle(0, r.astype(self.dtype)).ravel()


def solve(flags, div, is3d, precond, iters, tol=None, mutate=None, dtype=np.float64, max_iter=None):
    """tests/pcg_ref64.py solve64 with "mg" as a fourth preconditioner and the number format as an argument: with
    dtype=float32 vectors, alpha and beta are fp32 and dot products are accumulated in fp64, as on the device.
    Returns solve64's dict plus iters_comp {(b, c): iterations run} and iterations = their sum (tfl_pcg_last_iterations).
    max_iter: the loop's `iter <= maxIter` test (None: not applied)."""
    assert precond in R.PRECONDS + ("mg",)
    flags = np.asarray(flags)
    B, _, Z, Y, X = flags.shape
    tol2 = 0.0 if tol is None else float(np.float32(tol) * np.float32(tol))
    P = np.zeros((iters, B, 1, Z, Y, X))
    res = np.full(iters, -np.inf)
    comps = np.zeros((B, Z, Y, X), np.int64)
    sizes_all, res_comp, iters_comp = [], {}, {}
    dot = lambda a, b: float(np.dot(a.astype(np.float64), b.astype(np.float64)))
    for b in range(B):
        comp, sizes = R.label_components(flags[b, 0], is3d)
        comps[b] = comp
        sizes_all.append(sizes)
        rhs_grid = np.asarray(div[b, 0], dtype).ravel()
        for c, size in enumerate(sizes):
            if size == 1:
                continue
            pc = precond != "none" and size >= 5
            if pc and precond == "mg":
                C = MgComponent(flags[b, 0], comp, c, is3d, dtype, mutate)
            else:
                C = R._Component(flags[b, 0], comp, c, is3d, factor=pc)
            mask = C.mask.astype(dtype)
            x = np.zeros(rhs_grid.size, dtype)
            r = rhs_grid * mask
            rr1, rr0, prev_num = dot(r, r), 0.0, 0.0
            s = z = None
            hist, n_it = [np.sqrt(rr1)], 0
            for it in range(1, iters + 1):
                if rr1 > tol2 and (max_iter is None or n_it <= max_iter):
                    n_it += 1
                    if pc:
                        z = C.precond(r).astype(dtype)
                    num = dot(r, z) if pc else rr1
                    if it == 1:
                        s = (z if pc else r).copy()
                    else:
                        beta = dtype(dtype(num) / dtype(R._clamp(float(dtype(prev_num if pc else rr0)))))
                        s = beta * s + (z if pc else r)
                    w = (C.apply(s.astype(np.float64)) if dtype is np.float64 else _apply32(C, s)).astype(dtype)
                    alpha = dtype(dtype(num) / dtype(R._clamp(float(dtype(dot(s, w))))))
                    x = alpha * s + x
                    prev_num = num
                    r = -alpha * w + r
                    rr0, rr1 = rr1, dot(r, r)
                hist.append(np.sqrt(rr1))
                xs = x[C.idx].astype(np.float64)
                P[it - 1, b, 0].ravel()[C.idx] = (x[C.idx] - dtype(xs.sum() / size)) if dtype is not np.float64 else xs - xs.sum() / size
                res[it - 1] = max(res[it - 1], np.sqrt(rr1))
            res_comp[(b, c)] = np.array(hist)
            iters_comp[(b, c)] = n_it
    return dict(p=P, res=res, comp=comps, sizes=sizes_all, res_comp=res_comp, iters_comp=iters_comp,
                iterations=sum(iters_comp.values()))


def _apply32(C, s):
    w = C.diag.astype(np.float32) * s
    off = np.zeros_like(s)
    for o in C.offs:
        off[o:] += s[:-o]
        off[:-o] += s[o:]
    return (w - off) * C.mask.astype(np.float32)


def iterations_to(flags, div, is3d, precond, tol, max_iter=1000, dtype=np.float64):
    """iterations the solve takes to ||r|| <= tol, summed over the components (what tfl_pcg_last_iterations returns)"""
    return solve(flags, div, is3d, precond, max_iter + 1, tol=tol, dtype=dtype, max_iter=max_iter)["iterations"]


# ---- the cases ----------------------------------------------------------------------------------------------------------
def build_case(tf, name):
    """(flags, div, is3d); tf = any object with setWallBcsForward / velocityDivergenceForward (the oracle)"""
    import scenes
    from pcg_batched_cases import open_patch
    c = next(t[name] for t in (CASES, EXTRA_CASES, WIDE_CASES) if name in t)
    kw = {k: c[k] for k in ("B",) if k in c}
    sc, f, U, div = scenes.pcg_problem(tf, c["dims"], c["seed"], vel_cells=2.0, split=c.get("split", False), **kw)
    if c.get("item_wall") or c.get("open"):
        if c.get("item_wall"):                  # item 1 alone gets a wall across y: other flags per item, two large components
            f[1, :, :, f.shape[3] // 2, :] = 2.0
        if c.get("open"):                       # a patch of empty cells: the component around it is open
            open_patch(f, c["dims"], sc["is3d"])
        U = sc["U"].copy()
        tf.setWallBcsForward(U, f)
        div = np.zeros_like(sc["p"])
        tf.velocityDivergenceForward(U, f, div)
    return np.ascontiguousarray(f), np.ascontiguousarray(div), sc["is3d"]


@functools.lru_cache(maxsize=None)
def case(name):
    f, div, is3d = build_case(R._oracle(), name)
    for a in (f, div):
        a.setflags(write=False)
    return f, div, is3d


def cells(name):
    """fluid cells of a case's largest item"""
    f, _, _ = case(name)
    return int(((f.astype(np.int64) & 1) != 0).reshape(f.shape[0], -1).sum(axis=1).max())


@functools.lru_cache(maxsize=None)
def reference(name, precond="mg", depth=DEPTH, mutate=None, fp32=False):
    """solve() of a case with a tolerance that never fires, computed once per process and shared (read-only)"""
    f, div, is3d = case(name)
    out = solve(f, div, is3d, precond, depth, mutate=mutate, dtype=np.float32 if fp32 else np.float64)
    for k in ("p", "res", "comp"):
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def iterations(name, precond, tol=1e-5):
    f, div, is3d = case(name)
    return iterations_to(f, div, is3d, precond, tol)
