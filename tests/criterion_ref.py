"""Helper of tests/test_criterion_cpu.py and tests/test_hip_criterion.py: the cases of the fused criterion
(tfl_criterion_weight, tfl_fluidCriterion) and a numpy restatement of it, fp32 operation by operation in the order
include/tfluids_hip.h documents (one rounding per operation: numpy float32 arrays never contract).

The three tfluids pieces -- signedDistanceField, velocityDivergenceForward, velocityDivergenceBackward -- come from the CPU
checker handed in (`tf`: the C restatement of the reference, or the compiled reference itself; tests/test_criterion_cpu.py
holds the two equal on these cases). The loss sums are math.fsum over float64 squares (exact, rounded once). The MSE
arithmetic of the reference lives in Torch7's nn / THNN, outside the reference tree: that order is this library's."""
import functools
import math

import numpy as np

import scenes

F = np.float32

# (name, dims (Z, Y, X), B, how the device tensors are laid out): the smallest shapes that reach each kernel form
CASES = [
    ("3d-16x24x32", (16, 24, 32), 1, "aligned"),
    ("3d-ragged-13x17x23-b2", (13, 17, 23), 2, "aligned"),       # X % 4 != 0: the one-cell-per-thread form
    ("3d-short-row-8x12x16-b2", (8, 12, 16), 2, "aligned"),      # 8-lane row segments
    ("3d-wide-row-6x10x160", (6, 10, 160), 1, "aligned"),        # wider than one 32-lane segment: the memory taps at a segment end
    ("2d-64x96-b2", (1, 64, 96), 2, "aligned"),
    ("2d-ragged-33x47-b2", (1, 33, 47), 2, "aligned"),
    ("3d-misaligned-view", (16, 24, 32), 1, "misaligned"),       # sliced one float off a 16-byte boundary
    ("2d-misaligned-view", (1, 64, 96), 2, "misaligned"),
]
NAMES = [c[0] for c in CASES]
BORDER = (2.0, 3)                       # (borderWeight, borderWidth) of the weighted runs
LAMBDAS = {"all": (0.7, 1.3, 2.5), "p-off": (0.0, 1.3, 2.5), "u-off": (0.7, 0.0, 2.5), "div-off": (0.7, 1.3, 0.0)}
LOSS_REL = 1e-10                        # a non-negative fp64 sum of n <= 1e5 terms errs by at most (n - 1) 2^-53 ~ 1.1e-11 relative


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(pPred, UPred, pTarget, UTarget, flags): a scene with obstacles inside the walls and velocities of 0.4 cells per step;
    the targets are a second seeded scene's fields on the same flags"""
    i = NAMES.index(name)
    _, dims, B, _ = CASES[i]
    a = scenes.make_scene(dims, seed=60 + i, B=B, vel_cells=0.4)
    b = scenes.make_scene(dims, seed=160 + i, B=B, vel_cells=0.4)
    out = (a["p"], a["U"], b["p"], b["U"], a["flags"])
    for t in out:
        t.setflags(write=False)
    return out


def weight(tf, flags, borderWeight, borderWidth):
    """fluid_criterion.lua:145-158, one fp32 rounding per Lua call"""
    sdf = np.zeros_like(flags)
    tf.signedDistanceField(np.ascontiguousarray(flags), int(borderWidth), flags.shape[2] > 1, sdf)
    c = np.minimum(np.maximum(sdf, F(1)), F(borderWidth))
    c = c + F(-1)
    c = c * F(-1.0 / (borderWidth - 1))
    c = c + F(1)
    c = c * F(borderWeight - 1)
    return c + F(1)


def _sumsq(z):
    z = z.astype(np.float64).ravel()
    return math.fsum(z * z)


def criterion(tf, pP, UP, pT, UT, flags, w, lambdas, sizeAverage=True):
    """dict(loss = [pLoss, uLoss, divLoss, total] as Python floats, gradP, gradU)"""
    pl, ul, dl = lambdas
    n_p, n_u = pP.size, UP.size
    assert all(t.dtype == F for t in (pP, UP, pT, UT, flags)) and (w is None or w.dtype == F)
    flags = np.ascontiguousarray(flags)
    UP = np.ascontiguousarray(UP)
    zp = (w * pP - w * pT) if w is not None else (pP - pT)
    zu = (w * UP - w * UT) if w is not None else (UP - UT)          # w [B,1,Z,Y,X] broadcasts over the channels
    div = np.zeros_like(flags)
    tf.velocityDivergenceForward(UP, flags, div)
    zd = (w * div) if w is not None else div
    avg = (lambda s, n: s / n) if sizeAverage else (lambda s, n: s)
    lp = pl * avg(_sumsq(zp), n_p) if pl > 0 else 0.0
    lu = ul * avg(_sumsq(zu), n_u) if ul > 0 else 0.0
    ld = dl * avg(_sumsq(zd), n_p) if dl > 0 else 0.0
    normP = F(2.0 / n_p) if sizeAverage else F(2)
    normU = F(2.0 / n_u) if sizeAverage else F(2)

    def grad(norm, z, lam):
        g = norm * z
        if w is not None:
            g = g * w
        return g * F(lam)
    gradP = grad(normP, zp, pl) if pl > 0 else np.zeros_like(pP)
    gradU = np.zeros_like(UP)
    if ul > 0:
        gradU = gradU + grad(normU, zu, ul)
    if dl > 0:
        go = np.ascontiguousarray(grad(normP, zd, dl))
        dU = np.zeros_like(UP)
        tf.velocityDivergenceBackward(UP, flags, go, dU)
        gradU = gradU + dU
    assert gradP.dtype == F and gradU.dtype == F
    return dict(loss=[lp, lu, ld, (lp + lu) + ld], gradP=gradP, gradU=gradU)


@functools.lru_cache(maxsize=None)
def _expected(tf_key, name, weighted, lam, sizeAverage):
    tf = _TFS[tf_key]
    pP, UP, pT, UT, flags = make_case(name)
    w = weight(tf, flags, *BORDER) if weighted else None
    out = criterion(tf, pP, UP, pT, UT, flags, w, LAMBDAS[lam], sizeAverage)
    out["weight"] = w
    return out


_TFS = {}


def expected(tf, name, weighted, lam="all", sizeAverage=True):
    """the restatement's result for a case, computed once per process and shared (treat it as read-only)"""
    _TFS.setdefault(id(tf), tf)
    return _expected(id(tf), name, bool(weighted), lam, bool(sizeAverage))
