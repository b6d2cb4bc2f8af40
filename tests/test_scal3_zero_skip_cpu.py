"""The lane predicate `small` of advectScalar's short path (fluidnet_amd/csrc/advect_scalar3.hip): whenever
every component of the displacement is at most kSmallDisp in magnitude and the grid's extent is at most kSmallExtent, the
fast trace is a single short step that ends strictly inside the lane's own cell -- which is what lets a block whose tile is
all +0.0 write (+0, +0, +0) without tracing. trace_fast's arithmetic is restated here in numpy float32 (every operation
rounded once, `/` and sqrt correctly rounded as the kernel's div_by / sqrt_rcp_exact are) and run over a few million random and
adversarial displacements and cell coordinates. Both constants are read from the source, so the proof is pinned to the kernel."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "fluidnet_amd", "csrc", "advect_scalar3.hip")).read()
F = np.float32


def _constants():
    t = re.search(r"constexpr float kSmallDisp = ([0-9.]+)f;", SRC)
    e = re.search(r"constexpr int kSmallExtent = 1 << (\d+);", SRC)
    fl = re.search(r"constexpr float kFastLen = ([0-9.]+)f;", SRC)
    return F(t.group(1)), 1 << int(e.group(1)), F(fl.group(1))


T, EXTENT, FAST_LEN = _constants()


def trace_fast(ctr, d, fast):
    """trace_fast<FAST> up to the end point: (p, shortd), float32 throughout. ctr, d: (N, 3)"""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    l2 = (dx * dx + dy * dy) + dz * dz
    assert l2.dtype == np.float32
    nz = l2 > F(1e-6)
    if fast:
        p = np.where(nz[:, None], ctr + d, ctr)
        return p, l2 <= FAST_LEN * FAST_LEN
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.where(nz, np.sqrt(l2), F(0))
        q = np.where(nz[:, None], d / ln[:, None], F(0))      # len = 0: r = 0, div_by gives 0
    p = ctr + q * ln[:, None]
    assert p.dtype == np.float32
    return p, ln <= FAST_LEN


def small(d):
    return (np.abs(d) <= T).all(axis=1)      # ordered compares: a NaN makes it false


def _cells(rng, n):
    """cell indices of `deep` cells (1 .. extent - 2) per axis: uniform, around every power of two, and the ends of the range"""
    hi = EXTENT - 2
    edge = np.array(sorted({c for k in range(1, 17) for c in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 1 <= c <= hi} | {1, 2, hi - 1, hi}))
    c = rng.randint(1, hi + 1, size=(n, 3))
    pick = rng.rand(n, 3) < 0.5
    return np.where(pick, edge[rng.randint(0, len(edge), size=(n, 3))], c)


def _displacements(rng, n):
    """uniform in [-T, T], log-uniform magnitudes down to the denormals, and the adversarial values: +-T, its neighbours, 0, -0,
    the norm threshold 1e-6 = l2 from either side, mixed per component"""
    uni = rng.uniform(-float(T), float(T), size=(n, 3)).astype(F)
    logm = (float(T) * np.exp(rng.uniform(-105.0, 0.0, size=(n, 3)))).astype(F) * rng.choice([-1.0, 1.0], size=(n, 3)).astype(F)
    thr = np.sqrt(F(1e-6) / F(3))
    adv = np.array([T, -T, np.nextafter(T, F(0)), -np.nextafter(T, F(0)), F(0), F(-0.0), F(1e-3), F(-1e-3), thr, np.nextafter(thr, F(1)),
                    np.nextafter(thr, F(0)), F(1e-45), F(1.1754944e-38), F(0.25), F(-0.125)], dtype=F)
    advs = adv[rng.randint(0, len(adv), size=(n, 3))]
    sel = rng.randint(0, 3, size=(n, 3))
    return np.where(sel == 0, uni, np.where(sel == 1, logm, advs)).astype(F)


def _check(ctr_cell, d, fast):
    ctr = ctr_cell.astype(F) + F(0.5)
    assert (ctr.astype(np.float64) == ctr_cell + 0.5).all()          # the centres are exact below the extent bound
    p, shortd = trace_fast(ctr, d, fast)
    m = small(d)
    assert m.any()
    cell = ctr_cell[m].astype(np.float64)
    pm = p[m].astype(np.float64)
    assert shortd[m].all()                                            # len <= kFastLen: a single step
    assert np.isfinite(pm).all()
    assert ((pm > cell) & (pm < cell + 1.0)).all()                    # strictly inside the own cell on every axis
    assert (p[m].astype(np.int32) == ctr_cell[m]).all()               # (int)p: the tile index trace_fast forms is the own cell's
    # lerp_tile's base corner int(p - 0.5) is the cell or its lower neighbour: the own cell is one of the eight corners
    base = (p[m] - F(0.5)).astype(np.int32)
    assert ((base == ctr_cell[m]) | (base == ctr_cell[m] - 1)).all() and (p[m] - F(0.5) >= 0).all()
    # the step the trace makes is no longer than the displacement by more than a few ulp
    step = np.abs(pm - (cell + 0.5))
    assert (step <= np.abs(d[m].astype(np.float64)) * (1 + 4 * 2.0 ** -23) + 2.0 ** -9).all()
    return int(m.sum())


def test_constants_are_the_ones_reasoned_about():
    assert T == F(0.45) and EXTENT == 1 << 16 and FAST_LEN == F(0.99)
    # three components of T: the length stays below kFastLen with room to spare
    assert np.sqrt(3.0) * float(T) * (1 + 1e-6) < float(FAST_LEN)
    # ulp of the largest centre is 2^-8: half an ulp of rounding leaves T * (1 + few ulp) + 2^-9 < 0.5
    assert np.spacing(F(EXTENT - 1.5)) == F(2.0 ** -8) and float(T) * (1 + 1e-6) + 2.0 ** -9 < 0.5


def test_small_displacements_end_in_the_own_cell():
    rng = np.random.RandomState(20)
    n_small = 0
    for fast in (False, True):
        for _ in range(2):
            n_small += _check(_cells(rng, 1 << 20), _displacements(rng, 1 << 20), fast)
    assert n_small > 3 << 20


def test_every_cell_coordinate_with_the_extreme_displacements():
    """all 65534 deep cell coordinates of one axis x the displacements at +-T (all three components at the bound: the longest
    `small` step) and one ulp inside"""
    c = np.arange(1, EXTENT - 1)
    cells = np.stack([c, c[::-1], c], axis=1)
    for fast in (False, True):
        for v in (T, -T, np.nextafter(T, F(0)), -np.nextafter(T, F(0))):
            for signs in ((1, 1, 1), (1, -1, 1), (-1, 1, -1)):
                d = np.tile(np.array(signs, dtype=F) * v, (len(c), 1))
                assert _check(cells, d, fast) == len(c)


def test_the_predicate_rejects_what_the_proof_does_not_cover():
    d = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nextafter(T, F(1)), 0, 0], [0, -0.46, 0], [0.1, 0.2, 0.3]], dtype=F)
    assert small(d).tolist() == [False, False, False, False, False, True]
    # and the check above can fail: half a cell and more leaves the own cell (so T cannot be 0.5)
    ctr = np.full((1, 3), 7.5, dtype=F)
    p, _ = trace_fast(ctr, np.array([[0.5, 0, 0]], dtype=F), False)
    assert int(p[0, 0]) == 8
