"""The condition under which tfl_simulate_step advects a density over a list of bricks only (fluidnet_amd/csrc/
advect_scalar3_sparse.hip): with |u dt| <= 0.9 on every velocity word, a word of maccormackOurs' in-place
advectScalar can differ from its input word only within Chebyshev distance 4 of a word of the input that is not +0.0 -- counting
every cell, fluid or not. The C oracle's advectScalar is run over a few hundred seeded scenes (random obstacles, a 3^3 blob that may
overlap them, obstacles next to the blob, a blob inside an obstacle, a -0.0 word, speeds up to 0.9f / dt and on it) and the bound
is asserted on the bit patterns. A numpy model of the kernels' brick map -- nz -> L_B -> L_A on bricks of 64 x 4 x 4 cells -- must
cover every changed cell by L_B and every cell whose temporaries a cell of L_B reads (+-2) by L_A. The constants 0.9f and 64 / 4 / 4
are read from the source, so the bound is pinned to the kernels."""
import os
import re

import numpy as np

from scenes import FLUID, OBSTACLE, empty_domain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "fluidnet_amd", "csrc", "advect_scalar3_sparse.hip")).read()
F = np.float32
DT = 0.4
REACH = 4      # the derived bound: pass A reads s within +-2, pass B reads pass A's results within +-2


def _constants():
    d = re.search(r"constexpr float kSparseDisp = ([0-9.]+)f;", SRC)
    b = re.search(r"constexpr int kBrickX = (\d+), kBrickY = (\d+), kBrickZ = (\d+);", SRC)
    return F(d.group(1)), tuple(int(v) for v in b.groups())


DISP, BRICK = _constants()


def test_constants_are_the_sources():
    assert DISP == F(0.9) and BRICK == (64, 4, 4)
    # a brick is at least as thick as the reach on every axis: "within +-4 of a cell of the brick" stays inside its 1-ring
    assert min(BRICK) >= REACH
    # the scan's test, as the kernel writes it: an ordered compare of |u * dt| against the constant
    assert "__builtin_fabsf(u * dt) <= kSparseDisp ? 0u : 1u" in SRC


def test_the_policys_constants_are_the_ones_the_gpu_test_counts_with():
    import scal3_sparse_run as R
    host = open(os.path.join(ROOT, "fluidnet_amd", "csrc", "simulate.cpp")).read()
    assert int(re.search(r"constexpr unsigned kSparseProbe = (\d+);", host).group(1)) == R.POLICY_P
    assert float(re.search(r"constexpr double kSparseThreshold = ([0-9.]+);", host).group(1)) == 0.25
    assert R.BRICK == BRICK[::-1] and R.fastest_allowed(DT)[0] == fastest_allowed(DT)


def fastest_allowed(dt):
    """the largest float32 u with fl(u * dt) <= 0.9f: the scan lets it pass"""
    u = F(DISP / F(dt))
    while F(u * F(dt)) > DISP:
        u = np.nextafter(u, F(0))
    while F(np.nextafter(u, F(np.inf)) * F(dt)) <= DISP:
        u = np.nextafter(u, F(np.inf))
    return u


def dilate(mask, r):
    """cells within Chebyshev distance r of a set cell of mask [Z][Y][X]"""
    out = mask.copy()
    for axis in range(3):
        acc = out.copy()
        for sh in range(1, r + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(sh, None), slice(None, -sh)
            acc[tuple(lo)] |= out[tuple(hi)]
            acc[tuple(hi)] |= out[tuple(lo)]
        out = acc
    return out


def brick_lists(nonzero, box=None):
    """the model of k_scal3_scan + k_scal3_lists: cell masks of the bricks of L_A and L_B for one item's [Z][Y][X] mask of words
    that are not +0.0 (box: inclusive (x0, x1, y0, y1, z0, z1) of a setConstVals pair, or None)"""
    Z, Y, X = nonzero.shape
    bx, by, bz = BRICK
    nb = (-(-Z // bz), -(-Y // by), -(-X // bx))
    nz = np.zeros(nb, bool)
    for k, j, i in zip(*np.nonzero(nonzero)):
        nz[k // bz, j // by, i // bx] = True
    lb = dilate(nz, 1)
    if box is not None:
        x0, x1, y0, y1, z0, z1 = box
        lb[z0 // bz:z1 // bz + 1, y0 // by:y1 // by + 1, x0 // bx:x1 // bx + 1] = True
    la = dilate(lb, 1)

    def cells(m):
        return np.repeat(np.repeat(np.repeat(m, bz, 0), by, 1), bx, 2)[:Z, :Y, :X]
    return cells(la), cells(lb)


def scene(seed, dims):
    """flags, U, density of one scene; the blob's kind cycles with the seed"""
    Z, Y, X = dims
    rng = np.random.RandomState(seed)
    flags = empty_domain(1, Z, Y, X, True).astype(F)
    inner = flags == FLUID
    flags[inner & (rng.uniform(size=flags.shape) < 0.06)] = OBSTACLE
    vmax = fastest_allowed(DT)
    kind = seed % 5
    if kind == 0:      # speeds up to the bound, many words exactly on it
        U = rng.uniform(-1, 1, size=(1, 3, Z, Y, X)).astype(F) * vmax
        on = rng.uniform(size=U.shape) < 0.2
        U[on] = np.where(rng.uniform(size=on.sum()) < 0.5, vmax, -vmax)
    elif kind == 1:    # every word on the bound: the longest displacement the scan lets pass, diagonal
        U = np.full((1, 3, Z, Y, X), vmax, F) * np.where(rng.uniform(size=(1, 3, 1, 1, 1)) < 0.5, F(1), F(-1))
    else:
        U = (rng.uniform(-1, 1, size=(1, 3, Z, Y, X)) * rng.choice([0.3, 0.7, 1.0])).astype(F) * vmax
    U = np.clip(U, -vmax, vmax).astype(F)
    assert (np.abs((U * F(DT)).astype(F)) <= DISP).all()
    s = np.zeros((1, 1, Z, Y, X), F)
    c = [int(rng.randint(2, n - 4)) for n in (Z, Y, X)]
    blob = (0, 0, slice(c[0], c[0] + 3), slice(c[1], c[1] + 3), slice(c[2], c[2] + 3))
    s[blob] = rng.uniform(0.1, 1.0, size=(3, 3, 3)).astype(F)
    if kind == 2:      # obstacles next to the blob: a shell around it with gaps
        shell = (0, 0, slice(c[0] - 1, c[0] + 4), slice(c[1] - 1, c[1] + 4), slice(c[2] - 1, c[2] + 4))
        keep = flags[blob].copy()
        sh = flags[shell]
        sh[rng.uniform(size=sh.shape) < 0.6] = OBSTACLE
        flags[blob] = keep
    if kind == 3:      # the blob inside an obstacle, next to empty fluid
        flags[blob] = OBSTACLE
    if kind == 4:      # a single -0.0 word far from the blob counts as non-zero too
        far = tuple((v + n // 2) % (n - 2) + 1 for v, n in zip(c, (Z, Y, X)))
        s[(0, 0) + far] = F(-0.0)
    flags[:, :, 0, :, :] = flags[:, :, -1, :, :] = OBSTACLE
    flags[:, :, :, 0, :] = flags[:, :, :, -1, :] = OBSTACLE
    flags[:, :, :, :, 0] = flags[:, :, :, :, -1] = OBSTACLE
    return flags, U, s


def check(oracle, seed, dims, strength):
    flags, U, s = scene(seed, dims)
    before = s.copy()
    prev = oracle.strict
    oracle.strict = True      # a trace that hit a reference error path would say so
    try:
        oracle.advectScalar(DT, s, U, flags, "maccormackOurs", sDst=s, maccormackStrength=strength)
    finally:
        oracle.strict = prev
    nonzero = before.view(np.uint32)[0, 0] != 0
    changed = s.view(np.uint32)[0, 0] != before.view(np.uint32)[0, 0]
    assert nonzero.any()
    near = dilate(nonzero, REACH)
    far_changed = changed & ~near
    assert not far_changed.any(), (seed, dims, strength, np.argwhere(far_changed)[:4].tolist())
    la, lb = brick_lists(nonzero)
    assert not (changed & ~lb).any(), (seed, "a changed cell outside L_B")
    assert not (dilate(lb, 2) & ~la).any(), (seed, "a cell of L_B reads temporaries outside L_A")
    # how far the changes really went (random fields rarely chain the worst case)
    reach = 0
    for r in range(REACH + 1):
        if not (changed & ~dilate(nonzero, r)).any():
            break
        reach = r + 1
    return reach


def test_no_word_changes_beyond_distance_4_of_a_nonzero_word(oracle):
    worst = 0
    for seed in range(240):
        worst = max(worst, check(oracle, seed, (22, 26, 30), 0.6 if seed % 2 else 0.75))
    assert 1 <= worst <= REACH
    print("farthest changed cell: Chebyshev distance %d of a non-zero input word (bound %d)" % (worst, REACH))


def test_the_same_on_a_grid_two_bricks_wide(oracle):
    for seed in range(1000, 1060):
        check(oracle, seed, (13, 11, 70), 0.75 if seed % 2 else 0.6)


def test_the_box_of_a_boundary_pair_is_listed():
    """an all-zero density with a non-empty setConstVals box: L_B is the box's bricks, L_A their 1-ring"""
    nonzero = np.zeros((12, 12, 130), bool)
    la, lb = brick_lists(nonzero, box=(60, 70, 5, 6, 3, 3))
    assert lb[:4, 4:8, :128].all() and lb.sum() == 4 * 4 * 128
    assert la[:8, :12, :].all() and la.sum() == 8 * 12 * 130
