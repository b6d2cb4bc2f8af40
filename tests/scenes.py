"""Seeded synthetic scenes shared by the parity tests (CPU and GPU) and the golden generator.

Every field is a contiguous float32 [B, C, Z, Y, X] array, x fastest, like the reference's tensors
(torch/tfluids/third_party/grid.h:68-78). Flags hold Manta cell types as floats
(third_party/cell_type.h:22-33).
"""
import numpy as np

FLUID, OBSTACLE, EMPTY, OUTFLOW, STICK = 1, 2, 4, 16, 128
INFLOW, OPEN = 8, 32
# the flag alphabet: every single cell-type bit, the composites the kernels' decisions tell apart, and the word 0
ALPHABET = (1, 2, 4, 8, 16, 32, 128, 2 | 128, 4 | 16, 1 | 8, 4 | 32, 2 | 8, 1 | 16, 4 | 8, 0, 1 | 128)


def empty_domain(B, Z, Y, X, is3d, bnd=1):
    """generic/tfluids.cc:136-167 restated in numpy (test helper)."""
    f = np.full((B, 1, Z, Y, X), FLUID, np.float32)
    f[..., :bnd] = OBSTACLE
    f[..., X - bnd:] = OBSTACLE
    f[..., :bnd, :] = OBSTACLE
    f[..., Y - bnd:, :] = OBSTACLE
    if is3d:
        f[:, :, :bnd] = OBSTACLE
        f[:, :, Z - bnd:] = OBSTACLE
    return f


def add_obstacles(flags, is3d, rng, n_sphere=2, n_box=1, stick=False):
    B, _, Z, Y, X = flags.shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    for b in range(B):
        for _ in range(n_sphere):
            c = [rng.uniform(0.25, 0.75) * s for s in (X, Y, Z)]
            r = rng.uniform(0.08, 0.16) * min(X, Y, Z if is3d else X)
            d2 = (xx - c[0]) ** 2 + (yy - c[1]) ** 2 + ((zz - c[2]) ** 2 if is3d else 0)
            flags[b, 0][d2 <= r * r] = OBSTACLE | (STICK if stick else 0)
        for _ in range(n_box):
            lo = [int(rng.uniform(0.15, 0.6) * s) for s in (X, Y, Z)]
            sz = [max(1, int(rng.uniform(0.05, 0.2) * s)) for s in (X, Y, Z)]
            ks = slice(lo[2], lo[2] + sz[2]) if is3d else slice(0, 1)
            flags[b, 0, ks, lo[1]:lo[1] + sz[1], lo[0]:lo[0] + sz[0]] = OBSTACLE
    return flags


def smooth_field(shape, rng, modes=4):
    """Sum of a few random sinusoids: smooth, non-trivial, deterministic for a seeded rng."""
    B, C, Z, Y, X = shape
    zz, yy, xx = np.meshgrid(np.arange(Z) / max(Z, 1), np.arange(Y) / Y, np.arange(X) / X,
                             indexing="ij")
    out = np.zeros(shape, np.float64)
    for b in range(B):
        for c in range(C):
            for _ in range(modes):
                k = rng.randint(1, 4, size=3)
                ph = rng.uniform(0, 2 * np.pi, size=3)
                a = rng.uniform(0.3, 1.0)
                out[b, c] += a * np.sin(2 * np.pi * k[0] * xx + ph[0]) * \
                    np.sin(2 * np.pi * k[1] * yy + ph[1]) * \
                    (np.sin(2 * np.pi * k[2] * zz + ph[2]) if Z > 1 else 1.0)
    return out


def make_scene(dims, seed=0, B=1, vel_cells=2.5, dt=0.1, obstacles=True, empty_cells=False,
               stick=False, noise=0.0):
    """dims = (Z, Y, X); Z == 1 means 2-D. vel_cells = max |u_c|*dt in cells."""
    Z, Y, X = dims
    is3d = Z > 1
    C = 3 if is3d else 2
    rng = np.random.RandomState(seed)
    flags = empty_domain(B, Z, Y, X, is3d)
    if obstacles:
        add_obstacles(flags, is3d, rng, stick=stick)
    if empty_cells:  # a slab of empty / outflow cells for velocityUpdate, addGravity coverage
        j0 = int(0.8 * Y)
        sl = flags[:, :, 1:-1, j0:Y - 1, 1:X - 1] if is3d else flags[:, :, :, j0:Y - 1, 1:X - 1]
        sl[sl == FLUID] = EMPTY
        sl[..., -1, :][sl[..., -1, :] == EMPTY] = EMPTY | OUTFLOW
    U = smooth_field((B, C, Z, Y, X), rng)
    U *= vel_cells / dt / max(np.abs(U).max(), 1e-9)
    if noise > 0:
        U += noise * rng.randn(*U.shape)
    s = np.abs(smooth_field((B, 1, Z, Y, X), rng)) + 0.1
    p = smooth_field((B, 1, Z, Y, X), rng)
    return dict(flags=np.ascontiguousarray(flags, np.float32), U=U.astype(np.float32),
                density=s.astype(np.float32), p=p.astype(np.float32), is3d=is3d, dt=dt)


def rough_scene(dims, seed=0, B=1, obstacle_frac=0.1, empty_frac=0.0, dt=0.1):
    """White-noise U and p, salt-and-pepper obstacles at about `obstacle_frac` of the cells inside the walls and, with
    empty_frac > 0, empty cells: neighbouring voxels are uncorrelated, so a convolution tap that reads the wrong voxel is
    off by O(1). (The projection net's FlagsToOccupancy refuses empty cells, generic/tfluids.cu:355-371, so scenes that
    feed the net keep empty_frac = 0.)"""
    Z, Y, X = dims
    is3d = Z > 1
    C = 3 if is3d else 2
    rng = np.random.RandomState(seed)
    flags = empty_domain(B, Z, Y, X, is3d)
    inner = flags == FLUID
    draw = rng.uniform(size=flags.shape)
    flags[inner & (draw < obstacle_frac)] = OBSTACLE
    flags[inner & (draw >= obstacle_frac) & (draw < obstacle_frac + empty_frac)] = EMPTY
    U = rng.randn(B, C, Z, Y, X)
    p = rng.randn(B, 1, Z, Y, X)
    s = rng.uniform(0.1, 1.0, size=(B, 1, Z, Y, X))
    return dict(flags=np.ascontiguousarray(flags, np.float32), U=U.astype(np.float32), density=s.astype(np.float32),
                p=p.astype(np.float32), is3d=is3d, dt=dt)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def pcg_problem(tf, dims, seed, vel_cells=2.0, split=False, **kw):
    """flags + the divergence of a wall-BC'd random velocity field: the right-hand side of the reference's PCG test
    (test_tfluids.lua:836-906 does the same from its Manta fixtures). split=True walls off part of the domain (a
    second fluid component) and leaves one fluid cell enclosed on its own (a size-1 component, which the solver
    skips). tf = any object with the tfluids operator methods (oracle / ref / HIP adapter)."""
    sc = make_scene(dims, seed=seed, vel_cells=vel_cells, **kw)
    f = sc["flags"]
    if split:
        Z, Y, X = dims
        xs = X // 2
        f[..., xs] = 2.0                         # a wall across x
        f[..., xs + 1:xs + 4] = np.where(f[..., xs + 1:xs + 4] == 1.0, 1.0, f[..., xs + 1:xs + 4])
        j0, k0 = Y // 2, (Z // 2 if Z > 1 else 0)
        if Z > 1:
            f[:, :, k0 - 1:k0 + 2, j0 - 1:j0 + 2, 2:5] = 2.0
        else:
            f[:, :, :, j0 - 1:j0 + 2, 2:5] = 2.0
        f[:, :, k0, j0, 3] = 1.0                 # one fluid cell inside a 3^dim obstacle block
    U = sc["U"].copy()
    tf.setWallBcsForward(U, f)
    div = np.zeros_like(sc["p"])
    tf.velocityDivergenceForward(U, f, div)
    return sc, f, U, div


# ---- the flag alphabet: every cell-type word, next to every other, border included ---------------------------------------
def border_mask(shape, is3d):
    """True on the one-cell shell of a [B, 1, Z, Y, X] grid (x and y faces; z faces in 3-D)"""
    m = np.zeros(shape, bool)
    m[..., 0] = m[..., -1] = True
    m[..., 0, :] = m[..., -1, :] = True
    if is3d:
        m[:, :, 0] = m[:, :, -1] = True
    return m


def alphabet_scene(dims, seed, B=1, frac=1.0 / 3.0, border=False, words=ALPHABET, fluid_border=False, vel_cells=1.5,
                   noise=2.0, dt=0.1):
    """make_scene without obstacles and with white noise on U (neighbouring voxels uncorrelated), then a seeded `frac` of
    the cells overwritten with words drawn uniformly from `words`: inside the walls only, or with border=True on the
    border shell too (Manta's open domain; unless fluid_border is set, the fluid bit of a border word is replaced by empty:
    the PCG solver refuses fluid on the border, generic/tfluids.cu:1082-1090). The draw covers the whole [B, ...] array,
    so every sample of a batch has its own field."""
    Z, Y, X = dims
    sc = make_scene(dims, seed=seed, B=B, vel_cells=vel_cells, dt=dt, obstacles=False, noise=noise)
    f = sc["flags"]
    rng = np.random.RandomState(seed + 7919)
    pick = rng.uniform(size=f.shape) < frac
    w = np.asarray(words, np.int64)[rng.randint(len(words), size=f.shape)]
    shell = border_mask(f.shape, sc["is3d"])
    if border and not fluid_border:
        w = np.where(shell & ((w & FLUID) != 0), (w & ~FLUID) | EMPTY, w)
    target = pick & (~shell | bool(border))
    f[target] = w[target].astype(np.float32)
    return sc


def _faces(is3d):
    """(name, (dz, dy, dx)) of the face neighbours, opposite faces next to each other"""
    f = [("-x", (0, 0, -1)), ("+x", (0, 0, 1)), ("-y", (0, -1, 0)), ("+y", (0, 1, 0))]
    return f + [("-z", (-1, 0, 0)), ("+z", (1, 0, 0))] if is3d else f


def neighbourhood_design(n=len(ALPHABET)):
    """[n * n, 7] indices into the alphabet: centre, -x, +x, -y, +y, -z, +z of stencil t = (a, b). The centre is a, face m
    holds (m a + b) mod n with m = 0, 1, 2, 3, 5, 6 (two orthogonal Latin squares per axis): for every face (a, m a + b)
    runs through all n^2 ordered pairs, and for every axis the two faces differ by a, so (lo, hi) does too."""
    a, b = np.divmod(np.arange(n * n), n)
    return np.stack([a] + [(m * a + b) % n for m in (0, 1, 2, 3, 5, 6)], axis=1)


def neighbourhood_scene(dims, seed, B=1, words=ALPHABET, vel_cells=1.5, noise=2.0, dt=0.1):
    """The interior tiled with 3 x 3 (x 3) stencils whose centre and face neighbours run through neighbourhood_design
    (seeded: a permutation of the alphabet per role, the stencils in shuffled order, sample after sample continuing where
    the last one stopped, so that len(words)^2 stencils in all hold the full cover); the stencils' corners hold seeded
    random words, cells that no stencil reaches stay fluid, the border stays obstacle. neighbourhood_cover counts what a
    field holds."""
    Z, Y, X = dims
    sc = make_scene(dims, seed=seed, B=B, vel_cells=vel_cells, dt=dt, obstacles=False, noise=noise)
    f, is3d = sc["flags"], sc["is3d"]
    rng = np.random.RandomState(seed + 104729)
    n = len(words)
    wv = np.asarray(words, np.float32)
    design = neighbourhood_design(n)
    perms = [rng.permutation(n) for _ in range(7)]
    order = rng.permutation(n * n)
    nz, ny, nx = ((Z - 2) // 3 if is3d else 1), (Y - 2) // 3, (X - 2) // 3
    t = 0
    centres = np.zeros(f.shape, bool)
    for b in range(B):
        for tz in range(nz):
            for ty in range(ny):
                for tx in range(nx):
                    k, j, i = (2 + 3 * tz if is3d else 0), 2 + 3 * ty, 2 + 3 * tx       # the stencil's centre
                    ks = slice(k - 1, k + 2) if is3d else slice(0, 1)
                    blk = f[b, 0, ks, j - 1:j + 2, i - 1:i + 2]
                    blk[...] = wv[rng.randint(n, size=blk.shape)]
                    row = design[order[t % (n * n)]]
                    f[b, 0, k, j, i] = wv[perms[0][row[0]]]
                    centres[b, 0, k, j, i] = True
                    for m, (_, (dz, dy, dx)) in enumerate(_faces(is3d)):
                        f[b, 0, k + dz, j + dy, i + dx] = wv[perms[1 + m][row[1 + m]]]
                    t += 1
    sc["stencils"] = t
    sc["centres"] = centres
    return sc


def neighbourhood_cover(flags, is3d, words=ALPHABET, centres=None):
    """What a flag field holds, counted over every cell that has all its face neighbours in the array (all samples; with
    `centres`, a mask like neighbourhood_scene's "centres", over those cells only: the designed stencils without what their
    random corners and the seams between them add):
    {"face": {name: number of distinct ordered (centre word, neighbour word) pairs}, "axis": {name: number of distinct
    (word at the - face, word at the + face) pairs}, "full": len(words)^2}. Only words of `words` count."""
    idx = {int(w): i for i, w in enumerate(words)}
    n = len(words)
    code = np.vectorize(lambda v: idx.get(int(v), -1))(flags[:, 0]).astype(np.int64)
    B, Z, Y, X = code.shape
    core = (slice(None), slice(1, Z - 1) if is3d else slice(None), slice(1, Y - 1), slice(1, X - 1))
    c = code[core]

    def shifted(d):
        dz, dy, dx = d
        return code[:, (slice(1 + dz, Z - 1 + dz) if is3d else slice(None)), 1 + dy:Y - 1 + dy, 1 + dx:X - 1 + dx]

    sel = np.ones(c.shape, bool) if centres is None else centres[:, 0][core]

    def distinct(a, b):
        ok = (a >= 0) & (b >= 0) & sel
        return int(np.unique(a[ok] * n + b[ok]).size)

    faces = _faces(is3d)
    out = {"face": {}, "axis": {}, "full": n * n}
    for name, d in faces:
        out["face"][name] = distinct(c, shifted(d))
    for m in range(0, len(faces), 2):
        out["axis"][faces[m][0][1]] = distinct(shifted(faces[m][1]), shifted(faces[m + 1][1]))
    return out
