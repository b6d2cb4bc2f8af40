"""Shared by tests/test_oracle.py (CPU) and tests/test_hip_flag_alphabet.py (GPU): the flag-alphabet cases -- scenes of
tests/scenes.py alphabet_scene / neighbourhood_scene on the shapes below --, a guard that turns "the reference raises here" into
a comparable outcome, and a numpy restatement of the setWallBcs decision with which the CPU suite checks that the neighbourhood
scene would catch a one-bit decoding defect.

Shapes: small and ragged against the launch geometry (64 x 4 blocks, 4 cells per thread, 6-wide guarded rows). (4, 6, 68) is one
full lane segment plus a tail, (1, 9, 67) has an odd X (the one-cell-per-thread fallbacks), (8, 23, 50) x B = 2 is a small
grid whose 448 stencils hold the neighbourhood scene's full cover in 3-D; (1, 66, 130) holds it in 2-D."""
import numpy as np

import scenes
from golden.make_golden import run_ops

SHAPES3 = [(5, 9, 21), (4, 6, 68), (3, 3, 3), (6, 7, 130)]
SHAPES2 = [(1, 13, 21), (1, 9, 67), (1, 66, 130)]
COVER3 = (8, 23, 50)
B = 2
# (generator, border): the neighbourhood scene keeps the obstacle border
KINDS = [("alphabet", False), ("alphabet", True), ("neighbourhood", False)]
# FlagsToOccupancy. The reference's two builds differ. Its CUDA kernel (generic/tfluids.cu:355-371) tests the fluid BIT (-> 0),
# then the obstacle BIT (-> 1), writes -1 otherwise, and its host function never raises (:394-398, the check is commented out).
# Its CPU function (generic/tfluids.cc:175-210) takes the two plain words and raises on every other. The library implements
# the CUDA contract (the projection net's fused occupancy reads too); the compiled checker is the CPU function, so the two
# agree on PLAIN_WORDS, and elsewhere the tests put BitTestOccupancy in front of the oracle.
PLAIN_WORDS = (1, 2)
OCCUPANCY_WORDS = tuple(w for w in scenes.ALPHABET if w & 3)      # a 0 or a 1, not the -1


def occupancy_np(flags):
    """generic/tfluids.cu:362-370 restated"""
    w = flags.astype(np.int64)
    return np.where((w & 1) != 0, 0.0, np.where((w & 2) != 0, 1.0, -1.0)).astype(np.float32)


class BitTestOccupancy:
    """an operator object (oracle, compiled reference) with flagsToOccupancy replaced by the CUDA build's contract"""

    def __init__(self, impl):
        self._impl = impl

    def __getattr__(self, name):
        return getattr(self._impl, name)

    def flagsToOccupancy(self, flags, occupancy):
        occupancy[...] = occupancy_np(flags)


def seed_of(dims, kind, border):
    return 1000 + 7 * dims[0] + 13 * dims[1] + 17 * dims[2] + (500 if kind == "neighbourhood" else 0) + (250 if border else 0)


def scene(kind, dims, border=False, B=B, **kw):
    seed = seed_of(dims, kind, border)
    if kind == "alphabet":
        return scenes.alphabet_scene(dims, seed, B=B, border=border, **kw)
    assert not border
    return scenes.neighbourhood_scene(dims, seed, B=B, **kw)


def case_id(kind, dims, border):
    return "%s-%s%s" % (kind, "x".join(str(d) for d in dims), "-border" if border else "")


def holds_stencils(dims):
    """a 3 x 3 (x 3) stencil fits inside the border shell ((4, 6, 68) and (3, 3, 3) are too thin: alphabet scenes only)"""
    return all(d - 2 >= 3 for d in (dims if dims[0] > 1 else dims[1:]))


CASES = [(k, d, b) for d in SHAPES3 + SHAPES2 + [COVER3] for (k, b) in KINDS if k == "alphabet" or holds_stencils(d)]
CASE_IDS = [case_id(*c) for c in CASES]


def _errors():
    from oracle.oracle import OracleError
    from oracle.ref import RefError
    errs = [OracleError, RefError]
    try:
        from fluidnet_amd import TfluidsError
        errs.append(TfluidsError)
    except Exception:       # (no torch / no library: the CPU suite needs neither)
        pass
    return tuple(errs)


class Guard:
    """Wraps an implementation with the numpy operator surface: an operator that raises the implementation's own error (the
    reference's THError paths: a back-trace that starts in a blocked cell, ...) is recorded in .raised under the key run_ops
    files its result under instead of ending the run; on the GPU, where a trace that hits such a path is counted and not raised,
    a non-zero traceErrors() after the operator is recorded the same way."""

    def __init__(self, impl):
        self.impl, self.raised, self.errors = impl, set(), _errors()

    def __getattr__(self, name):
        fn = getattr(self.impl, name)

        def call(*a, **kw):
            key = name
            if name == "advectScalar":
                key = "advectScalar_" + a[4]
            elif name == "advectVel":
                key = "advectVel_" + a[3]
            try:
                r = fn(*a, **kw)
            except self.errors:
                self.raised.add(key)
                return None
            if name.startswith("advect") and hasattr(self.impl, "traceErrors") and self.impl.traceErrors() != 0:
                self.raised.add(key)
            return r
        return call


RUN_OPS_KEYS = {"setWallBcsForward": "setWallBcs", "velocityDivergenceForward": "divergence", "velocityUpdateForward": "velocityUpdate",
                "vorticityConfinement": "vorticity", "addBuoyancy": "buoyancy", "addGravity": "gravity"}


def guarded_ops(impl, sc):
    """(run_ops results, set of result keys whose operator raised)"""
    g = Guard(impl)
    out = run_ops(g, sc)
    return out, {RUN_OPS_KEYS.get(k, k) for k in g.raised}


def compare_ops(got, want, what):
    """bit equality of two guarded_ops results: the same operators raise on both sides, every other result is equal word
    for word and finite. Returns (words compared, operators that raised on both sides)."""
    (a, ra), (b, rb) = got, want
    assert ra == rb, (what, "raised on one side only", sorted(ra ^ rb))
    words, bad = 0, []
    for k in sorted(b):
        if k in rb:
            continue
        assert np.isfinite(a[k]).all(), (what, k)
        words += a[k].size
        n = int((a[k] != b[k]).sum())
        if n:
            bad.append((k, n, float(np.abs(a[k] - b[k]).max())))
    assert not bad, "%s: not bit-exact: %s" % (what, bad)
    return words, sorted(rb)


# ---- the setWallBcs decision restated in numpy (third_party/tfluids.cc:926-1002) ------------------------------------------
def _nb(w, d):
    """the words of the neighbours at offset d = (dz, dy, dx), 0 outside the grid"""
    out = np.zeros_like(w)
    src = [slice(max(0, s), w.shape[2 + a] + min(0, s)) for a, s in enumerate(d)]
    dst = [slice(max(0, -s), w.shape[2 + a] + min(0, -s)) for a, s in enumerate(d)]
    out[(slice(None), slice(None)) + tuple(dst)] = w[(slice(None), slice(None)) + tuple(src)]
    return out


def wall_mask_np(flags, is3d, defect=None):
    """[B, C, Z, Y, X] bool: the velocity components setWallBcs zeroes. defect = "stick-y" drops the stick test of the y
    axis (one term of the decision), the kind of slip a rebuilt mask makes."""
    w = flags.astype(np.int64)
    cf, co = (w & 1) != 0, (w & 2) != 0
    act = cf | co
    z = []
    for d in ((0, 0, -1), (0, -1, 0), (-1, 0, 0)):
        m = _nb(w, d)
        z.append(act & (((m & 2) != 0) | (co & ((m & 1) != 0))))
    sx = ((_nb(w, (0, 0, -1)) | _nb(w, (0, 0, 1))) & 128) != 0
    sy = ((_nb(w, (0, -1, 0)) | _nb(w, (0, 1, 0))) & 128) != 0
    sz = ((_nb(w, (-1, 0, 0)) | _nb(w, (1, 0, 0))) & 128) != 0
    if defect == "stick-y":
        sy = np.zeros_like(sy)
    if not is3d:
        sz = np.zeros_like(sz)
    zx = z[0] | (cf & (sy | sz))
    zy = z[1] | (cf & (sx | sz))
    zz = z[2] | (cf & (sx | sy))
    return np.concatenate([zx, zy, zz] if is3d else [zx, zy], axis=1)


def set_wall_bcs_np(U, flags, is3d, defect=None):
    return np.where(wall_mask_np(flags, is3d, defect), np.float32(0), U)


# ---- the PCG scene: no fluid on the border, and a Dirichlet cell next to every fluid component -------------------------------
def singular_components(oracle, flags, is3d):
    """With the oracle's own labelling (findConnectedFluidComponents as solveLinearSystemPCG uses it): per sample, the multi-cell
    fluid components that touch no cell which is neither fluid nor obstacle (an empty, outflow, ... neighbour adds to the
    diagonal of setupLaplacian without a column: the Dirichlet condition that makes the component's system non-singular); the
    number of multi-cell components; and the mask of the one-cell components, which the solver skips (p stays 0 there)."""
    comp, n = oracle.findConnectedFluidComponents(flags, is3d)
    w = flags.astype(np.int64)
    assert np.array_equal(comp >= 0, (w & 1) != 0)
    near = np.zeros(flags.shape, bool)
    for _, d in scenes._faces(is3d):
        near |= (_nb(w, d) & 3) == 0          # (a neighbour outside the grid cannot occur: no fluid on the border)
    out, multi, single = [], 0, np.zeros(flags.shape, bool)
    for b in range(flags.shape[0]):
        bad = []
        for c in range(int(n[b])):
            m = comp[b, 0] == c
            if m.sum() == 1:
                single[b, 0] |= m
            else:
                multi += 1
                if not (near[b, 0] & m).any():
                    bad.append(c)
        out.append(bad)
    return out, multi, single


def pcg_scene(dims, seed, B=B, border=False):
    """alphabet scene for the PCG solver: fluid kept off the border, a modest velocity"""
    return scenes.alphabet_scene(dims, seed, B=B, border=border, vel_cells=1.0, noise=0.5)


def plume(Zt, words, seed, Y=20, X=24):
    """tests/test_hip_slab_methods.py's 3-D plume with a quarter of its interior fluid cells overwritten with `words`"""
    import test_hip_slab_methods as M
    b = M.scene(Zt, Y, X)
    rng = np.random.RandomState(seed)
    f = b["flags"]
    shell = scenes.border_mask(f.shape, True)
    pick = (rng.uniform(size=f.shape) < 0.25) & ~shell & (f == 1.0)
    w = np.asarray(words, np.float32)[rng.randint(len(words), size=f.shape)]
    f[pick] = w[pick]
    return b
