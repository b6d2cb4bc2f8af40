"""The data-set generator's scene arithmetic restated in numpy (fluidnet_amd/csrc/tfl_datagen.hpp): the
counter-based hash and its value map in uint32, the primitive rasteriser and the MAC-staggered curl in float32, every operation
in the order the header states, so that the kernels' bits can be asked for. The initial state and the stepped run on top of an
operator object (the oracle on the CPU), a plan checker, and the number of roundings behind the divergence bound of the curl."""
import numpy as np

SPHERE, BOX = 0, 1
F = np.float32


# ---- the hash -----------------------------------------------------------------------------------------------------------------
def noise_mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise_hash(seed, run, comp, cell):
    with np.errstate(over="ignore"):
        h = noise_mix(np.uint32((int(seed) + 0x9e3779b9) & 0xffffffff))
        h = noise_mix(h ^ np.uint32(int(run) & 0xffffffff))
        h = noise_mix(h ^ np.uint32(comp))
        return noise_mix(h ^ np.asarray(cell, np.uint32))


def noise_value(h):
    return ((h >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * F(1.0 / 8388608.0)


def noise_field(seed, run, C, dims, B=1):
    """tfl_noise_potential -> [B, C, Z, Y, X]; item b is run + b"""
    Z, Y, X = dims
    cell = np.arange(Z * Y * X, dtype=np.uint32)
    out = np.empty((B, C, Z, Y, X), np.float32)
    for b in range(B):
        for c in range(C):
            out[b, c] = noise_value(noise_hash(seed, int(run) + b, c, cell)).reshape(Z, Y, X)
    return out


# ---- the rasteriser -------------------------------------------------------------------------------------------------------------
def inside(prim, is3D, dims):
    Z, Y, X = dims
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    cx, cy, cz = i.astype(F) + F(0.5), j.astype(F) + F(0.5), k.astype(F) + F(0.5)
    a, b = [F(v) for v in prim["a"]], [F(v) for v in prim["b"]]
    if prim["kind"] == SPHERE:
        dx, dy = cx - a[0], cy - a[1]
        d2 = dx * dx + dy * dy
        if is3D:
            dz = cz - a[2]
            d2 = d2 + dz * dz
        return d2 <= b[0] * b[0]
    ins = (cx >= a[0]) & (cx <= b[0]) & (cy >= a[1]) & (cy <= b[1])
    return ins & (cz >= a[2]) & (cz <= b[2]) if is3D else ins


def scene_flags(obstacles, blobs, is3D, dims):
    """tfl_scene_flags -> (flags, density) [1, 1, Z, Y, X]"""
    Z, Y, X = dims
    flags = np.full((Z, Y, X), 2.0, np.float32)
    if is3D:
        flags[1:-1, 1:-1, 1:-1] = 1.0
    else:
        flags[:, 1:-1, 1:-1] = 1.0
    for o in obstacles:
        flags[inside(o, is3D, dims) & (flags == 1.0)] = 2.0
    rho = np.zeros((Z, Y, X), np.float32)
    for bl in blobs:
        rho[inside(bl, is3D, dims)] = F(bl["val"])
    rho[flags != 1.0] = 0.0
    return flags.reshape(1, 1, Z, Y, X), rho.reshape(1, 1, Z, Y, X)


# ---- the curl -------------------------------------------------------------------------------------------------------------------
def _plus(f, axis):
    """f(+1 along axis), the index clamped at the grid's end"""
    n = f.shape[axis]
    return np.take(f, np.minimum(np.arange(n) + 1, n - 1), axis=axis)


def curl_mac(psi, amp, is3D):
    """tfl_curl_mac: psi [1, 1 | 3, Z, Y, X] float32 -> U [1, 2 | 3, Z, Y, X]; axes of a [Z, Y, X] field: z = 0, y = 1, x = 2"""
    amp = F(amp)
    d = lambda f, axis: (_plus(f, axis) - f).astype(F)
    if not is3D:
        f = psi[0, 0]
        return np.stack([amp * d(f, 1), amp * (-d(f, 2))])[None].astype(F)
    px, py, pz = psi[0, 0], psi[0, 1], psi[0, 2]
    u = amp * (d(pz, 1) - d(py, 0)).astype(F)
    v = amp * (d(px, 0) - d(pz, 2)).astype(F)
    w = amp * (d(py, 2) - d(px, 1)).astype(F)
    return np.stack([u, v, w])[None].astype(F)


def curl_roundings_bound(is3D):
    """c of |div| <= c 2^-24 max|psi| for the MAC divergence (summed exactly) of curl_mac(psi, amp = 1). With M = max|psi| and
    e = 2^-24: a first difference is at most 2 M and is rounded once (error <= 2 M e). 2-D: a component IS one difference (the
    negation and the product with 1 are exact), and the divergence sums 4 components: 4 * 2 = 8. 3-D: a component is the
    difference of two first differences (errors 2 * 2 M e, carried through) and is at most 4 M (1 + e), rounded once more
    (<= 4 M e (1 + e)): 8 M e (1 + e) per component, 6 components: 48 (1 + e). The exact field's divergence is zero."""
    e = 2.0 ** -24
    return 8.0 if not is3D else 48.0 * (1.0 + e)


def mac_divergence64(U, is3D):
    """d_x u + d_y v (+ d_z w) in float64 on the cells that have all their plus-neighbours -> [Z', Y - 1, X - 1]"""
    U = U[0].astype(np.float64)
    zs = slice(0, U.shape[1] - 1) if is3D else slice(None)
    div = (U[0][zs, :-1, 1:] - U[0][zs, :-1, :-1]) + (U[1][zs, 1:, :-1] - U[1][zs, :-1, :-1])
    if is3D:
        div = div + (U[2][1:, :-1, :-1] - U[2][:-1, :-1, :-1])
    return div


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def check_plan(plan):
    """every primitive's cells inside the one-cell border (2 cells off it for obstacles and emitters), no emitter cell in an
    obstacle (nor next to one), the tables within the kernel's limit"""
    is3D, dims = plan["is3D"], plan["dims"]
    Z, Y, X = dims
    assert len(plan["obstacles"]) <= 32 and len(plan["blobs"]) <= 32
    border = np.ones(dims, bool)
    inner = (slice(2, Z - 2) if is3D else slice(None), slice(2, Y - 2), slice(2, X - 2))
    border[inner] = False
    flags, _ = scene_flags(plan["obstacles"], [], is3D, dims)
    obstacle = flags[0, 0] != 1.0
    if plan.get("voxels") is not None:
        assert plan["voxels"].shape == dims
        obstacle = obstacle | (plan["voxels"] != 0)
    for o in plan["obstacles"]:
        ins = inside(o, is3D, dims)
        assert ins.any() and not (ins & border).any(), o
    near = obstacle.copy()
    for ax in range(3):
        near |= np.roll(obstacle, 1, ax) | np.roll(obstacle, -1, ax)
    for e in plan["emitters"]:
        ins = inside(e, is3D, dims)
        assert ins.any() and not (ins & border).any() and not (ins & near).any(), e
    assert plan["speed"] * plan["dt"] <= 0.45 + 1e-6
    for e in plan["emitters"]:
        assert max(abs(v) for v in e["vel"]) * plan["dt"] <= 0.45 + 1e-6


# ---- the initial state and the run, on an operator object (oracle.OracleTfluids) ---------------------------------------------------
def initial_velocity(ops, plan, noise_seed):
    is3D, dims = plan["is3D"], plan["dims"]
    psi = noise_field(noise_seed[0], noise_seed[1], 3 if is3D else 1, dims)
    for _ in range(plan["noise_passes"]):
        dst = np.empty_like(psi)
        ops.rectangularBlur(psi, plan["noise_radius"], is3D, dst)
        psi = dst
    U1 = curl_mac(psi, 1.0, is3D)
    peak = F(np.abs(U1).max())
    amp = float(F(plan["speed"]) / peak) if peak > 0 else 0.0
    return curl_mac(psi, amp, is3D), amp


def init_state(ops, plan, noise_seed, pairs):
    """fluidnet_amd.datagen.init_state in numpy; pairs = datagen.emitter_pairs(plan)"""
    is3D, dims = plan["is3D"], plan["dims"]
    flags, density = scene_flags(plan["obstacles"], plan["blobs"], is3D, dims)
    if plan.get("voxels") is not None:
        occ = plan["voxels"].astype(bool).reshape(flags.shape)
        flags[occ], density[occ] = 2.0, 0.0
    U, _ = initial_velocity(ops, plan, noise_seed)
    U = np.ascontiguousarray(U)
    p, div = np.zeros_like(flags), np.zeros_like(flags)
    ops.setWallBcsForward(U, flags)
    ops.velocityDivergenceForward(U, flags, div)
    ops.solveLinearSystemPCG(p, flags, div, is3D, 1e-4, plan["maxIter"], "ic0")
    ops.velocityUpdateForward(U, flags, p)
    p[...] = 0.0
    batch = dict(pDiv=p, UDiv=U, flags=flags, density=density)
    (ubc, umk), (dbc, dmk) = pairs
    if ubc is not None:
        batch["UBC"], batch["UBCInvMask"] = ubc, umk
    if dbc is not None:
        batch["densityBC"], batch["densityBCInvMask"] = dbc, dmk
    return batch


def run_frames(ops, simulate_np, plan, gconf, mconf, noise_seed, pairs):
    """the generator's run by the definition's two-call form: per step copy the state, simulate(output_div=True) on the copy
    (the divergent frame), simulate on the state (the target frame) -> [(divergent, target)] of dicts p / U / flags / density"""
    batch = init_state(ops, plan, noise_seed, pairs)
    out = []
    for k in range(int(gconf["steps"])):
        if k % int(gconf["saveEvery"]) == 0:
            cp = {key: (v.copy() if key in ("pDiv", "UDiv", "density") else v) for key, v in batch.items()}
            simulate_np.simulate(ops, mconf, cp, None, output_div=True)
            divergent = dict(p=cp["pDiv"], U=cp["UDiv"], flags=cp["flags"], density=cp["density"])
        simulate_np.simulate(ops, mconf, batch, None)
        if k % int(gconf["saveEvery"]) == 0:
            out.append((divergent, dict(p=batch["pDiv"].copy(), U=batch["UDiv"].copy(), flags=batch["flags"], density=batch["density"].copy())))
    return out


# the generated sets of the tests: 2 runs x 6 saved frames, saveEvery = 2
GEN_SEED, GEN_RUNS = 11, 2
GEN_CASES = [(False, (1, 32, 32)), (True, (12, 16, 20))]


def gen_gconf(is3D, dims):
    from fluidnet_amd import datagen
    return datagen.default_gconf(is3D, dims, steps=12, saveEvery=2)
