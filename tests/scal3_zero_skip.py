"""Cases and helpers of tests/test_hip_scal3_zero_skip.py (the short path of advectScalar's tile kernels for blocks whose
staged tile is all +0.0, fluidnet_amd/csrc/advect_scalar3.hip): scenes on a 70 x 13 x 11 grid with B = 2 -- two tile columns
in x, one of them ragged, interior and edge blocks in y and z, both block shapes the default picks (pass A 64 x 4 x 2 threads
on a halo-2 tile, pass B 64 x 4 threads x 2 planes on a halo-1 tile) -- a model of which blocks the kernels must find empty,
and the code that runs one case and records bits, temporaries and the EXPERIMENTS flavour's block counters."""
import hashlib
import itertools

import numpy as np

import scenes

DIMS, B, DT = (11, 13, 70), 2, 0.1          # (Z, Y, X)
TX, TY, PZ = 64, 4, 2                       # cells per block of either pass at this size
METHODS = ("maccormackOurs", "eulerOurs")
MODES = ("exact", "fast")
MASK_BITS = 0x7fc5a5a5
F = np.float32
# the interior block of pass A the single-cell cases walk around: cells x 0..63, y 4..7, z 4..5
BX, BY, BZ = (0, 63), (4, 7), (4, 5)


def base(dims=DIMS, batch=B, seed=3, vel_cells=0.2):
    """empty domain, density all +0.0, a smooth velocity with max |u dt| = vel_cells"""
    Z, Y, X = dims
    rng = np.random.RandomState(seed)
    U = scenes.smooth_field((batch, 3, Z, Y, X), rng)
    U *= vel_cells / DT / np.abs(U).max()
    return dict(s=np.zeros((batch, 1, Z, Y, X), F), U=np.ascontiguousarray(U, F), flags=scenes.empty_domain(batch, Z, Y, X, True))


def n_blocks(shape):
    Bn, _, Z, Y, X = shape
    return -(-X // TX) * -(-Y // TY) * -(-Z // PZ) * Bn


def zero_blocks(field, flags, halo):
    """blocks of a pass that stages `field` with this halo whose tile holds only +0.0 and mask words: every cell of the
    block's box + halo that lies inside the array and is fluid has the bit pattern 0 (a fluid word that happens to carry the
    mask word's bits counts as non-zero)"""
    Bn, _, Z, Y, X = field.shape
    nz = (field.view(np.uint32) != 0) & ((flags.astype(np.int64) & scenes.FLUID) != 0)
    n = 0
    for b, k0, y0, x0 in itertools.product(range(Bn), range(0, Z, PZ), range(0, Y, TY), range(0, X, TX)):
        box = nz[b, 0, max(k0 - halo, 0):k0 + PZ + halo, max(y0 - halo, 0):y0 + TY + halo, max(x0 - halo, 0):x0 + TX + halo]
        n += not box.any()
    return n


def single_cell_positions():
    """(z, y, x) of one non-zero cell: at distance 1 and 2 outside every face, edge and corner of the block (BX, BY, BZ), just
    inside it, and (x only: the block starts at the wall) at distance 3, outside pass A's halo"""
    xs = (1, 30, BX[1], BX[1] + 1, BX[1] + 2, BX[1] + 3)
    ys = (BY[0] - 2, BY[0] - 1, BY[0], BY[1], BY[1] + 1, BY[1] + 2)
    zs = (BZ[0] - 2, BZ[0] - 1, BZ[0], BZ[1], BZ[1] + 1, BZ[1] + 2)
    return list(itertools.product(zs, ys, xs))


def threshold_velocities(T):
    """(below, above): the largest float v with |fl(v * dt)| <= T and its successor, dt = fl(0.1) as the kernel multiplies"""
    dt = F(DT)
    v = F(T) / dt
    while np.abs(v * dt) > F(T):
        v = np.nextafter(v, F(0))
    while np.abs(np.nextafter(v, F(np.inf)) * dt) <= F(T):
        v = np.nextafter(v, F(np.inf))
    return v, np.nextafter(v, F(np.inf))


def cases(T=0.45):
    """name -> dict(s, U, flags): every case of the issue except the single-cell walk (single_cell_case)"""
    out = {}
    out["all_zero"] = base()
    out["golden_shape_all_zero"] = base(dims=(12, 14, 16), batch=1, seed=4)
    # one word of the halo of the otherwise empty block, in a fluid cell: -0.0, a denormal, +inf, a NaN
    for name, bits in (("neg_zero", 0x80000000), ("denormal", 0x00000001), ("inf", 0x7f800000), ("nan", 0x7fc00000)):
        c = base()
        c["s"].view(np.uint32)[0, 0, BZ[1] + 1, BY[1] + 1, 40] = bits
        c["s"].view(np.uint32)[1, 0, BZ[0] - 2, BY[0], 65] = bits
        out["word_" + name] = c
    # a 3 x 3 x 3 obstacle inside the zero region with a non-zero density inside it (the tile hides those cells), and an obstacle
    # cell next to the border shell
    c = base()
    c["flags"][:, 0, 4:7, 5:8, 20:23] = scenes.OBSTACLE
    c["s"][:, 0, 4:7, 5:8, 20:23] = 0.75
    c["flags"][0, 0, 1, 1, 1] = scenes.OBSTACLE
    c["flags"][1, 0, 5, 11, 68] = scenes.OBSTACLE
    c["s"][0, 0, 1, 1, 1] = -2.0
    c["s"][1, 0, 5, 11, 68] = 3.0
    out["obstacle_with_density"] = c
    # velocities on an all-zero density
    c = base()
    c["U"][...] = 0.0
    out["u_zero"] = c
    c = base()
    lo, hi = threshold_velocities(T)
    Z, Y, X = DIMS
    n = 0
    for k in range(1, Z - 1):
        for j in range(1, Y - 1):           # one cell per 64-lane row (= per wave and plane) in either tile column
            for i in (2 + (7 * j + 13 * k) % 58, 65 + (j + k) % 3):
                comp, v = n % 3, (lo, hi, -lo, -hi)[n % 4]
                n += 1
                idx = [k, j, i]
                c["U"][:, comp, k, j, i] = v
                idx[2 - comp] += 1
                c["U"][:, comp, idx[0], idx[1], idx[2]] = v          # both faces: the centred velocity is v exactly
    out["u_threshold"] = c
    c = base()
    c["U"][:, 0, 2:6, 2:9, 10:50] = 12.0       # |u dt| = 1.2: the generic trace
    c["U"][:, 2, 6:9, 5:11, 60:69] = -15.0
    out["u_long"] = c
    c = base()
    c["U"][0, 0, 5, 6, 33] = np.nan
    c["U"][1, 1, 3, 9, 66] = np.inf
    c["U"][0, 2, 8, 2, 5] = -np.inf
    out["u_nan_inf"] = c
    # item 0 empty, item 1 a dense smooth random field
    c = base()
    rng = np.random.RandomState(9)
    c["s"][1] = (np.abs(scenes.smooth_field((1, 1) + DIMS, rng)) + 0.1 + 0.05 * rng.rand(1, 1, *DIMS)).astype(F)[0]
    out["item1_dense"] = c
    return out


def single_cell_case(pos, value=1.0):
    c = base()
    z, y, x = pos
    c["s"][:, 0, z, y, x] = value
    return c


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(case, method, mode, device="cuda:0"):
    """one advectScalar call on the GPU: dict(out, fwd, bounds, counted = the EXPERIMENTS flavour's (pass A, pass B) counters,
    want = the blocks the model finds empty). fwd and bounds are the operator's temporaries (maccormackOurs only; the bounds of
    border cells are never written and are zeroed here)."""
    import torch
    from fluidnet_amd import tfluids
    dev = torch.device(device)
    s, U, flags = (torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("s", "U", "flags"))
    prev = tfluids.set_advect_mode(s, mode)
    try:
        tfluids.scal3ZeroBlocks(s)
        tfluids.advectScalar(DT, s, U, flags, method)
        counted = tfluids.scal3ZeroBlocks(s)
    finally:
        tfluids.set_advect_mode(s, prev)
    r = dict(out=s.cpu().numpy(), counted=counted, fwd=None, bounds=None)
    two_pass = method == "maccormackOurs"
    if two_pass:
        sh = tuple(flags.shape)
        sizes = [sh, sh, (sh[0], 3) + sh[2:], (sh[0], 3) + sh[2:]]
        tmp = tfluids.getTempStorage(s, sizes)
        r["fwd"] = tmp[0].cpu().numpy().copy()
        bounds = tmp[2][:, :2].cpu().numpy().copy()
        bounds[np.broadcast_to(scenes.border_mask(sh, True), bounds.shape)] = 0.0
        r["bounds"] = bounds
    r["want"] = (zero_blocks(case["s"], case["flags"], 2 if two_pass else 1), zero_blocks(r["fwd"], case["flags"], 1) if two_pass else 0)
    return r


def same_as_oracle(got, want):
    """np.array_equal as tests/test_hip_parity.py compares this operator, with NaN equal to NaN where the oracle yields one"""
    return np.array_equal(got, want, equal_nan=True)
