"""Helper of tests/test_model_grad_cpu.py and tests/test_hip_model_backward.py: a differentiable restatement of the projection
net (torch/lib/model.lua:27-398) in torch on the CPU -- the yardstick of tfl_model_backward -- with the test models, scenes and
four mutants of the backward pass.

forward(): the graph with F.conv2d / F.conv3d, SetWallBcs, VelocityDivergence and VelocityUpdate restated as mask arithmetic
(one-sided differences by cell type), the three input-scale forms, the three non-linearities and the pressure skip, in the
dtype asked for (float64 = the yardstick; float32 = PyTorch-CPU's own fp32 answer, the witness). grads(): the parameter
gradients of sum(gradP p) + sum(gradU U) from torch.autograd. manual_grads(): the same gradients layer by layer in the
formulas of include/tfluids_hip.h tfl_model_backward, which can be broken on purpose (MUTANTS); unbroken it equals autograd.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import scenes

BAR = 1e-5          # per-tensor rel-L2: the project's standing parity bar for fp32 conv arithmetic (README)
TILE_X = 32         # the weight-gradient kernel's tile width (fluidnet_amd/csrc/tfl_train.hpp kWgTX)
MUTANTS = ("no-act-mask", "unmirrored-taps", "tap-off-by-one-in-last-x-tile", "no-scale")


# ---- models ---------------------------------------------------------------------------------------------------------
def _k5_skip(is3D):
    rng = np.random.RandomState(4)
    dim = 3 if is3D else 2
    shapes = [(8, 3, 5), (8, 8, 3), (1, 9, 1)]
    return [((rng.randn(co, ci, *([k] * dim)) * 0.3).astype(np.float32), (rng.randn(co) * 0.01).astype(np.float32))
            for co, ci, k in shapes]


def make_model(kind, is3D, opts=None, seed=3):
    """a FluidNetModel: 'default' | 'yang' (lib/model.lua's layer tables, seeded) | 'k5-skip' (8 k5, 8 k3, 1 k1 + addPressureSkip)"""
    from fluidnet_amd import FluidNetModel
    if kind == "k5-skip":
        return FluidNetModel(_k5_skip(is3D), is3D, opts=dict(opts or {}, addPressureSkip=True))
    m = FluidNetModel.from_mconf(dict(opts or {}, modelType=kind), is3D, seed=seed)
    if (opts or {}).get("nonlinType") == "sigmoid":
        # The seeded weights are small: every sigmoid output would sit within 0.05 of 0.5, a near-constant layer input, and
        # the weight gradients behind it would be sums that nearly cancel (ill-conditioned in fp32 for PyTorch as for anyone:
        # tests/test_model_grad_cpu.py). Six times the weights spread the activations over the sigmoid's range.
        m.layers = [(w * np.float32(6.0), b) for w, b in m.layers]
    return m


# (name, kind, is3D, opts, (B, Z, Y, X)). Shapes: ragged tiles in x and y, grids thinner than a kernel, batch.
S3 = [(2, 5, 7, 19), (1, 8, 12, 36), (1, 3, 4, 66)]
S2 = [(2, 1, 9, 33), (1, 1, 16, 64), (3, 1, 5, 130)]
CASES = [
    ("default3d-a", "default", True, None, S3[0]), ("default3d-b", "default", True, None, S3[1]),
    ("default3d-c", "default", True, None, S3[2]),
    ("default2d-a", "default", False, None, S2[0]), ("default2d-b", "default", False, None, S2[1]),
    ("default2d-c", "default", False, None, S2[2]),
    ("yang3d", "yang", True, None, S3[0]), ("yang2d", "yang", False, None, S2[2]),
    ("k5-skip3d", "k5-skip", True, None, S3[1]), ("k5-skip2d", "k5-skip", False, None, S2[0]),
    # one model per opts switch
    ("norm-off", "default", False, dict(normalizeInput=False), S2[0]),
    ("norm-l2-pdiv", "default", True, dict(normalizeInputFunc="norm", normalizeInputChan="pDiv"), S3[2]),
    ("norm-std-div", "default", False, dict(normalizeInputChan="div"), S2[2]),
    ("relu6", "default", False, dict(nonlinType="relu6"), S2[0]),
    ("sigmoid", "default", True, dict(nonlinType="sigmoid"), S3[0]),
    ("skip-default", "default", False, dict(addPressureSkip=True), S2[1]),
    ("udiv-with-pdiv", "default", True, dict(inputChannels=dict(UDiv=True)), S3[0]),
    ("udiv-without-pdiv", "default", False, dict(inputChannels=dict(UDiv=True, pDiv=False)), S2[0]),
]
NAMES = [c[0] for c in CASES]
GRAD_MODES = ("both", "p-only", "u-only")


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """(pDiv, UDiv, flags, gradP, gradU) of a case, read-only. White-noise fields (a tap that reads the wrong voxel is off by
    O(1)), salt-and-pepper obstacles, a box of obstacle cells whose corner sits on the weight-gradient kernel's tile edge
    (x = 32 where the grid reaches it, y = 8), and the border obstacle cells of emptyDomain."""
    i = NAMES.index(name)
    B, Z, Y, X = CASES[i][4]
    sc = scenes.rough_scene((Z, Y, X), seed=300 + i, B=B, obstacle_frac=0.08)
    f = sc["flags"]
    x0 = 31 if X > 34 else max(1, X // 2 - 1)
    y0 = 7 if Y > 10 else max(1, Y // 2 - 1)
    z0 = slice(1, Z - 1) if Z > 2 else slice(0, 1)
    f[:, :, z0, y0:y0 + 2, x0:x0 + 2] = scenes.OBSTACLE
    rng = np.random.RandomState(900 + i)
    # (gradP with a mean: the last layer's gradBias is the plain sum of the gradient at pPred, to which the gradU part adds
    # terms that cancel exactly -- see rel_l2_per_tensor -- so a zero-mean gradP would leave that one tensor ill-conditioned)
    gP = (rng.randn(*sc["p"].shape) + 0.5).astype(np.float32)
    gU = rng.randn(*sc["U"].shape).astype(np.float32)
    out = (sc["p"], sc["U"], np.ascontiguousarray(f), gP, gU)
    for t in out:
        t.setflags(write=False)
    return out


# ---- the restated operators -------------------------------------------------------------------------------------------
def _bits(flags):
    f = flags.astype(np.int64)
    return dict(fluid=(f & scenes.FLUID) != 0, obst=(f & scenes.OBSTACLE) != 0, empty=(f & scenes.EMPTY) != 0,
                outflow=(f & scenes.OUTFLOW) != 0, stick=(f & scenes.STICK) != 0)


def _prev(a, axis):
    """a at the minus-neighbour along `axis` (False / 0 where there is none)"""
    out = np.zeros_like(a)
    idx_dst = [slice(None)] * a.ndim
    idx_src = [slice(None)] * a.ndim
    idx_dst[axis] = slice(1, None)
    idx_src[axis] = slice(0, -1)
    out[tuple(idx_dst)] = a[tuple(idx_src)]
    return out


def _next(a, axis):
    return np.flip(_prev(np.flip(a, axis), axis), axis)


def wall_keep_mask(flags, is3D):
    """[B, C, Z, Y, X] of 0 / 1: the components setWallBcsForward leaves (tfluids.cc:926-1002)"""
    b = _bits(flags[:, 0])
    C = 3 if is3D else 2
    axes = [3, 2, 1][:C]          # x, y, z axes of a [B, Z, Y, X] array
    act = b["fluid"] | b["obst"]
    zero = []
    for c in range(C):
        ax = axes[c]
        has_prev = np.ones_like(act)
        idx = [slice(None)] * 4
        idx[ax] = 0
        has_prev[tuple(idx)] = False
        z = act & has_prev & (_prev(b["obst"], ax) | (b["obst"] & _prev(b["fluid"], ax)))
        zero.append(z)
    for c in range(C):            # stick neighbours along c zero the OTHER components of a fluid cell
        ax = axes[c]
        st = b["fluid"] & (_prev(b["stick"], ax) | _next(b["stick"], ax))
        for o in range(C):
            if o != c:
                zero[o] = zero[o] | st
    return np.stack([~z for z in zero], axis=1).astype(np.float64)


def _interior(shape, is3D):
    m = np.zeros(shape, bool)
    if is3D:
        m[:, 1:-1, 1:-1, 1:-1] = True
    else:
        m[:, :, 1:-1, 1:-1] = True
    return m


def _shift_next(t, dim):
    """t at the plus-neighbour along dim (wraps: only read at interior cells)"""
    return torch.roll(t, -1, dim)


def _shift_prev(t, dim):
    return torch.roll(t, 1, dim)


def divergence(U, flags, is3D):
    """velocityDivergenceForward (tfluids.cc:1008-1066) of a [B, C, Z, Y, X] tensor"""
    b = _bits(flags[:, 0])
    on = torch.from_numpy((b["fluid"] & _interior(b["fluid"].shape, is3D)).astype(np.float64)).to(U.dtype)
    d = (U[:, 0] - _shift_next(U[:, 0], 3)) + (U[:, 1] - _shift_next(U[:, 1], 2))
    if is3D:
        d = d + (U[:, 2] - _shift_next(U[:, 2], 1))
    return (d * on).unsqueeze(1)


def velocity_update(U, p, flags, is3D):
    """velocityUpdateForward (tfluids.cc:1072-1156): U [B, C, ..] minus the one-sided pressure difference by cell type"""
    b = _bits(flags[:, 0])
    inner = _interior(b["fluid"].shape, is3D)
    C = 3 if is3D else 2
    axes = [3, 2, 1][:C]
    fl = b["fluid"] & inner
    em = b["empty"] & ~b["outflow"] & ~b["fluid"] & inner
    T = lambda m: torch.from_numpy(m.astype(np.float64)).to(U.dtype)
    pc = p[:, 0]
    out = []
    for c in range(C):
        ax = axes[c]
        pf, pe = _prev(b["fluid"], ax), _prev(b["empty"], ax)
        pp = _shift_prev(pc, ax)
        u = U[:, c]
        u = u - T(fl & pf) * (pc - pp) - T(fl & pe) * pc
        u = u * T(~(em & ~pf)) + T(em & pf) * pp
        out.append(u)
    return torch.stack(out, dim=1)


def occupancy(flags):
    b = _bits(flags)
    return np.where(b["fluid"], 0.0, np.where(b["obst"], 1.0, -1.0))


def _act(h, nonlin):
    return {"relu": torch.relu, "relu6": lambda t: torch.clamp(t, 0.0, 6.0), "sigmoid": torch.sigmoid}[nonlin](h)


def _conv(h, w, b, is3D):
    pad = (w.shape[-1] - 1) // 2
    return F.conv3d(h, w, b, padding=pad) if is3D else F.conv2d(h[:, :, 0], w, b, padding=pad).unsqueeze(2)


def _head(pDiv, UDiv, flags, opts, is3D, dtype):
    """what the conv stack is fed: (x, skip, scale [B,1,1,1,1], U_bc), all constants of the parameters"""
    from fluidnet_amd.model import _resolve_opts
    o = _resolve_opts(opts)
    ic = o["inputChannels"]
    T = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    U_bc = T(UDiv) * T(wall_keep_mask(flags, is3D))
    div = divergence(U_bc, flags, is3D)
    p = T(pDiv)
    B = p.shape[0]
    if o["normalizeInput"]:
        src = {"UDiv": U_bc, "pDiv": p, "div": div}[o["normalizeInputChan"]].reshape(B, -1)
        n = src.shape[1]
        if o["normalizeInputFunc"] == "std":
            scale = torch.sqrt((n * (src * src).sum(1) - src.sum(1) ** 2) / (n * (n - 1.0)))
        else:
            scale = torch.sqrt((src * src).sum(1))
    else:
        scale = torch.ones(B, dtype=dtype)
    sc = scale.reshape(-1, 1, 1, 1, 1)
    chans = []
    if ic["pDiv"]:
        chans.append(p / sc)
    if ic["UDiv"]:
        chans.append(U_bc / sc)
    if ic["div"]:
        chans.append(div / sc)
    chans.append(T(occupancy(flags)))
    skip = p / sc if o["addPressureSkip"] else None
    return torch.cat(chans, dim=1), skip, sc, U_bc, o


def _tail(pPred, sc, U_bc, flags, is3D):
    """(p, U) from the last layer's output (model.lua:372-390)"""
    keep = torch.from_numpy(wall_keep_mask(flags, is3D)).to(pPred.dtype)
    U = velocity_update(U_bc / sc, pPred, flags, is3D) * sc
    return pPred * sc, U * keep


def forward(layers, pDiv, UDiv, flags, opts=None, dtype=torch.float64):
    """(p, U, params): the model's outputs as torch tensors and the leaf parameter tensors [(w, b)] they depend on"""
    is3D = UDiv.shape[1] == 3
    x, skip, sc, U_bc, o = _head(pDiv, UDiv, flags, opts, is3D, dtype)
    params = [(torch.from_numpy(np.asarray(w)).to(dtype).requires_grad_(True), torch.from_numpy(np.asarray(b)).to(dtype).requires_grad_(True))
              for w, b in layers]
    h = x
    for l, (w, b) in enumerate(params):
        last = l + 1 == len(params)
        if last and skip is not None:
            h = torch.cat([h, skip], dim=1)
        h = _conv(h, w, b, is3D)
        if _PRE is not None:
            _PRE.append(h)    # (the layers' pre-activation outputs, for grads(l1=True))
        if not last:
            h = _act(h, o["nonlinType"])
    p, U = _tail(h, sc, U_bc, flags, is3D)
    return p, U, params


_PRE = None


def grads(layers, pDiv, UDiv, flags, gradP, gradU, opts=None, dtype=torch.float64, l1=False):
    """[(gradWeight, gradBias)] as float64 numpy arrays: d/dparams of sum(gradP p) + sum(gradU U) (either may be None).
    l1: also, per layer, the L1 norm of the gradient at its pre-activation output (the summands of its gradBias)."""
    global _PRE
    _PRE = pre = []
    try:
        p, U, params = forward(layers, pDiv, UDiv, flags, opts, dtype)
    finally:
        _PRE = None
    T = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    loss = p.sum() * 0
    if gradP is not None:
        loss = loss + (p * T(gradP)).sum()
    if gradU is not None:
        loss = loss + (U * T(gradU)).sum()
    flat = [t for wb in params for t in wb]
    g = torch.autograd.grad(loss, flat + pre)
    out = [(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(len(params))]
    return (out, [float(t.abs().sum()) for t in g[len(flat):]]) if l1 else out


def manual_grads(layers, pDiv, UDiv, flags, gradP, gradU, opts=None, mutant=None, dtype=torch.float64):
    """The same gradients by the layer-by-layer formulas, optionally broken:
      no-act-mask                     g_pre = g_out, the activation's derivative left out
      unmirrored-taps                 the data gradient convolves with W transposed but NOT mirrored
      tap-off-by-one-in-last-x-tile   tap 0 of every gradWeight reads x one voxel to the right for the positions of the last,
                                      ragged 32-wide x-tile (nothing changes where X is a multiple of 32)
      no-scale                        g_pPred formed as if the input scale were 1
    """
    assert mutant is None or mutant in MUTANTS
    is3D = UDiv.shape[1] == 3
    with torch.no_grad():
        x, skip, sc, U_bc, o = _head(pDiv, UDiv, flags, opts, is3D, dtype)
        ws = [(torch.from_numpy(np.asarray(w)).to(dtype), torch.from_numpy(np.asarray(b)).to(dtype)) for w, b in layers]
        xs, ys, h = [], [], x
        for l, (w, b) in enumerate(ws):
            last = l + 1 == len(ws)
            if last and skip is not None:
                h = torch.cat([h, skip], dim=1)
            xs.append(h)
            h = _conv(h, w, b, is3D)
            if not last:
                h = _act(h, o["nonlinType"])
            ys.append(h)
    # g at pPred: the tail is linear in pPred, so autograd of the tail alone is its exact transpose
    pPred = ys[-1].clone().requires_grad_(True)
    p, U = _tail(pPred, torch.ones_like(sc) if mutant == "no-scale" else sc, U_bc, flags, is3D)
    T = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    loss = p.sum() * 0
    if gradP is not None:
        loss = loss + (p * T(gradP)).sum()
    if gradU is not None:
        loss = loss + (U * T(gradU)).sum()
    g = torch.autograd.grad(loss, pPred)[0]
    out = [None] * len(ws)
    nd = 3 if is3D else 2
    with torch.no_grad():
        for l in range(len(ws) - 1, -1, -1):
            w, _ = ws[l]
            if l + 1 < len(ws) and mutant != "no-act-mask":
                y = ys[l]
                d = {"relu": (y > 0).to(dtype), "relu6": ((y > 0) & (y < 6)).to(dtype), "sigmoid": y * (1 - y)}[o["nonlinType"]]
                g = g * d
            xin = xs[l]
            k = w.shape[-1]
            r = (k - 1) // 2
            sq = (lambda t: t) if is3D else (lambda t: t[:, :, 0])
            conv = F.conv3d if is3D else F.conv2d
            # gradWeight[co][ci][tap] = sum x[ci][pos + tap] g[co][pos]: a convolution of x by g with the batch as channels
            gw = conv(sq(xin).transpose(0, 1), sq(g).transpose(0, 1), padding=r).transpose(0, 1)
            X = xin.shape[-1]
            x_tail = (X // TILE_X) * TILE_X
            if mutant == "tap-off-by-one-in-last-x-tile" and x_tail < X:
                # tap 0 = offset (-r, -r, -r): redo it with the positions x >= x_tail reading one voxel further right
                pad = [r, r + 1] + [r, r] * (nd - 1)
                xp = F.pad(sq(xin), pad)
                sizes = xin.shape[2:] if is3D else xin.shape[3:]
                def window(off):
                    idx = [slice(None), slice(None)] + [slice(0, s) for s in sizes[:-1]] + [slice(off, off + sizes[-1])]
                    return xp[tuple(idx)]
                xa, xb = window(0).clone(), window(1)
                xa[..., x_tail:] = xb[..., x_tail:]
                dims = "zyx"[3 - nd:]
                gw[(slice(None), slice(None)) + (0,) * nd] = torch.einsum("bc%s,bo%s->oc" % (dims, dims), xa, sq(g))
            gb = g.sum(dim=[0, 2, 3, 4])
            out[l] = (gw.double().numpy(), gb.double().numpy())
            if l > 0:
                wt = w.transpose(0, 1)
                if mutant != "unmirrored-taps":
                    wt = wt.flip(list(range(2, 2 + nd)))
                g = conv(sq(g), wt, padding=r)
                if not is3D:
                    g = g.unsqueeze(2)
                if l + 1 == len(ws) and skip is not None:
                    g = g[:, :-1]          # the joined pDiv/scale channel: its data gradient is dropped
    return out


def rel_l2_per_tensor(got, want, zero_l1=None):
    """[(rel-L2 of gradWeight, rel-L2 of gradBias)] per layer.
    zero_l1 (the gradU-only runs only: the L1 norm of the gradient at pPred): the LAST layer's gradBias is then zero by
    construction -- the velocity update reads only differences of pPred between fluid cells (the test scenes have no empty
    cells: the net's occupancy input does not take them), so a constant added to pPred changes no output. The float64 yardstick
    holds rounding noise of 1e-15 there, and a relative error against it is undefined. That one tensor is the plain sum of the
    gradient at pPred over all voxels, so it is held to the same bar relative to that sum's condition instead:
    |got - want| <= BAR * sum |g_pPred|. Every other tensor, in every run, is held to plain rel-L2."""
    out = [(scenes.rel_l2(gw, ww), scenes.rel_l2(gb, wb)) for (gw, gb), (ww, wb) in zip(got, want)]
    if zero_l1 is not None:
        gb, wb = np.asarray(got[-1][1], np.float64), np.asarray(want[-1][1], np.float64)
        out[-1] = (out[-1][0], float(np.abs(gb - wb).max() / zero_l1))
    return out


def worst(got, want, zero_l1=None):
    return max(max(pair) for pair in rel_l2_per_tensor(got, want, zero_l1))


def mutant_applies(mutant, layers, opts, X):
    """does the mutant change anything for this model / grid at all"""
    from fluidnet_amd.model import _resolve_opts
    if mutant == "unmirrored-taps":
        return any(w.shape[-1] > 1 for w, _ in layers[1:])          # mirroring one tap is the identity
    if mutant == "tap-off-by-one-in-last-x-tile":
        return X % TILE_X != 0
    if mutant == "no-scale":
        return bool(_resolve_opts(opts)["normalizeInput"])
    return len(layers) > 1


@functools.lru_cache(maxsize=None)
def expected(name, mode="both"):
    """(the fp64 gradients of a case, PyTorch-CPU-fp32's, zero_l1 for rel_l2_per_tensor: set in the gradU-only mode alone);
    computed once per process, treat as read-only"""
    _, kind, is3D, opts, _ = case(name)
    m = make_model(kind, is3D, opts)
    pDiv, UDiv, flags, gP, gU = make_inputs(name)
    gP = None if mode == "u-only" else gP
    gU = None if mode == "p-only" else gU
    g64, l1 = grads(m.layers, pDiv, UDiv, flags, gP, gU, m.opts, torch.float64, l1=True)
    return g64, grads(m.layers, pDiv, UDiv, flags, gP, gU, m.opts, torch.float32), (l1[-1] if mode == "u-only" else None)


# ---- the closed loop: ProjectionNet + FluidCriterion + plain SGD ------------------------------------------------------
# 2-D 32 x 32, B = 2; targets by a Jacobi projection (calcPUTargets). LR and STEPS were chosen on the CPU with the fp64
# restatement so that its loss falls by at least half (tests/test_model_grad_cpu.py holds that).
LOOP = dict(dims=(1, 32, 32), B=2, seed=77, lambdas=(1.0, 1.0, 1.0), lr=0.005, steps=20, jacobi_iters=50, gain=3.0)


def loop_scene():
    sc = scenes.make_scene(LOOP["dims"], seed=LOOP["seed"], B=LOOP["B"], vel_cells=0.4)
    return sc["p"] * 0, sc["U"], sc["flags"]


def loop_model():
    """the seeded 2-D default net with `gain` times its weights (the seeded ones leave SGD on a plateau for its first steps)"""
    m = make_model("default", False, seed=5)
    m.layers = [(w * np.float32(LOOP["gain"]), b) for w, b in m.layers]
    return m


def criterion_loss(p, U, pT, UT, flags, lambdas):
    """nn.FluidCriterion without a border weight, sizeAverage: lambda-weighted MSE of p, U and the divergence of U"""
    is3D = U.shape[1] == 3
    lp, lu, ld = lambdas
    T = lambda a: torch.from_numpy(np.array(a)).to(p.dtype)
    return lp * ((p - T(pT)) ** 2).mean() + lu * ((U - T(UT)) ** 2).mean() + ld * (divergence(U, flags, is3D) ** 2).mean()


def train_loop(layers, opts, pDiv, UDiv, flags, pT, UT, lambdas, lr, steps, dtype=torch.float64):
    """plain SGD on the restatement: ([loss before each step] + [loss after the last], [params after each step])"""
    cur = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in layers]
    losses, history = [], []
    for _ in range(steps):
        p, U, params = forward(cur, pDiv, UDiv, flags, opts, dtype)
        loss = criterion_loss(p, U, pT, UT, flags, lambdas)
        flat = [t for wb in params for t in wb]
        g = torch.autograd.grad(loss, flat)
        losses.append(float(loss.detach()))
        cur = [((params[i][0] - lr * g[2 * i]).detach().double().numpy(), (params[i][1] - lr * g[2 * i + 1]).detach().double().numpy())
               for i in range(len(params))]
        history.append(cur)
    with torch.no_grad():
        p, U, _ = forward(cur, pDiv, UDiv, flags, opts, dtype)
        losses.append(float(criterion_loss(p, U, pT, UT, flags, lambdas)))
    return losses, history
