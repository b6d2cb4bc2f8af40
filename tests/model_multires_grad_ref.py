"""Helper of tests/test_model_multires_grad_cpu.py and tests/test_hip_model_multires_backward.py: the differentiable restatement
of tests/model_grad_ref.py for linear models whose resolution changes -- 2x average pooling behind a layer and
nn.{Spatial,Volumetric}ConvolutionUpsample (lib/modules/spatial_convolution_upsample.lua:47-108, restated as in
oracle/simulate_np.py: view / permute) -- i.e. the `tog` layer tables and custom ones. The yardstick of the training pass that
tfl_model_enable_multires_training switches on.

The graph is held in torch on the CPU: F.conv*, F.avg_pool*, the view / permute shuffle, model_input_grad_ref's head (pDiv and
UDiv may be leaves) and model_grad_ref's tail. float64 = the yardstick; float32 = PyTorch's own answer, the witness.
manual_grads() restates, layer by layer, the formulas the kernels implement (pool backward fused with the mask, the strided
weight gradient of the inner convolution, the data gradient summed over the sub-positions) and can be broken on purpose.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import model_grad_ref as R
import model_input_grad_ref as IR
import scenes

BAR = R.BAR
GRAD_MODES = R.GRAD_MODES
MUTANTS = ("pool-without-scale", "pool-one-child", "mask-before-shuffle", "sub-positions-transposed", "dgrad-sub0-only")


# ---- models and cases ---------------------------------------------------------------------------------------------------
def _custom(is3D, nonlin):
    """[8 k3 pool 2, 8 k3, 8 k1 up 2, 1 k3]: an upsample layer that is followed by an activation and is not the last"""
    from fluidnet_amd import FluidNetModel
    rng = np.random.RandomState(11)
    dim = 3 if is3D else 2
    S = 2 ** dim
    gain = 6.0 if nonlin == "sigmoid" else 1.0      # (model_grad_ref.make_model: spread the activations over the sigmoid's range)
    layers = []
    for co, ci, k, u in [(8, 3, 3, 1), (8, 8, 3, 1), (8, 8, 1, 2), (1, 8, 3, 1)]:
        w = (rng.randn(co * (S if u > 1 else 1), ci, *([k] * dim)) * gain * np.sqrt(2.0 / (ci * k ** dim))).astype(np.float32)
        b = (rng.randn(co * (S if u > 1 else 1)) * 0.05).astype(np.float32)
        layers.append((w, b))
    return FluidNetModel(layers, is3D, pool=[2, 1, 1, 1], up=[1, 1, 2, 1], opts=dict(nonlinType=nonlin))


def make_model(kind, is3D):
    """'tog' (lib/model.lua's layer tables, seeded) | 'custom-relu6' | 'custom-sigmoid'"""
    from fluidnet_amd import FluidNetModel
    if kind == "tog":
        return FluidNetModel.tog(is3D, seed=3, scale=1.0)
    return _custom(is3D, kind.split("-")[1])


# (name, kind, is3D, (B, Z, Y, X)): the smallest shapes at which each path can go wrong (the issue's table)
CASES = [
    ("tog3d-a", "tog", True, (2, 4, 8, 36)),        # one plane at the coarsest level; tile edge at x = 32 on the fine level
    ("tog3d-b", "tog", True, (1, 8, 12, 68)),       # ragged third x-tile fine, ragged second tile at half resolution (34), Y/4 = 3
    ("tog2d-a", "tog", False, (2, 1, 10, 34)),
    ("tog2d-b", "tog", False, (1, 1, 16, 64)),
    ("tog2d-c", "tog", False, (3, 1, 6, 132)),      # half resolution 66: ragged tile on the coarse level
    ("custom2d-relu6", "custom-relu6", False, (2, 1, 10, 68)),
    ("custom2d-sigmoid", "custom-sigmoid", False, (2, 1, 10, 68)),
    ("custom3d-relu6", "custom-relu6", True, (1, 4, 10, 36)),
    ("custom3d-sigmoid", "custom-sigmoid", True, (1, 4, 10, 36)),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def model_of(name):
    _, kind, is3D, _ = case(name)
    return make_model(kind, is3D)


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """(pDiv, UDiv, flags, gradP, gradU), read-only: model_grad_ref.make_inputs' kind -- white noise, salt-and-pepper obstacles, a
    box of obstacle cells whose corner sits on the weight-gradient kernel's tile edge (x = 32 where the grid reaches it, y = 8)"""
    i = NAMES.index(name)
    B, Z, Y, X = CASES[i][3]
    sc = scenes.rough_scene((Z, Y, X), seed=700 + i, B=B, obstacle_frac=0.08)
    f = sc["flags"]
    x0 = 31 if X > 34 else max(1, X // 2 - 1)
    y0 = 7 if Y > 10 else max(1, Y // 2 - 1)
    z0 = slice(1, Z - 1) if Z > 2 else slice(0, 1)
    f[:, :, z0, y0:y0 + 2, x0:x0 + 2] = scenes.OBSTACLE
    rng = np.random.RandomState(1300 + i)
    gP = (rng.randn(*sc["p"].shape) + 0.5).astype(np.float32)
    gU = rng.randn(*sc["U"].shape).astype(np.float32)
    out = (sc["p"], sc["U"], np.ascontiguousarray(f), gP, gU)
    for t in out:
        t.setflags(write=False)
    return out


# ---- the restated graph -------------------------------------------------------------------------------------------------
def _T(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)


def shuffle(h, u, is3D):
    """the reference's view / permute on a [B, C u^dim, Z, Y, X] tensor (2-D: Z = 1 stays)"""
    b = h.shape[0]
    if is3D:
        no, (t, hh, ww) = h.shape[1] // u ** 3, h.shape[2:]
        return h.view(b, no, u, u, u, t, hh, ww).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(b, no, t * u, hh * u, ww * u)
    no, (hh, ww) = h.shape[1] // u ** 2, h.shape[3:]
    return h[:, :, 0].view(b, no, u, u, hh, ww).permute(0, 1, 4, 2, 5, 3).reshape(b, no, 1, hh * u, ww * u)


def unshuffle(g, u, is3D, transposed=False):
    """the shuffle's transpose (= its inverse): fine [B, C, uZ, uY, uX] -> [B, C u^dim, Z, Y, X], channel co u^dim + sub with
    sub = (sz u + sy) u + sx. transposed: the mutant, sy <-> sx (3-D: sz <-> sx)"""
    b, no = g.shape[:2]
    if is3D:
        t, hh, ww = [s // u for s in g.shape[2:]]
        perm = (0, 1, 7, 5, 3, 2, 4, 6) if transposed else (0, 1, 3, 5, 7, 2, 4, 6)
        return g.view(b, no, t, u, hh, u, ww, u).permute(*perm).reshape(b, no * u ** 3, t, hh, ww)
    hh, ww = [s // u for s in g.shape[3:]]
    perm = (0, 1, 5, 3, 2, 4) if transposed else (0, 1, 3, 5, 2, 4)
    return g[:, :, 0].view(b, no, hh, u, ww, u).permute(*perm).reshape(b, no * u * u, 1, hh, ww)


def _pool(h, is3D):
    return F.avg_pool3d(h, 2) if is3D else F.avg_pool2d(h[:, :, 0], 2).unsqueeze(2)


def _unpool(g, is3D):
    """every coarse cell over its 2^dim children (no scale)"""
    for ax in ([2, 3, 4] if is3D else [3, 4]):
        g = g.repeat_interleave(2, dim=ax)
    return g


def stack(params, pool, up, x, nonlin, is3D, keep=None):
    """the conv stack: pPred from the net input. keep: a dict that receives xs (layer inputs), ys (post-activation outputs at
    the convolution's output resolution, behind the shuffle, in front of the pool)"""
    h, xs, ys = x, [], []
    for l, (w, b) in enumerate(params):
        last = l + 1 == len(params)
        xs.append(h)
        h = R._conv(h, w, b, is3D)
        if up[l] > 1:
            h = shuffle(h, up[l], is3D)
        if not last:
            h = R._act(h, nonlin)
        ys.append(h)
        if pool[l] > 1:
            h = _pool(h, is3D)
    if keep is not None:
        keep.update(xs=xs, ys=ys)
    return h


def net(m, params, p, Ud, flags, keep=None):
    x, _, sc, U_bc, o = IR.head(p, Ud, flags, m.opts, m.is3D)
    pPred = stack(params, m.pool, m.up, x, o["nonlinType"], m.is3D, keep)
    if keep is not None:
        keep.update(x=x, sc=sc, U_bc=U_bc, o=o, pPred=pPred)
    return R._tail(pPred, sc, U_bc, flags, m.is3D)


def _mode(name, mode):
    _, _, _, gP, gU = make_inputs(name)
    return (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


@functools.lru_cache(maxsize=None)
def grads(name, mode="both", dtype=torch.float64):
    """([(gradWeight, gradBias)], (gradPDiv, gradUDiv), L1 norm of the gradient at pPred) of sum(gradP p) + sum(gradU U) by
    torch.autograd, float64 numpy; computed once per process, read-only"""
    m = model_of(name)
    pDiv, UDiv, flags, _, _ = make_inputs(name)
    gP, gU = _mode(name, mode)
    params = IR._params(m.layers, dtype, grad=True)
    p0, U0 = _T(pDiv, dtype).requires_grad_(True), _T(UDiv, dtype).requires_grad_(True)
    keep = {}
    p, U = net(m, params, p0, U0, flags, keep)
    flat = [t for wb in params for t in wb]
    g = torch.autograd.grad(IR._loss(p, U, gP, gU), flat + [p0, U0, keep["pPred"]], allow_unused=True)
    n = len(params)
    par = [(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(n)]
    inp = tuple((torch.zeros_like(t) if gi is None else gi).double().numpy() for gi, t in zip(g[2 * n:2 * n + 2], (p0, U0)))
    for a in [t for wb in par for t in wb] + list(inp):
        a.setflags(write=False)
    return par, inp, float(g[2 * n + 2].abs().sum())


def manual_grads(name, mode="both", mutant=None, dtype=torch.float64):
    """([(gradWeight, gradBias)], (gradPDiv, gradUDiv)) by the layer-by-layer formulas of DESIGN.md 3.26, optionally broken:
      pool-without-scale         the pool's backward hands every child the whole gradient, the 1 / 2^dim left out
      pool-one-child             ... hands the gradient (times 1 / 2^dim) to child (0, 0, 0) only
      mask-before-shuffle        an upsample layer's activation mask taken on the inner convolution's channels, in front of the shuffle
      sub-positions-transposed   the un-shuffle reads sub-position (sz, sy, sx) where (sz, sx, sy) [3-D: (sx, sy, sz)] belongs
      dgrad-sub0-only            an upsample layer's data gradient from sub-position 0 alone
    The head in front of the first layer's data gradient is model_input_grad_ref's business: here it is autograd's, fed g_x."""
    assert mutant is None or mutant in MUTANTS
    m = model_of(name)
    is3D = m.is3D
    pDiv, UDiv, flags, _, _ = make_inputs(name)
    gP, gU = _mode(name, mode)
    nd = 3 if is3D else 2
    with torch.no_grad():
        ws = IR._params(m.layers, dtype)
        keep = {}
        net(m, ws, _T(pDiv, dtype), _T(UDiv, dtype), flags, keep)
    xs, ys, o = keep["xs"], keep["ys"], keep["o"]
    # the gradient at pPred and the direct paths of the tail, by autograd of head + tail alone (pPred a constant)
    p0, U0 = _T(pDiv, dtype).requires_grad_(True), _T(UDiv, dtype).requires_grad_(True)
    x, _, sc, U_bc, _ = IR.head(p0, U0, flags, m.opts, is3D)
    pp = keep["pPred"].clone().requires_grad_(True)
    p, U = R._tail(pp, sc, U_bc, flags, is3D)
    loss = IR._loss(p, U, gP, gU)
    g = torch.autograd.grad(loss, pp, retain_graph=True)[0]
    sq = (lambda t: t) if is3D else (lambda t: t[:, :, 0])
    un = (lambda t: t) if is3D else (lambda t: t.unsqueeze(2))
    conv = F.conv3d if is3D else F.conv2d
    dact = lambda y: {"relu": (y > 0).to(dtype), "relu6": ((y > 0) & (y < 6)).to(dtype), "sigmoid": y * (1 - y)}[o["nonlinType"]]
    out = [None] * len(ws)
    with torch.no_grad():
        for l in range(len(ws) - 1, -1, -1):
            w, _ = ws[l]
            last, u = l + 1 == len(ws), m.up[l]
            S = u ** nd
            if m.pool[l] > 1:      # one pass: un-pool, scale, mask
                if mutant == "pool-one-child":
                    z = torch.zeros_like(ys[l])
                    z[:, :, ::(2 if is3D else 1), ::2, ::2] = g
                    g = z
                else:
                    g = _unpool(g, is3D)
                if mutant != "pool-without-scale":
                    g = g / 2 ** nd
                g = g * dact(ys[l])
            elif not last and not (u > 1 and mutant == "mask-before-shuffle"):
                g = g * dact(ys[l])
            gi = g
            if u > 1:
                gi = unshuffle(g, u, is3D, transposed=mutant == "sub-positions-transposed")
                if not last and mutant == "mask-before-shuffle":
                    gi = gi * dact(ys[l]).reshape(gi.shape)      # (the fine array read as if it were the inner convolution's)
            r = (w.shape[-1] - 1) // 2
            gw = conv(sq(xs[l]).transpose(0, 1), sq(gi).transpose(0, 1), padding=r).transpose(0, 1)
            out[l] = (gw.double().numpy(), gi.sum(dim=[0, 2, 3, 4]).double().numpy())
            if u > 1 and mutant == "dgrad-sub0-only":
                gi = gi * (torch.arange(gi.shape[1]) % S == 0).to(dtype).reshape(1, -1, 1, 1, 1)
            g = un(conv(sq(gi), w.transpose(0, 1).flip(list(range(2, 2 + nd))), padding=r))
    gin = torch.autograd.grad(loss + (x * g).sum(), [p0, U0], allow_unused=True)
    inp = tuple((torch.zeros_like(t) if gi is None else gi).double().numpy() for gi, t in zip(gin, (p0, U0)))
    return out, inp


def mutant_applies(mutant, name):
    """does the case have the layer the mutant breaks"""
    m = model_of(name)
    n = len(m.layers)
    if mutant.startswith("pool"):
        return any(v > 1 for v in m.pool)
    if mutant == "mask-before-shuffle":
        return any(u > 1 and l + 1 < n for l, u in enumerate(m.up))
    if mutant == "dgrad-sub0-only":
        return any(u > 1 and l > 0 for l, u in enumerate(m.up))
    return any(u > 1 for u in m.up)


def rel_l2_per_tensor(name, mode, got, want, l1):
    """model_grad_ref.rel_l2_per_tensor. In the gradU-only mode the last layer's gradBias is zero by construction where that
    layer is a plain convolution (the sum of the gradient at pPred over all voxels): held to BAR * sum |g_pPred| there. An
    upsample layer's gradBias sums over one sub-lattice each, which does not cancel: plain rel-L2."""
    zero = l1 if (mode == "u-only" and model_of(name).up[-1] == 1) else None
    return R.rel_l2_per_tensor(got, want, zero)


def worst(name, mode, got, want, l1):
    return max(max(pair) for pair in rel_l2_per_tensor(name, mode, got, want, l1))


# ---- the closed loop: run_epoch.Closure on the 2-D tog, B = 2, 1 x 16 x 32 ------------------------------------------------------
# manta targets (a damped copy of the inputs, as tests/test_hip_run_epoch.py makes them), no pressure term (the closure would
# re-centre pTarget in place), no long-term pass; Adam with default_conf.lua's figures and the clip at 1.
LOOP = dict(dims=(1, 16, 32), B=2, seed=91, steps=3, lambdas=(0.0, 1.0, 1.0),
            adam=dict(learningRate=0.0025, learningRateDecay=0, beta1=0.9, beta2=0.999, epsilon=1e-4, weightDecay=0), clip=1.0)


def loop_model():
    from fluidnet_amd import FluidNetModel
    return FluidNetModel.tog(False, seed=5, scale=1.0)


def loop_batch():
    """numpy: pDiv, UDiv, flags, pTarget, UTarget"""
    sc = scenes.make_scene(LOOP["dims"], seed=LOOP["seed"], B=LOOP["B"], vel_cells=0.6)
    return dict(pDiv=sc["p"], UDiv=sc["U"], flags=sc["flags"], pTarget=sc["p"] * np.float32(0.5), UTarget=sc["U"] * np.float32(0.9))


@functools.lru_cache(maxsize=None)
def loop_series():
    """the fp64 series: the loss in front of each of LOOP's steps and behind the last, the parameters walked by optim_ref's
    restatement of the clipped Adam step"""
    import optim_ref as O
    m, b = loop_model(), loop_batch()
    cfg = dict(LOOP["adam"], method=O.ADAM, gradNormThreshold=LOOP["clip"])
    x = [np.asarray(t, np.float64) for wb in m.layers for t in wb]
    st = O.new_state(x, cfg)
    losses = []
    for step in range(LOOP["steps"] + 1):
        params = [(torch.from_numpy(x[2 * i]).requires_grad_(True), torch.from_numpy(x[2 * i + 1]).requires_grad_(True)) for i in range(len(m.layers))]
        p, U = net(m, params, _T(b["pDiv"], torch.float64), _T(b["UDiv"], torch.float64), b["flags"])
        loss = R.criterion_loss(p, U, b["pTarget"], b["UTarget"], b["flags"], LOOP["lambdas"])
        losses.append(float(loss.detach()))
        if step == LOOP["steps"]:
            break
        g = torch.autograd.grad(loss, [t for wb in params for t in wb])
        x, _ = O.step(x, [t.numpy() for t in g], st, cfg)
    return losses
