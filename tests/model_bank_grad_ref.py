"""Helper of tests/test_model_bank_grad_cpu.py and tests/test_hip_model_bank_backward.py: a differentiable float64 restatement
of the banked projection net (lib/model.lua:253-362: 'mres' and 'dilate' banks, 'concat' and 'add' joins) in torch on the CPU --
the yardstick of tfl_model_backward / tfl_model_backward_input on graph models.

Head and tail are model_grad_ref's (_head, _tail; with pDiv / UDiv as autograd leaves: model_input_grad_ref.head, the same
formulas on tensors). The stack is tests/model_graph_ref.graph_stack's, re-expressed on tensors that require grad. manual_grads():
the same gradients module by module in the formulas the kernels implement -- join backward, per-bank weight / data gradients at
the bank's tap spacing, split backward -- which can be broken on purpose (MUTANTS); unbroken it equals autograd.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import model_grad_ref as R
import model_input_grad_ref as I
import scenes

BAR = R.BAR
GRAD_MODES = R.GRAD_MODES
MUTANTS = ("pyramid-pool-backward-unscaled", "upsample-backward-one-child", "weight-gradient-ignores-dilation",
           "add-join-feeds-bank-1-only", "concat-slices-swapped")

# The smallest grids at which each mechanism can still go wrong: divisible by 4 (three mres banks); x = one full and one ragged
# 32-wide weight-gradient tile; y = more than one 8-row tile; the coarsest level's x is odd-sized (10 and 9 cells: 40 / 4, 36 / 4);
# tap spacing 4 reaches past both z faces of the 8-deep grid.
G2 = (2, 1, 24, 40)
G3 = (2, 8, 12, 36)


def _g(n, kind, agg, **kw):
    return dict(banksNum=n, banksType=kind, banksAggregateMethod=agg, **kw)


# (name, modelType, is3D, opts, graph, (B, Z, Y, X))
CASES = [("%s%d-%s-%s" % (kind, n, agg, "3d" if is3D else "2d"), "default", is3D, None, _g(n, kind, agg), G3 if is3D else G2)
         for kind in ("mres", "dilate") for agg in ("concat", "add") for n in (2, 3) for is3D in (False, True)]
CASES += [
    # layers in front of the split: the split's backward feeds a parameter gradient
    ("mres3-add-split2-join4-2d", "default", False, None, _g(3, "mres", "add", banksSplitStage=2, banksJoinStage=4), G2),
    ("dilate2-concat-split2-join3-3d", "default", True, None, _g(2, "dilate", "concat", banksSplitStage=2, banksJoinStage=3), G3),
    ("yang-mres2-concat-3d", "yang", True, None, _g(2, "mres", "concat"), G3),
    ("yang-dilate3-add-2d", "yang", False, None, _g(3, "dilate", "add", banksSplitStage=1, banksJoinStage=2), G2),
    ("sigmoid-mres2-add-2d", "default", False, dict(nonlinType="sigmoid"), _g(2, "mres", "add"), G2),
    ("relu6-dilate2-concat-2d", "default", False, dict(nonlinType="relu6"), _g(2, "dilate", "concat"), G2),
    ("skip-dilate2-add-3d", "default", True, dict(addPressureSkip=True), _g(2, "dilate", "add"), G3),
    ("udiv-mres2-concat-2d", "default", False, dict(inputChannels=dict(UDiv=True)), _g(2, "mres", "concat"), G2),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


def make_model(name, seed=3):
    """the seeded FluidNetModel of a case (FluidNetModel.from_mconf: lib/model.lua's layer table with the case's banks)"""
    from fluidnet_amd import FluidNetModel
    _, kind, is3D, opts, graph, _ = case(name)
    m = FluidNetModel.from_mconf(dict(opts or {}, modelType=kind, **graph), is3D, seed=seed)
    if (opts or {}).get("nonlinType") == "sigmoid":
        m.layers = [(w * np.float32(6.0), b) for w, b in m.layers]      # (model_grad_ref.make_model: spread over the sigmoid's range)
    return m


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """(pDiv, UDiv, flags, gradP, gradU) of a case, read-only: model_grad_ref.make_inputs's recipe (white-noise fields,
    salt-and-pepper obstacles, an obstacle box on the weight-gradient tile's corner, a gradP with a mean)"""
    i = NAMES.index(name)
    B, Z, Y, X = CASES[i][5]
    sc = scenes.rough_scene((Z, Y, X), seed=700 + i, B=B, obstacle_frac=0.08)
    f = sc["flags"]
    z0 = slice(1, Z - 1) if Z > 2 else slice(0, 1)
    f[:, :, z0, 7:9, 31:33] = scenes.OBSTACLE
    rng = np.random.RandomState(1300 + i)
    gP = (rng.randn(*sc["p"].shape) + 0.5).astype(np.float32)
    gU = rng.randn(*sc["U"].shape).astype(np.float32)
    out = (sc["p"], sc["U"], np.ascontiguousarray(f), gP, gU)
    for t in out:
        t.setflags(write=False)
    return out


# ---- the stack ----------------------------------------------------------------------------------------------------------
def _graph_of(model):
    from fluidnet_amd.model import DEFAULT_GRAPH
    return model.graph or dict(DEFAULT_GRAPH)


def _modules(model):
    """[(stage, bank)] in creation order, the stage count"""
    from fluidnet_amd.model import conv_modules
    g = _graph_of(model)
    n = g["banksNum"]
    nst = len(model.layers) - (n - 1) * (g["banksJoinStage"] - g["banksSplitStage"]) if n > 1 else len(model.layers)
    return conv_modules(nst, g), nst


def _dil(model, bank):
    g = _graph_of(model)
    return 2 ** bank if (g["banksNum"] > 1 and g["banksType"] == "dilate") else 1


def _conv(t, w, b, is3D, dil=1):
    r = (w.shape[-1] - 1) // 2
    return (F.conv3d if is3D else F.conv2d)(t, w, b, padding=dil * r, dilation=dil)


def stack(x, params, model, skip=None, keep=None):
    """pPred from the net input x [B, C, Z, Y, X] (model_graph_ref.graph_stack on torch tensors, any dtype, differentiable).
    keep: a dict that receives xs / ys (every module's input and post-activation output, squeezed in 2-D)"""
    is3D = model.is3D
    g = _graph_of(model)
    n, mres, concat = g["banksNum"], g["banksType"] == "mres", g["banksAggregateMethod"] == "concat"
    avg = F.avg_pool3d if is3D else F.avg_pool2d
    mods, _ = _modules(model)
    act = model.opts["nonlinType"]
    h = x if is3D else x[:, :, 0]
    hl, xs, ys = [h], [], []
    for mi, (st, bank) in enumerate(mods):
        if bank == 0 and n > 1 and st == g["banksSplitStage"]:
            for i in range(1, n):
                hl.append(avg(hl[i - 1], 2) if mres else hl[0])
        if bank == 0 and n > 1 and st == g["banksJoinStage"]:
            if mres:
                hl = [hl[0]] + [F.interpolate(hl[i], scale_factor=2 ** i, mode="nearest") for i in range(1, n)]
            if concat:
                hl = [torch.cat(hl, dim=1)]
            else:
                s = hl[0]
                for t in hl[1:]:
                    s = s + t
                hl = [s]
        w, b = params[mi]
        last = mi + 1 == len(mods)
        t = hl[bank]
        if last and skip is not None:
            t = torch.cat([t, skip if is3D else skip[:, :, 0]], dim=1)
        xs.append(t)
        t = _conv(t, w, b, is3D, _dil(model, bank))
        if not last:
            t = R._act(t, act)
        ys.append(t)
        hl[bank] = t
    if keep is not None:
        keep.update(xs=xs, ys=ys)
    return hl[0] if is3D else hl[0].unsqueeze(2)


def _T(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)


def _params(layers, dtype, grad=False):
    return [(_T(w, dtype).requires_grad_(grad), _T(b, dtype).requires_grad_(grad)) for w, b in layers]


def forward(model, layers, pDiv, UDiv, flags, dtype=torch.float64, leaves=False):
    """(p, U, params, (pDiv, UDiv) tensors, pPred). leaves: pDiv and UDiv are autograd leaves (the head on tensors)"""
    is3D = model.is3D
    params = _params(layers, dtype, grad=True)
    if leaves:
        p0, U0 = _T(pDiv, dtype).requires_grad_(True), _T(UDiv, dtype).requires_grad_(True)
        x, skip, sc, U_bc, _ = I.head(p0, U0, flags, model.opts, is3D)
    else:
        p0 = U0 = None
        x, skip, sc, U_bc, _ = R._head(pDiv, UDiv, flags, model.opts, is3D, dtype)
    pPred = stack(x, params, model, skip)
    p, U = R._tail(pPred, sc, U_bc, flags, is3D)
    return p, U, params, (p0, U0), pPred


def _loss(p, U, gP, gU):
    return I._loss(p, U, gP, gU)


def grads(model, layers, pDiv, UDiv, flags, gradP, gradU, dtype=torch.float64, inputs=False):
    """([(gradWeight, gradBias)], the L1 norm of the gradient at pPred, (gradPDiv, gradUDiv) or None) as float64 numpy, of
    sum(gradP p) + sum(gradU U) (either may be None), by torch.autograd"""
    p, U, params, (p0, U0), pPred = forward(model, layers, pDiv, UDiv, flags, dtype, leaves=inputs)
    flat = [t for wb in params for t in wb]
    g = torch.autograd.grad(_loss(p, U, gradP, gradU), flat + [pPred] + ([p0, U0] if inputs else []), allow_unused=True)
    n = len(params)
    out = [(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(n)]
    gin = None
    if inputs:
        gin = tuple((torch.zeros_like(t) if gi is None else gi).double().numpy() for gi, t in zip(g[2 * n + 1:], (p0, U0)))
    return out, float(g[2 * n].abs().sum()), gin


# ---- the formulas of the kernels, module by module -------------------------------------------------------------------------
def _wgrad(x, g, k, dil, is3D):
    """gradWeight[co][ci][tap] = sum_pos x[ci][pos + dil (tap - r)] g[co][pos]: a convolution of x by g with the batch as channels;
    the forward's tap spacing is this convolution's stride"""
    r = (k - 1) // 2
    conv = F.conv3d if is3D else F.conv2d
    return conv(x.transpose(0, 1), g.transpose(0, 1), padding=dil * r, stride=dil).transpose(0, 1)


def manual_grads(model, layers, pDiv, UDiv, flags, gradP, gradU, mutant=None, dtype=torch.float64):
    """([(gradWeight, gradBias)], g_x = the gradient at the net input x [B, C, Z, Y, X]) by the formulas of DESIGN.md 3.18,
    optionally broken:
      pyramid-pool-backward-unscaled     P^T replicates the coarse cell over its children without the 1 / 2^dim
      upsample-backward-one-child        the join hands an mres bank one child of each replicated block instead of the block's sum
      weight-gradient-ignores-dilation   a dilated module's weight gradient reads x at tap spacing 1
      add-join-feeds-bank-1-only         an 'add' join passes its gradient to the first bank alone
      concat-slices-swapped              a 'concat' join hands bank i the channel slice of bank n - 1 - i
    """
    assert mutant is None or mutant in MUTANTS
    is3D = model.is3D
    nd = 3 if is3D else 2
    g_ = _graph_of(model)
    n, mres, concat = g_["banksNum"], g_["banksType"] == "mres", g_["banksAggregateMethod"] == "concat"
    split, join = g_["banksSplitStage"], g_["banksJoinStage"]
    mods, nst = _modules(model)
    act = model.opts["nonlinType"]
    with torch.no_grad():
        x, skip, sc, U_bc, _ = R._head(pDiv, UDiv, flags, model.opts, is3D, dtype)
        ws = _params(layers, dtype)
        acts = {}
        pPred = stack(x, ws, model, skip, keep=acts)
        xs, ys = acts["xs"], acts["ys"]
    pp = pPred.clone().requires_grad_(True)
    p, U = R._tail(pp, sc, U_bc, flags, is3D)
    g = torch.autograd.grad(_loss(p, U, gradP, gradU), pp)[0]        # (the tail is linear in pPred: its exact transpose)
    g = g if is3D else g[:, :, 0]
    out = [None] * len(ws)
    first_of = {}
    for mi, (st, bank) in enumerate(mods):
        first_of.setdefault(st, mi)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    avg = F.avg_pool3d if is3D else F.avg_pool2d
    with torch.no_grad():
        gl = [g]
        for st in range(nst, 0, -1):
            live = n if (n > 1 and split <= st < join) else 1
            for bank in range(live):
                mi = first_of[st] + bank
                w, _ = ws[mi]
                gy = gl[bank]
                last = mi + 1 == len(ws)
                if not last:
                    y = ys[mi]
                    gy = gy * {"relu": (y > 0).to(dtype), "relu6": ((y > 0) & (y < 6)).to(dtype), "sigmoid": y * (1 - y)}[act]
                d = _dil(model, bank) if live > 1 else 1
                k = w.shape[-1]
                out[mi] = (_wgrad(xs[mi], gy, k, 1 if mutant == "weight-gradient-ignores-dilation" else d, is3D).double().numpy(),
                           gy.sum(dim=[0] + list(range(2, 2 + nd))).double().numpy())
                wt = w.transpose(0, 1).flip(list(range(2, 2 + nd)))
                gx = (F.conv3d if is3D else F.conv2d)(gy, wt, padding=d * ((k - 1) // 2), dilation=d)
                if last and skip is not None:
                    gx = gx[:, :-1]          # the joined pDiv/scale channel is no output of the stack
                gl[bank] = gx
            if n > 1 and st == join:         # the join's backward: gl = [g at the join's output] -> one gradient per bank
                gj = gl[0]
                C = gj.shape[1] // n if concat else gj.shape[1]
                banks = []
                for i in range(n):
                    if concat:
                        s = (n - 1 - i) if mutant == "concat-slices-swapped" else i
                        gi = gj[:, s * C:(s + 1) * C]
                    else:
                        gi = gj if (i == 0 or mutant != "add-join-feeds-bank-1-only") else torch.zeros_like(gj)
                    if mres and i > 0:
                        f = 2 ** i
                        if mutant == "upsample-backward-one-child":
                            gi = gi[(slice(None), slice(None)) + (slice(None, None, f),) * nd]
                        else:
                            gi = avg(gi, f) * float(f ** nd)          # the sum over the block of replicated cells
                    banks.append(gi.contiguous())
                gl = banks
            if n > 1 and st == split:        # the split's backward: the banks' data gradients -> one
                if mres:
                    scale = 1.0 if mutant == "pyramid-pool-backward-unscaled" else 1.0 / 2 ** nd
                    acc = gl[n - 1]
                    for i in range(n - 2, -1, -1):
                        acc = gl[i] + up(acc) * scale
                    gl = [acc]
                else:
                    s = gl[0]
                    for t in gl[1:]:
                        s = s + t
                    gl = [s]
    g_x = gl[0] if is3D else gl[0].unsqueeze(2)
    return out, g_x.double().numpy()


def x_grad(model, layers, pDiv, UDiv, flags, gradP, gradU, dtype=torch.float64):
    """the gradient at the net input x by autograd (what manual_grads's g_x restates)"""
    is3D = model.is3D
    x, skip, sc, U_bc, _ = R._head(pDiv, UDiv, flags, model.opts, is3D, dtype)
    x = x.clone().requires_grad_(True)
    pPred = stack(x, _params(layers, dtype), model, skip)
    p, U = R._tail(pPred, sc, U_bc, flags, is3D)
    return torch.autograd.grad(_loss(p, U, gradP, gradU), x)[0].double().numpy()


def mutant_applies(mutant, name):
    g = dict(case(name)[4])
    mres, concat = g["banksType"] == "mres", g["banksAggregateMethod"] == "concat"
    if mutant == "pyramid-pool-backward-unscaled":
        return mres                       # (in g_x; in the parameter gradients too where layers precede the split)
    if mutant == "upsample-backward-one-child":
        return mres
    if mutant == "weight-gradient-ignores-dilation":
        return not mres
    if mutant == "add-join-feeds-bank-1-only":
        return not concat
    return concat


rel_l2_per_tensor = R.rel_l2_per_tensor


@functools.lru_cache(maxsize=None)
def expected(name, mode="both"):
    """(the fp64 parameter gradients, PyTorch-CPU-fp32's, zero_l1 (u-only mode: see model_grad_ref.rel_l2_per_tensor), the fp64
    (gradPDiv, gradUDiv), PyTorch-CPU-fp32's); computed once per process, read-only"""
    m = make_model(name)
    pDiv, UDiv, flags, gP, gU = make_inputs(name)
    gP = None if mode == "u-only" else gP
    gU = None if mode == "p-only" else gU
    g64, l1, in64 = grads(m, m.layers, pDiv, UDiv, flags, gP, gU, torch.float64, inputs=True)
    g32, _, in32 = grads(m, m.layers, pDiv, UDiv, flags, gP, gU, torch.float32, inputs=True)
    return g64, g32, (l1 if mode == "u-only" else None), in64, in32


# ---- the closed loop on a banked model: model_grad_ref.LOOP's scene, rate and step count ---------------------------------------
LOOP_GRAPH = _g(2, "mres", "add")


def loop_model():
    """the seeded 2-D default table with two mres banks joined by 'add', `gain` times its weights (as model_grad_ref.loop_model)"""
    from fluidnet_amd import FluidNetModel
    m = FluidNetModel.from_mconf(dict(modelType="default", **LOOP_GRAPH), False, seed=5)
    m.layers = [(w * np.float32(R.LOOP["gain"]), b) for w, b in m.layers]
    return m


def train_loop(model, layers, pDiv, UDiv, flags, pT, UT, lambdas, lr, steps, dtype=torch.float64):
    """plain SGD on the restatement: ([loss before each step] + [loss after the last], [params after each step])"""
    cur = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in layers]
    losses, history = [], []
    for _ in range(steps):
        p, U, params, _, _ = forward(model, cur, pDiv, UDiv, flags, dtype)
        loss = R.criterion_loss(p, U, pT, UT, flags, lambdas)
        flat = [t for wb in params for t in wb]
        g = torch.autograd.grad(loss, flat)
        losses.append(float(loss.detach()))
        cur = [((params[i][0] - lr * g[2 * i]).detach().double().numpy(), (params[i][1] - lr * g[2 * i + 1]).detach().double().numpy())
               for i in range(len(params))]
        history.append(cur)
    with torch.no_grad():
        p, U, _, _, _ = forward(model, cur, pDiv, UDiv, flags, dtype)
        losses.append(float(R.criterion_loss(p, U, pT, UT, flags, lambdas)))
    return losses, history
