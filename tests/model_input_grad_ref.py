"""Helper of tests/test_model_input_grad_cpu.py and tests/test_hip_model_input_grad.py: the restatement of
tests/model_grad_ref.py with pDiv and UDiv as autograd leaves -- the yardstick of tfl_model_backward_input -- the same gradients
by the formulas the kernels implement (include/tfluids_hip.h tfl_model_backward_input), which can be broken on
purpose (MUTANTS), and the chained net(net(x)) that ProjectionNet(input_grad=True) makes trainable.

The operators, cases, inputs and the bar are model_grad_ref's; only the head is restated here, because R._head takes numpy
inputs and so cuts the graph in front of the scale.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import model_grad_ref as R

BAR = R.BAR
MUTANTS = ("scale-constant", "first-layer-unmirrored", "skip-gradient-dropped", "vu-direct-path-dropped",
           "no-wall-mask-on-result", "divergence-transpose-wrong-side")


# Two cases beyond model_grad_ref's 18, for the one path they leave out: the scale taken from the divergence while the net input
# has no div channel, so that the backward recomputes U_bc and its divergence. name -> (kind, is3D, opts, the case whose inputs it takes)
EXTRA = {
    "norm-std-div-without-div-chan": ("default", False, dict(normalizeInputChan="div", inputChannels=dict(div=False, UDiv=True)), "default2d-a"),
    "norm-l2-div-without-div-chan": ("default", True, dict(normalizeInputFunc="norm", normalizeInputChan="div",
                                                           inputChannels=dict(div=False, UDiv=True)), "default3d-a"),
}
NAMES = R.NAMES + list(EXTRA)


def spec(name):
    """(kind, is3D, opts) of a case of model_grad_ref or of EXTRA"""
    if name in EXTRA:
        return EXTRA[name][:3]
    return R.case(name)[1:4]


def make_inputs(name):
    return R.make_inputs(EXTRA[name][3] if name in EXTRA else name)


def _model(name):
    kind, is3D, opts = spec(name)
    return R.make_model(kind, is3D, opts)


def _T(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)


def head(p, Ud, flags, opts, is3D):
    """R._head for torch tensors p, Ud (possibly leaves): (x, skip, scale [B,1,1,1,1], U_bc, resolved opts)"""
    from fluidnet_amd.model import _resolve_opts
    o = _resolve_opts(opts)
    ic = o["inputChannels"]
    dtype = p.dtype
    U_bc = Ud * _T(R.wall_keep_mask(flags, is3D), dtype)
    div = R.divergence(U_bc, flags, is3D)
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
    chans.append(_T(R.occupancy(flags), dtype))
    skip = p / sc if o["addPressureSkip"] else None
    return torch.cat(chans, dim=1), skip, sc, U_bc, o


def net(params, p, Ud, flags, opts, is3D, keep_acts=None):
    """(p, U) of one pass; params: [(w, b)] torch tensors. keep_acts: a dict that receives xs (layer inputs) and ys (outputs)"""
    x, skip, sc, U_bc, o = head(p, Ud, flags, opts, is3D)
    h = x
    xs, ys = [], []
    for l, (w, b) in enumerate(params):
        last = l + 1 == len(params)
        if last and skip is not None:
            h = torch.cat([h, skip], dim=1)
        xs.append(h)
        h = R._conv(h, w, b, is3D)
        if not last:
            h = R._act(h, o["nonlinType"])
        ys.append(h)
    if keep_acts is not None:
        keep_acts.update(xs=xs, ys=ys, sc=sc, U_bc=U_bc, o=o)
    return R._tail(h, sc, U_bc, flags, is3D)


def _params(layers, dtype, grad=False):
    return [(_T(w, dtype).requires_grad_(grad), _T(b, dtype).requires_grad_(grad)) for w, b in layers]


def _mode_grads(name, mode):
    _, _, _, gP, gU = make_inputs(name)
    return (None if mode == "u-only" else gP), (None if mode == "p-only" else gU)


def _loss(p, U, gP, gU):
    loss = p.sum() * 0
    if gP is not None:
        loss = loss + (p * _T(gP, p.dtype)).sum()
    if gU is not None:
        loss = loss + (U * _T(gU, p.dtype)).sum()
    return loss


@functools.lru_cache(maxsize=None)
def input_grads(name, mode="both", dtype=torch.float64):
    """(gradPDiv, gradUDiv) as float64 numpy arrays: d/d(pDiv, UDiv) of sum(gradP p) + sum(gradU U) by autograd; read-only"""
    m = _model(name)
    pDiv, UDiv, flags, _, _ = make_inputs(name)
    gP, gU = _mode_grads(name, mode)
    p0, U0 = _T(pDiv, dtype).requires_grad_(True), _T(UDiv, dtype).requires_grad_(True)
    p, U = net(_params(m.layers, dtype), p0, U0, flags, m.opts, m.is3D)
    g = torch.autograd.grad(_loss(p, U, gP, gU), [p0, U0], allow_unused=True)
    out = tuple((torch.zeros_like(t) if gi is None else gi).double().numpy() for gi, t in zip(g, (p0, U0)))
    for a in out:
        a.setflags(write=False)
    return out


def _vu_masks(flags, is3D):
    """per component c: (the cell overwrites u_c: empty, not outflow, interior, minus-neighbour not fluid)"""
    b = R._bits(flags[:, 0])
    inner = R._interior(b["fluid"].shape, is3D)
    C = 3 if is3D else 2
    axes = [3, 2, 1][:C]
    em = b["empty"] & ~b["outflow"] & ~b["fluid"] & inner
    return [em & ~R._prev(b["fluid"], ax) for ax in axes]


def manual_input_grads(name, mode="both", dtype=torch.float64, mutant=None):
    """The same two gradients by the six pieces of DESIGN.md 3.16, optionally broken:
      scale-constant                    the input scale treated as a constant of the inputs (g_s = 0)
      first-layer-unmirrored            the first layer's data gradient convolves with W transposed but NOT mirrored
      skip-gradient-dropped             the joined skip channel's gradient left out (skip models only)
      vu-direct-path-dropped            the velocity update's gradient to its velocity input left out (gradU given only)
      no-wall-mask-on-result            gradUDiv = g_Ubc without the wall mask
      divergence-transpose-wrong-side   the divergence's transpose gathers the plus-neighbour (div channel or div normaliser only)
    """
    assert mutant is None or mutant in MUTANTS
    m = _model(name)
    is3D = m.is3D
    pDiv, UDiv, flags, _, _ = make_inputs(name)
    gP, gU = _mode_grads(name, mode)
    nd = 3 if is3D else 2
    C = nd
    axes = [3, 2, 1][:C]
    with torch.no_grad():
        ws = _params(m.layers, dtype)
        acts = {}
        p_out, U_out = net(ws, _T(pDiv, dtype), _T(UDiv, dtype), flags, m.opts, is3D, keep_acts=acts)
        xs, ys, sc, U_bc, o = acts["xs"], acts["ys"], acts["sc"], acts["U_bc"], acts["o"]
        ic = o["inputChannels"]
        q = 1.0 / sc
        keep = _T(R.wall_keep_mask(flags, is3D), dtype)
        pT = _T(pDiv, dtype)
        gPt = torch.zeros_like(pT) if gP is None else _T(gP, dtype)
        gUt = torch.zeros_like(U_bc) if gU is None else _T(gU, dtype)
        pPred = ys[-1]
        h = sc * keep * gUt
    # VU is linear in pPred: its transpose by autograd of the operator alone (what tfl_model_backward already forms)
    pp = pPred.clone().requires_grad_(True)
    g = torch.autograd.grad((R.velocity_update(torch.zeros_like(U_bc), pp, flags, is3D) * h).sum(), pp)[0] + sc * gPt
    with torch.no_grad():
        sq = (lambda t: t) if is3D else (lambda t: t[:, :, 0])
        un = (lambda t: t) if is3D else (lambda t: t.unsqueeze(2))
        conv = F.conv3d if is3D else F.conv2d
        g_skip = None
        for l in range(len(ws) - 1, -1, -1):
            w, _ = ws[l]
            if l + 1 < len(ws):
                y = ys[l]
                g = g * {"relu": (y > 0).to(dtype), "relu6": ((y > 0) & (y < 6)).to(dtype), "sigmoid": y * (1 - y)}[o["nonlinType"]]
            wt = w.transpose(0, 1)
            if not (l == 0 and mutant == "first-layer-unmirrored"):
                wt = wt.flip(list(range(2, 2 + nd)))
            g = un(conv(sq(g), wt, padding=(w.shape[-1] - 1) // 2))
            if l + 1 == len(ws) and o["addPressureSkip"]:
                g_skip, g = g[:, -1:], g[:, :-1]
        g_x = g
        ch = 0
        zero1 = torch.zeros_like(pT)
        g_qp, g_qU, g_qd = zero1.clone(), torch.zeros_like(U_bc), zero1.clone()
        if ic["pDiv"]:
            g_qp = g_qp + g_x[:, ch:ch + 1]; ch += 1
        if ic["UDiv"]:
            g_qU = g_qU + g_x[:, ch:ch + C]; ch += C
        if ic["div"]:
            g_qd = g_qd + g_x[:, ch:ch + 1]; ch += 1
        if g_skip is not None and mutant != "skip-gradient-dropped":
            g_qp = g_qp + g_skip
        if mutant != "vu-direct-path-dropped":
            over = torch.stack([_T(mk, dtype) for mk in _vu_masks(flags, is3D)], dim=1)
            g_qU = g_qU + h * (1 - over)
        d = R.divergence(U_bc, flags, is3D)
        S = lambda t: t.reshape(t.shape[0], -1).sum(1).reshape(-1, 1, 1, 1, 1)
        g_s = S(gPt * pPred) + q * S(gUt * U_out) - q * (S(g_qp * q * pT) + S(g_qU * q * U_bc) + S(g_qd * q * d))
        ds = {"UDiv": None, "pDiv": None, "div": None}
        if o["normalizeInput"] and mutant != "scale-constant":
            chan = o["normalizeInputChan"]
            src = {"UDiv": U_bc, "pDiv": pT, "div": d}[chan]
            n = src[0].numel()
            if o["normalizeInputFunc"] == "std":
                ds[chan] = g_s * (src - S(src) / n) / ((n - 1.0) * sc)
            else:
                ds[chan] = g_s * src / sc
        g_d = q * g_qd + (0 if ds["div"] is None else ds["div"])
        b = R._bits(flags[:, 0])
        on = _T((b["fluid"] & R._interior(b["fluid"].shape, is3D)), dtype)
        og = on * g_d[:, 0]
        shift = R._shift_next if mutant == "divergence-transpose-wrong-side" else R._shift_prev
        Dt = torch.stack([og - shift(og, ax) for ax in axes], dim=1)
        g_Ubc = q * g_qU + Dt + (0 if ds["UDiv"] is None else ds["UDiv"])
        gUD = g_Ubc if mutant == "no-wall-mask-on-result" else keep * g_Ubc
        gPD = q * g_qp + (0 if ds["pDiv"] is None else ds["pDiv"])
    return gPD.double().numpy(), gUD.double().numpy()


def mutant_applies(mutant, name, mode):
    """does the mutant change anything for this case and gradient mode at all"""
    from fluidnet_amd.model import _resolve_opts
    o = _resolve_opts(spec(name)[2])
    if spec(name)[0] == "k5-skip":
        o["addPressureSkip"] = True
    if mutant == "scale-constant":
        return bool(o["normalizeInput"])
    if mutant == "skip-gradient-dropped":
        return bool(o["addPressureSkip"])
    if mutant == "vu-direct-path-dropped":
        return mode != "p-only"
    if mutant == "divergence-transpose-wrong-side":
        return bool(o["inputChannels"]["div"]) or (o["normalizeInput"] and o["normalizeInputChan"] == "div")
    return True


def rel_l2(got, want):
    """plain rel-L2; an all-zero yardstick asks for an all-zero answer (0 or inf)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nw = np.linalg.norm(want)
    if nw == 0:
        return 0.0 if not got.any() else float("inf")
    return float(np.linalg.norm(got - want) / nw)


def worst(got, want):
    return max(rel_l2(g, w) for g, w in zip(got, want))


# ---- two (or more) chained passes: net(net(x)), the loss on the last outputs ---------------------------------------------
CHAIN_CASES = ("default2d-a", "default3d-a", "k5-skip2d", "yang3d", "sigmoid")


@functools.lru_cache(maxsize=None)
def chain_param_grads(name, passes=2, dtype=torch.float64):
    """([(gradWeight, gradBias)], (gradPDiv, gradUDiv)) of sum(gradP p_n) + sum(gradU U_n), (p_i, U_i) = net(p_{i-1}, U_{i-1}),
    flags fixed, the parameters shared by the passes; float64 numpy, read-only"""
    m = _model(name)
    pDiv, UDiv, flags, gP, gU = make_inputs(name)
    params = _params(m.layers, dtype, grad=True)
    p0, U0 = _T(pDiv, dtype).requires_grad_(True), _T(UDiv, dtype).requires_grad_(True)
    p, U = p0, U0
    for _ in range(passes):
        p, U = net(params, p, U, flags, m.opts, m.is3D)
    flat = [t for wb in params for t in wb]
    g = torch.autograd.grad(_loss(p, U, gP, gU), flat + [p0, U0])
    n = len(params)
    return ([(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(n)],
            (g[2 * n].double().numpy(), g[2 * n + 1].double().numpy()))
