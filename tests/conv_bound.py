"""Per-voxel fp64 error bounds for the projection ConvNet (every conv path of tfl_model_forward).

forward_bound() evaluates the net of oracle/simulate_np.model_forward (or, for graph models, tests/model_graph_ref.py) in
float64 on the same fp32 inputs and weights, and beside every value a rigorous upper bound on how far an fp32 evaluation
by the named conv path may lie from it -- running-error analysis, layer by layer, all in fp64 (u = 2^-24):

  net input      ApplyScale's division is one rounding; the scale itself is allowed 1 ulp (its sums run in another order on
                 the GPU): e0 = 2u |x| on the divided channels, 0 on the occupancy
  conv layer     e = conv(|W|, e_in) + rounding(path) + representation(path), every conv of |W| with the layer's own padding,
                 dilation and sub-position shuffle
  non-linearity  ReLU / relu6 are 1-Lipschitz and exact; sigmoid is 1/4-Lipschitz, plus its own evaluation (5u, below)
  pooling        average: the mean of e plus the rounding of the window sum; max: the max of e over the window
  joins          concat carries e, add adds e plus one rounding; nearest upsampling and the shuffle permute e
  batch norm     folded on the host to fmaf(v, scale, shift), scale and shift rounded once each from fp64
  outputs        p = pPred * scale and U = (U_bc / scale - grad pPred) * scale, each operation one rounding (below)

The constants of each path are derived from its kernel's arithmetic; none is fitted to observed errors. gamma(n, r) is the
usual n r / (1 - n r), the bound on n successive roundings of relative size r.

  fp32        conv.hip (direct / generic / graph): an fmaf chain from the bias, gamma(fan_in + 1, u)
  mfma        conv_mfma.hip, conv2d_mfma.hip: fp32 operands on the matrix cores, gamma(fan_in + 1, 2u)
  winograd    conv_valu.hip: the k = 3 layers as Winograd F(2, 3) along x (see _winograd_mag); the fused 1x1x1 tail in
              fp32 fmaf, gamma(fan_in + 1, u)
  mfma16      conv_mfma16.hip: the k = 3 layers and the tail's 8 -> 8 k = 1 layer on split fp16 operands (see _M16), the
              last 8 -> 1 layer in fp32 fmaf, gamma(fan_in + 1, u)

ASSUMPTION (every MFMA path): the internal rounding of an MFMA's accumulation is not documented for gfx950 and has not been
measured here. It is taken to be at most 2u per addition -- twice a correctly rounded fp32 add -- over every product the
accumulator takes in.
"""
import math

import numpy as np

from oracle import simulate_np as S

U32 = 2.0 ** -24                   # unit roundoff of fp32
FLUID, OBSTACLE, EMPTY, OUTFLOW = 1, 2, 4, 16


def gamma(n, r=U32):
    return n * r / (1.0 - n * r)


# conv_mfma16.hip: a = a_h + 2^-11 a_l with a_h = fp16(a), a_l = fp16((a - a_h) 2^11) (split_h / split_pair; the weights
# the same after the per-layer exponent 2^e that puts max |w| 2^e in [8, 16)). |a - a_h| <= 2^-11 |a| and a_l carries that
# residual to 2^-11 of itself: the pair represents a within 2^-22 |a|. Below fp16's normal range (2^-14) the rounding of
# a half is absolute, at most half of 2^-24, which the 2^-11 scaling of a_l turns into 2^-36 in a.
M16_REL = 2.0 ** -22
M16_FLOOR = 2.0 ** -36
# Products of two halves are exact in fp32. Each of the two accumulators of an output channel (w_h row, w_l row) takes two
# partial products per (tap, input channel): a_h w 2^11 and a_l w -- 2 fan_in additions at 2u. Their summed magnitudes are
# at most (1 + 2^-10) and 2^-11 (1 + 2^-10) of sum |w_hat| |a_hat| after the post-scale: the factor (1 + 2^-9) covers both.
# The recombination fma(D1, 2^-11, D0) and the epilogue fma(., 2^-(11+e), bias) round once each.
M16_SUM = 1.0 + 2.0 ** -9

# the 3-D `default` topology (model.lua:219-226) and the 2-D one (myModel2D)
DEFAULT3 = [(8, 3, 3), (8, 8, 3), (8, 8, 3), (8, 8, 1), (1, 8, 1)]
DEFAULT2 = [(16, 3, 3), (16, 16, 3), (16, 16, 3), (16, 16, 3), (1, 16, 1)]


def topology(layers):
    return [(w.shape[0], w.shape[1], w.shape[-1]) for w, _ in layers]


def conv_path(model, env_path=None):
    """The forward tfl_model_create picks for `model` (tfl_model.hpp ConvPath) with TFL_CONV_PATH = env_path (None = unset)."""
    custom = S.model_opts(model.opts) != S.model_opts(None)
    if model.graph is not None or custom or any(v > 1 for v in model.pool + model.up):
        return "fp32"
    top = topology(model.layers)
    if model.is3D and top == DEFAULT3:
        return {None: "mfma16", "mfma16": "mfma16", "mfma": "mfma", "direct": "fp32"}.get(env_path, "winograd")
    if not model.is3D and top == DEFAULT2:
        return "fp32" if env_path == "direct" else "mfma"
    return "fp32"


def m16_exponent(w):
    """conv3_m16_pack_weights / conv3_m16_pack_tail: e with max |w| 2^e in [8, 16) (0 for an all-zero or non-finite w)."""
    mx = float(np.max(np.abs(w))) if w.size else 0.0
    if mx > 0.0 and math.isfinite(mx):
        return 4 - math.frexp(mx)[1]
    return 0


class Walker:
    """The conv stack of model_graph_ref.graph_stack (plain models are its one-bank case), over an evaluator `ev` whose
    values may be anything: ev.conv / act / pool / bn / shuffle / avg2 / up_nearest / concat / add / cat_skip."""

    def __init__(self, model):
        self.model = model
        self.g = model.graph or dict(banksNum=1, banksType="mres", banksAggregateMethod="concat", banksSplitStage=1,
                                     banksJoinStage=3, poolType="avg", addBatchNorm=False, bn=None)

    def run(self, ev, h, skip=None):
        from model_graph_ref import creation_order
        m, g = self.model, self.g
        n = g["banksNum"]
        nstages = len(m.layers) - (n - 1) * (g["banksJoinStage"] - g["banksSplitStage"]) if n > 1 else len(m.layers)
        mods = creation_order(nstages, g)
        hl = [h]
        for mi, (st, bank) in enumerate(mods):
            if bank == 0 and n > 1 and st == g["banksSplitStage"]:
                for i in range(1, n):
                    hl.append(ev.avg2(hl[i - 1]) if g["banksType"] == "mres" else hl[0])
            if bank == 0 and n > 1 and st == g["banksJoinStage"]:
                if g["banksType"] == "mres":
                    hl = [hl[0]] + [ev.up_nearest(hl[i], 2 ** i) for i in range(1, n)]
                if g["banksAggregateMethod"] == "concat":
                    hl = [ev.concat(hl)]
                else:
                    s = hl[0]
                    for t in hl[1:]:
                        s = ev.add(s, t)
                    hl = [s]
            w, b = m.layers[mi]
            last = mi + 1 == len(mods)
            t = hl[bank]
            if last and skip is not None:
                t = ev.cat_skip(t, skip)
            dil = 2 ** bank if (n > 1 and g["banksType"] == "dilate") else 1
            t = ev.conv(t, mi, w, b, dil)
            if m.up[mi] > 1:
                t = ev.shuffle(t, m.up[mi])
            if not last:
                t = ev.act(t, m.opts["nonlinType"])
                if m.pool[mi] > 1:
                    t = ev.pool(t, m.pool[mi], g["poolType"])
                if g["addBatchNorm"]:
                    t = ev.bn(t, g["bn"][mi])
            hl[bank] = t
        return hl[0]


def _shuffle(h, u, is3d):
    from model_graph_ref import _shuffle as sh
    return sh(h, u, is3d)


class BoundEval:
    """Values are (a, e): the fp64 value and the bound on |fp32 - fp64|, torch float64 tensors [B, C, (Z,) Y, X]."""

    def __init__(self, model, path):
        import torch
        import torch.nn.functional as F
        self.torch, self.F = torch, F
        self.model, self.path, self.is3d = model, path, model.is3D
        self.dim = 3 if model.is3D else 2

    def _t(self, a):
        return self.torch.from_numpy(np.asarray(a, np.float64))

    def _conv(self, x, w, b, dil):
        pad = dil * (w.shape[-1] - 1) // 2
        f = self.F.conv3d if self.is3d else self.F.conv2d
        return f(x, w, b, padding=pad, dilation=dil)

    def conv(self, v, li, w, b, dil):
        a, e = v
        W, Bv = self._t(w), self._t(b)
        aW = W.abs()
        y = self._conv(a, W, Bv, dil)
        m = a.abs() + e                                   # bound on |fp32 input|
        fan = w.shape[1] * w.shape[-1] ** self.dim
        kind = self.layer_kind(li)
        if kind == "m16":
            # representation: |w_hat - w| <= dW, |a_hat - a_k| <= dA (module comment); the products of the pairs differ from
            # those of the fp32 operands by at most |W| dA + dW |a_k| + dW dA
            ex = m16_exponent(w)
            dW = M16_REL * aW + M16_FLOOR * 2.0 ** -ex * (W != 0).to(W.dtype)
            inside = self.torch.ones_like(m[:, :1]).expand_as(m)          # the zero padding is represented exactly
            dA = M16_REL * m + M16_FLOOR * inside
            rep = self._conv(m, dW, None, dil) + self._conv(dA, aW + dW, None, dil)
            mag = self._conv(m, aW, None, dil) + rep                     # sum |w_hat| |a_hat|
            rnd = (gamma(2 * fan, 2 * U32) * M16_SUM + 2 * U32 * (1 + 4 * U32)) * mag + U32 * Bv.abs().view(1, -1, *([1] * self.dim))
            err = rep + rnd
        elif kind == "wino":
            # V = B^T d rounds once, U = G g twice (host: 0.5 ((g0 + g2) + g1)), each product enters one fmaf of a 9 cin
            # chain, y0 = (M0 + M1) + M2 / y1 = (M1 - M2) - M3 two more, the bias one: gamma(9 cin + 6) on the magnitudes
            n = 9 * w.shape[1] + 6
            err = gamma(n) * (self._winograd_mag(m, aW) + Bv.abs().view(1, -1, 1, 1, 1))
        else:
            r = 2 * U32 if kind == "mfma" else U32
            err = gamma(fan + 1, r) * (self._conv(m, aW, None, dil) + Bv.abs().view(1, -1, *([1] * self.dim)))
        return y, self._conv(e, aW, None, dil) + err

    def layer_kind(self, li):
        """which arithmetic layer li runs in on this path"""
        if self.path == "mfma16":
            return "m16" if li < 4 else "fp32"
        if self.path == "winograd":
            return "wino" if li < 3 else "fp32"
        return "mfma" if self.path == "mfma" else "fp32"

    def _winograd_mag(self, m, aW):
        """|A^T| ((|G| |g|) . (|B^T| |d|)) summed over (c_in, dz, dy): a lane owns the x-pair (x, x + 1), x even, reads
        d0..d3 = a[x - 1 .. x + 2] and forms y0 = M0 + M1 + M2, y1 = M1 - M2 - M3 with M_p = V_p U_p,
        V = (d0 - d2, d1 + d2, d2 - d1, d1 - d3), U = (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2). With S = |g0| +
        |g1| + |g2| and |U_1|, |U_2| <= S / 2 the magnitudes are, as taps (x - 1, x, x + 1) of the output voxel:
        y0 (x even): (|g0|, S, |g0| + S);  y1 (x odd): (S + |g2|, S, |g2|)."""
        torch = self.torch
        g0, g1, g2 = aW[..., 0], aW[..., 1], aW[..., 2]
        s = g0 + g1 + g2
        k_even = torch.stack([g0, s, g0 + s], dim=-1)
        k_odd = torch.stack([s + g2, s, g2], dim=-1)
        te, to = self._conv(m, k_even, None, 1), self._conv(m, k_odd, None, 1)
        odd = (torch.arange(m.shape[-1]) % 2 == 1).view(*([1] * (m.dim() - 1)), -1)
        return torch.where(odd, to, te)

    def shuffle(self, v, u):
        return tuple(_shuffle(t, u, self.is3d) for t in v)

    def act(self, v, kind):
        a, e = v
        if kind in ("relu", "relu6"):
            # 1-Lipschitz, and flat outside [0, 6]: where the whole interval a +- e lies below 0 (above 6) both
            # evaluations give 0 (6) exactly, and where it straddles the kink the error is at most the part beyond it
            top = 6.0 if kind == "relu6" else math.inf
            eo = self.torch.minimum(e, self.torch.minimum((a + e).clamp(min=0.0), (top - a + e).clamp(min=0.0)))
            return a.clamp(0.0, top), eo
        # 1 / (1 + expf(-v)) (conv.hip conv_act): ocml's expf taken to be within 1 ulp (2u), the add and the division one
        # rounding each -- 4u relative to first order; 5u covers the second-order terms. sigma(a_hat) <= sigma(a) + e / 4.
        s = self.torch.sigmoid(a)
        return s, 0.25 * e + 5 * U32 * (s + 0.25 * e)

    def pool(self, v, k, kind):
        a, e = v
        F = self.F
        if kind == "max":       # |max(a_hat) - max(a)| <= max |a_hat - a|
            mp = F.max_pool3d if self.is3d else F.max_pool2d
            return mp(a, k), mp(e, k)
        return self.avg2(v)

    def avg2(self, v):
        # k_avg_pool2 / k_pool2_ex: a 2^dim window summed pairwise (at most dim roundings per term: gamma(2^dim - 1) is
        # larger), the power-of-two scaling exact
        a, e = v
        ap = self.F.avg_pool3d if self.is3d else self.F.avg_pool2d
        return ap(a, 2), ap(e, 2) + gamma(2 ** self.dim - 1) * ap(a.abs() + e, 2)

    def bn(self, v, d):
        # model_build.cpp bn_fold: sc = w / sqrt(var + eps), sh = b - mean sc in fp64, each rounded to fp32 once; y = fmaf(v, sc, sh)
        a, e = v
        sh_ = (1, -1) + (1,) * self.dim
        wt = np.ones_like(d["running_mean"], np.float64) if d.get("weight") is None else np.asarray(d["weight"], np.float64)
        bi = np.zeros_like(wt) if d.get("bias") is None else np.asarray(d["bias"], np.float64)
        sc = wt / np.sqrt(np.asarray(d["running_var"], np.float64) + d["eps"])
        sh = bi - np.asarray(d["running_mean"], np.float64) * sc
        sc_t, sh_t = self._t(sc).view(sh_), self._t(sh).view(sh_)
        y = a * sc_t + sh_t
        m = a.abs() + e
        err = sc_t.abs() * (1 + U32) * e + U32 * (sc_t.abs() * m + sh_t.abs()) \
            + U32 * (1 + U32) * (sc_t.abs() * m + sh_t.abs())
        return y, err

    def up_nearest(self, v, f):
        return tuple(self.F.interpolate(t, scale_factor=f, mode="nearest") for t in v)

    def concat(self, vs):
        torch = self.torch
        return torch.cat([a for a, _ in vs], dim=1), torch.cat([e for _, e in vs], dim=1)

    def add(self, x, y):
        s = x[0] + y[0]
        es = x[1] + y[1]
        return s, es + U32 * (s.abs() + es)

    def cat_skip(self, v, skip):
        return self.concat([v, skip])


def _update_plan(flags, is3d):
    """velocityUpdateForward's decisions per cell and component (tfluids.cc:1072-1156, model.hip k_project): for every
    component c, 'sub' = u -= pC - pN, 'subc' = u -= pC, 'addn' = u = u + pN, 'zero' = u = 0, else untouched."""
    B, _, Z, Y, X = flags.shape
    f = flags[:, 0].astype(np.int64)
    inner = np.zeros((B, Z, Y, X), bool)
    if is3d:
        inner[:, 1:Z - 1, 1:Y - 1, 1:X - 1] = True
    else:
        inner[:, :, 1:Y - 1, 1:X - 1] = True
    C = 3 if is3d else 2
    plan = []
    for c in range(C):
        ax = 3 - c                     # x, y, z neighbour below
        fn = np.roll(f, 1, axis=ax)
        fluid, empty = (f & FLUID) != 0, ((f & EMPTY) != 0) & ((f & OUTFLOW) == 0)
        nfl, nem = (fn & FLUID) != 0, (fn & EMPTY) != 0
        plan.append(dict(sub=inner & fluid & nfl, subc=inner & fluid & ~nfl & nem,
                         addn=inner & ~fluid & empty & nfl, zero=inner & ~fluid & empty & ~nfl))
    return plan


def _neighbour(p, c):
    return np.roll(p, 1, axis=4 - c)


def forward_bound(ops, model, pDiv, UDiv, flags, path=None, conv_env=None):
    """(p64, U64, bound_p, bound_U, info) for model.forward([pDiv, UDiv, flags]) on conv path `path` (default: the one
    conv_path(model, conv_env) names). info: the fp32 restatement's scale, the mask of U components velocityUpdate leaves
    untouched (where the GPU must equal the restatement bit for bit), max |activation| per hidden layer (fp64)."""
    import torch
    path = path or conv_path(model, conv_env)
    o = S.model_opts(model.opts)
    ic = o["inputChannels"]
    is3d = UDiv.shape[1] == 3
    U_bc = UDiv.copy()
    ops.setWallBcsForward(U_bc, flags)
    div = np.zeros_like(pDiv)
    ops.velocityDivergenceForward(U_bc, flags, div)
    if o["normalizeInput"]:
        src = {"UDiv": U_bc, "pDiv": pDiv, "div": div}[o["normalizeInputChan"]]
        if o["normalizeInputFunc"] == "std":
            scale = S.input_scale(src)
        else:
            x2 = src.reshape(src.shape[0], -1).astype(np.float64)
            scale = np.sqrt((x2 * x2).sum(1)).astype(np.float32)
    else:
        scale = np.ones(pDiv.shape[0], np.float32)
    s64 = scale.astype(np.float64).reshape(-1, 1, 1, 1, 1)
    occ = np.zeros_like(pDiv)
    ops.flagsToOccupancy(flags, occ)
    chans, errs = [], []
    for on, f in ((ic["pDiv"], pDiv), (ic["UDiv"], U_bc), (ic["div"], div)):
        if on:
            x = f.astype(np.float64) / s64
            chans.append(x)
            errs.append(2 * U32 * np.abs(x))
    chans.append(occ.astype(np.float64))
    errs.append(np.zeros_like(chans[-1]))
    x64, e64 = np.concatenate(chans, 1), np.concatenate(errs, 1)
    sk = None
    if o["addPressureSkip"]:
        s = pDiv.astype(np.float64) / s64
        sk = (torch.from_numpy(s), torch.from_numpy(2 * U32 * np.abs(s)))
        if not is3d:
            sk = tuple(t[:, :, 0] for t in sk)
    h = (torch.from_numpy(x64), torch.from_numpy(e64))
    if not is3d:
        h = tuple(t[:, :, 0] for t in h)
    ev = BoundEval(model, path)
    acts = []
    orig_act = ev.act

    def act(v, kind):
        r = orig_act(v, kind)
        acts.append(float(r[0].abs().max()))
        return r
    ev.act = act
    pp, ep = Walker(model).run(ev, h, sk)
    if not is3d:
        pp, ep = pp.unsqueeze(2), ep.unsqueeze(2)
    pp, ep = pp.numpy(), ep.numpy()

    # p = pPred * scale: one rounding, and the scale's 1 ulp (2u)
    p64 = pp * s64
    bound_p = s64 * ep * (1 + 3 * U32) + 3.01 * U32 * np.abs(p64)
    # U = SetWallBcs((U_bc / scale - grad pPred) * scale), each step one rounding
    u0 = U_bc.astype(np.float64) / s64
    eu = 3.01 * U32 * np.abs(u0)                         # the division and the scale's ulp
    U64 = u0.copy()
    EU = eu.copy()
    untouched = np.ones(U_bc.shape, bool)
    pl = _update_plan(flags, is3d)
    pc, ec = pp[:, 0], ep[:, 0]
    for c, P in enumerate(pl):
        pn, en = _neighbour(pp, c)[:, 0], _neighbour(ep, c)[:, 0]
        uc, e_uc = U64[:, c], EU[:, c]
        d = pc - pn
        ed = ec + en + U32 * (np.abs(d) + ec + en)
        for key, val, ev_ in (("sub", uc - d, e_uc + ed), ("subc", uc - pc, e_uc + ec), ("addn", uc + pn, e_uc + en)):
            msk = P[key]
            val_e = ev_ + U32 * (np.abs(val) + ev_)
            uc = np.where(msk, val, uc)
            e_uc = np.where(msk, val_e, e_uc)
        touched = P["sub"] | P["subc"] | P["addn"]
        uc = np.where(P["zero"], 0.0, uc)
        e_uc = np.where(P["zero"], 0.0, e_uc)
        U64[:, c], EU[:, c] = uc, e_uc
        untouched[:, c] = ~touched
    U64 = U64 * s64
    bound_U = s64 * EU * (1 + 3 * U32) + 3.01 * U32 * np.abs(U64)
    wall = np.ones(U_bc.shape, np.float32)
    ops.setWallBcsForward(wall, flags)
    assert np.isin(wall, (0.0, 1.0)).all(), "setWallBcs is not a pure zeroing here"
    z = wall == 0
    U64[z] = 0.0
    bound_U[z] = 0.0
    untouched |= z
    return p64, U64, bound_p, bound_U, dict(scale=scale, untouched=untouched, acts=acts, path=path)


def worst(got, want, bound):
    """(max err / bound, flat index of the worst voxel): a voxel with err > 0 where the bound is 0 counts as infinitely over."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r.flat[i]), i


def report(name, got, want, bound, tile=(32, 8, 4)):
    """one line on the worst voxel of `got` against (want, bound): index (b, c, z, y, x), values, bound and the tile
    (tx, ty, tz of the given tile size) it lies in"""
    r, i = worst(got, want, bound)
    idx = np.unravel_index(i, got.shape)
    b, c, z, y, x = idx
    return ("%s: max err/bound %.3g at (b=%d c=%d z=%d y=%d x=%d) got %.9g fp64 %.9g bound %.3g tile (%d, %d, %d)"
            % (name, r, b, c, z, y, x, float(got[idx]), float(want[idx]), float(bound[idx]),
               x // tile[0], y // tile[1], z // tile[2]))
