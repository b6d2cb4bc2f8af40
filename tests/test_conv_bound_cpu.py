"""CPU checks of the per-voxel error bound of tests/conv_bound.py, before any GPU run trusts it: faithful fp32 evaluations
(an fmaf chain tap by tap, and an emulation of conv_mfma16.hip's split-fp16 arithmetic) lie inside it at every voxel; five
mutants of the kind tiled kernels produce -- a mis-addressed tap in the last ragged tile, a flipped kernel, an early edge,
another sample's scale, the wrong out-of-range scale branch -- fall outside it; and the aggregate fp64 witness, which a
worst-case bound cannot replace, tells the split operands from fp16-only ones."""
import numpy as np
import pytest
import torch

import conv_bound as CB
import model_graph_ref as R
import scenes
from fluidnet_amd import FluidNetModel
from oracle import simulate_np as S


def f32(t):
    return t.to(torch.float64).to(torch.float32)


class Fp32Eval:
    """A plain fp32 evaluation: each conv an fmaf chain from the bias, tap by tap and input channel by input channel (an
    fmaf emulated as the exact fp64 product-sum rounded to fp32), everything else in fp32 torch."""

    def __init__(self, model):
        self.model, self.is3d = model, model.is3D
        self.dim = 3 if model.is3D else 2

    def taps(self, w, dil):
        k = w.shape[-1]
        r = (k - 1) // 2
        rz = r if self.is3d else 0
        for dz in range(-rz, rz + 1):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yield dz, dy, dx, (w[:, :, dz + rz, dy + r, dx + r] if self.is3d else w[:, :, dy + r, dx + r])

    def shifted(self, h, dz, dy, dx, dil):
        """h read at (z + dz dil, y + dy dil, x + dx dil), zero outside the grid"""
        out = torch.zeros_like(h)
        sh = (dz * dil, dy * dil, dx * dil) if self.is3d else (dy * dil, dx * dil)
        src, dst = [], []
        for s, n in zip(sh, h.shape[2:]):
            src.append(slice(max(s, 0), n + min(s, 0)))
            dst.append(slice(max(-s, 0), n + min(-s, 0)))
        out[(slice(None), slice(None)) + tuple(dst)] = h[(slice(None), slice(None)) + tuple(src)]
        return out

    def conv(self, h, li, w, b, dil):
        wt = torch.from_numpy(np.asarray(w, np.float32)).to(torch.float64)
        acc = torch.from_numpy(np.asarray(b, np.float32)).view(1, -1, *([1] * self.dim)).expand(h.shape[0], -1, *h.shape[2:])
        acc = acc.clone()
        for dz, dy, dx, g in self.taps(wt, dil):
            hs = self.shifted(h, dz, dy, dx, dil).to(torch.float64)
            for ci in range(h.shape[1]):
                acc = f32(acc.to(torch.float64) + g[:, ci].view(1, -1, *([1] * self.dim)) * hs[:, ci:ci + 1])
        return acc

    def shuffle(self, h, u):
        return CB._shuffle(h, u, self.is3d)

    def act(self, h, kind):
        if kind == "relu":
            return h.clamp(min=0.0)
        if kind == "relu6":
            return h.clamp(0.0, 6.0)
        return torch.sigmoid(h)

    def pool(self, h, k, kind):
        if kind == "max":
            return (torch.nn.functional.max_pool3d if self.is3d else torch.nn.functional.max_pool2d)(h, k)
        return self.avg2(h)

    def avg2(self, h):
        return (torch.nn.functional.avg_pool3d if self.is3d else torch.nn.functional.avg_pool2d)(h, 2)

    def bn(self, h, d):
        wt = np.ones_like(d["running_mean"], np.float64) if d.get("weight") is None else np.asarray(d["weight"], np.float64)
        bi = np.zeros_like(wt) if d.get("bias") is None else np.asarray(d["bias"], np.float64)
        sc = wt / np.sqrt(np.asarray(d["running_var"], np.float64) + d["eps"])
        sh = bi - np.asarray(d["running_mean"], np.float64) * sc
        v = (1, -1) + (1,) * self.dim
        sct = torch.from_numpy(sc.astype(np.float32)).view(v).to(torch.float64)
        sht = torch.from_numpy(sh.astype(np.float32)).view(v).to(torch.float64)
        return f32(h.to(torch.float64) * sct + sht)

    def up_nearest(self, h, f):
        return torch.nn.functional.interpolate(h, scale_factor=f, mode="nearest")

    def concat(self, hs):
        return torch.cat(hs, dim=1)

    def add(self, a, b):
        return a + b

    def cat_skip(self, h, skip):
        return torch.cat([h, skip], dim=1)


def _split(t):
    """conv_mfma16.hip split_h: (fp16(a), fp16((a - fp16(a)) 2^11)) as fp64 tensors"""
    hi = t.to(torch.float16).to(torch.float32)
    lo = ((t - hi) * 2048.0).to(torch.float16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


class M16Eval(Fp32Eval):
    """conv_mfma16.hip's arithmetic for the layers it runs (the three k = 3 layers and the tail's 8 -> 8): weights scaled by
    2^e and split as conv3_m16_pack_weights, activations as split_h, the exact products of the halves accumulated into two
    fp32 accumulators per output channel (w_h row, w_l row) one MFMA at a time (the products of one (dz, dy) row and one
    activation term summed exactly, as a K = 32 block, then added to the accumulator with one fp32 rounding), then
    fma(fma(D1, 2^-11, D0), 2^-(11+e), bias). lo=False drops the low halves: fp16-only operands."""

    def __init__(self, model, lo=True):
        super().__init__(model)
        self.lo = lo

    def conv(self, h, li, w, b, dil):
        if li >= 4:
            return super().conv(h, li, w, b, dil)
        e = CB.m16_exponent(w)
        ws = torch.from_numpy(np.ldexp(np.asarray(w, np.float32), e))
        wh, wl = _split(ws)
        ah_all, al_all = _split(h.to(torch.float32))
        if not self.lo:
            wl, al_all = torch.zeros_like(wl), torch.zeros_like(al_all)
        B = h.shape[0]
        D = [torch.zeros((B, w.shape[0]) + tuple(h.shape[2:]), dtype=torch.float32) for _ in range(2)]
        k = w.shape[-1]
        r = (k - 1) // 2
        for dz in range(-r, r + 1):
            for dy in range(-r, r + 1):
                for term in (0, 1):
                    for t, wt in enumerate((wh, wl)):
                        blk = torch.zeros_like(D[t], dtype=torch.float64)
                        for dx in range(-r, r + 1):
                            a = self.shifted(ah_all if term == 0 else al_all, dz, dy, dx, dil)
                            g = wt[:, :, dz + r, dy + r, dx + r] * (2048.0 if term == 0 else 1.0)
                            blk += torch.einsum("oc,bczyx->bozyx", g, a)
                        D[t] = f32(D[t].to(torch.float64) + blk)
        t = f32(D[1].to(torch.float64) * 2.0 ** -11 + D[0].to(torch.float64))
        bias = torch.from_numpy(np.asarray(b, np.float32)).view(1, -1, 1, 1, 1).to(torch.float64)
        return f32(t.to(torch.float64) * 2.0 ** -(11 + e) + bias)


def _run(ops, model, sc, ev, mutate_x=None):
    """(p, U) of oracle/simulate_np.model_forward with its conv stack evaluated by `ev` (mutate_x: the net input changed
    on its way into the stack); ev = None: a net that predicts pPred = NaN everywhere, so that every U component that
    depends on it comes out NaN"""
    saved = S.conv_stack

    def stack(x, layers, is3d, dtype="float32", pool=None, up=None, nonlin="relu", skip=None):
        if mutate_x is not None:
            x = mutate_x(x)
        if ev is None:
            return np.full((x.shape[0], 1) + x.shape[2:], np.nan, np.float32)
        h = torch.from_numpy(np.ascontiguousarray(x))
        sk = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip))
        if not is3d:
            h = h[:, :, 0]
            sk = None if sk is None else sk[:, :, 0]
        out = CB.Walker(model).run(ev, h, sk)
        if not is3d:
            out = out.unsqueeze(2)
        return out.to(torch.float32).numpy()
    S.conv_stack = stack
    try:
        return S.model_forward(ops, model.layers, sc["p"], sc["U"], sc["flags"], opts=model.opts)
    finally:
        S.conv_stack = saved


def _layers2d():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "myModel2D_weights.npz"))
    return [(z["w%d" % i], z["b%d" % i]) for i in range(5)]


def _mconf(n, bt, agg, bn, **kw):
    m = dict(banksNum=n, banksType=bt, banksAggregateMethod=agg, banksSplitStage=2, banksJoinStage=4)
    m.update(kw)
    if bn != "off":
        m.update(addBatchNorm=True, batchNormAffine=bn == "affine")
    return m


# every topology of the GPU matrix (tests/test_hip_conv_bound.py), small grids
TOPOLOGIES = {
    "default3d": (lambda: FluidNetModel.default_3d(seed=3), (5, 9, 33)),
    "default2d": (lambda: FluidNetModel(_layers2d(), False), (1, 17, 33)),
    "tog3d": (lambda: FluidNetModel.tog(True, seed=9), (4, 8, 16)),
    "tog2d": (lambda: FluidNetModel.tog(False, seed=9), (1, 16, 34)),
    "yang3d": (lambda: FluidNetModel.from_mconf(dict(modelType="yang"), True, seed=4), (5, 9, 17)),
    "yang2d": (lambda: FluidNetModel.from_mconf(dict(modelType="yang"), False, seed=4), (1, 17, 33)),
    "relu6": (lambda: FluidNetModel.from_mconf(dict(nonlinType="relu6"), True, seed=2), (5, 9, 17)),
    "sigmoid": (lambda: FluidNetModel.from_mconf(dict(nonlinType="sigmoid"), True, seed=2), (5, 9, 17)),
    "skip_norm_udiv": (lambda: FluidNetModel.from_mconf(dict(addPressureSkip=True, normalizeInputFunc="norm",
                                                             inputChannels=dict(UDiv=True)), True, seed=2), (5, 9, 17)),
    "mres_concat_affine": (lambda: FluidNetModel.from_mconf(_mconf(2, "mres", "concat", "affine"), True, seed=2), (4, 8, 16)),
    "dilate_add_plain": (lambda: FluidNetModel.from_mconf(_mconf(2, "dilate", "add", "plain"), True, seed=3), (5, 9, 17)),
    "tog_banks_max": (lambda: FluidNetModel.from_mconf(dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5,
                                                            poolType="max", addBatchNorm=True), True, seed=9), (8, 16, 32)),
}


def _forward64(oracle, model, sc, path):
    return CB.forward_bound(oracle, model, sc["p"], sc["U"], sc["flags"], path=path)


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_bound_holds_for_faithful_fp32_evaluations(oracle, name):
    build, dims = TOPOLOGIES[name]
    model = build()
    for kind in ("smooth", "rough"):
        sc = scenes.make_scene(dims, seed=5, vel_cells=0.4, B=2) if kind == "smooth" else scenes.rough_scene(dims, seed=5, B=2)
        path = CB.conv_path(model)
        p64, U64, bp, bU, info = _forward64(oracle, model, sc, path)
        evs = [("fp32", Fp32Eval(model))]
        if path == "mfma16":
            evs.append(("mfma16", M16Eval(model)))
        for en, ev in evs:
            p, U = _run(oracle, model, sc, ev)
            rp, _ = CB.worst(p, p64, bp)
            rU, _ = CB.worst(U, U64, bU)
            print("%s %s %s: max err/bound p %.3g U %.3g" % (name, kind, en, rp, rU))
            assert rp <= 1.0, CB.report(en + " p", p, p64, bp)
            assert rU <= 1.0, CB.report(en + " U", U, U64, bU)
        # the restatement (PyTorch-CPU fp32) is an fp32 evaluation too, and where velocityUpdate leaves U alone it is
        # (U_bc / scale) * scale, independent of the net
        if model.graph is None:
            pr, Ur = S.model_forward(oracle, model.layers, sc["p"], sc["U"], sc["flags"], pool=model.pool, up=model.up,
                                     opts=model.opts)
        else:
            pr, Ur = R.model_forward(oracle, model, sc["p"], sc["U"], sc["flags"])
        assert CB.worst(pr, p64, bp)[0] <= 1.0 and CB.worst(Ur, U64, bU)[0] <= 1.0
        zero_net = _run(oracle, model, sc, None)[1]
        m = info["untouched"]
        assert np.array_equal(Ur[m], zero_net[m])


def test_untouched_mask_is_exactly_what_the_net_does_not_reach(oracle):
    model = FluidNetModel.default_3d(seed=3)
    sc = scenes.rough_scene((6, 9, 17), seed=2, B=2)
    *_, info = _forward64(oracle, model, sc, "fp32")
    _, U = _run(oracle, model, sc, None)
    assert np.array_equal(np.isfinite(U), info["untouched"])


def test_bound_is_not_vacuous(oracle):
    """A worst-case bound cannot be as tight as the error it bounds, but it must stay small against the field: the largest
    bound is a small fraction of the largest |p|. (Not 1e-4: worst-case propagation multiplies by sum |W| over the layers --
    about 150 for default_3d, whose output is 3e-3 of its input; measured 1.1e-2 for mfma16, 2.7e-3 for fp32.)"""
    for build, dims, path, lim in [(lambda: FluidNetModel.default_3d(seed=3), (9, 17, 33), "mfma16", 3e-2),
                                   (lambda: FluidNetModel.default_3d(seed=3), (9, 17, 33), "fp32", 1e-2),
                                   (lambda: FluidNetModel.default_3d(seed=3), (9, 17, 33), "winograd", 1e-2),
                                   (lambda: FluidNetModel(_layers2d(), False), (1, 33, 65), "mfma", 1e-2)]:
        model = build()
        sc = scenes.make_scene(dims, seed=1, vel_cells=0.4, B=2)
        p64, _, bp, _, _ = _forward64(oracle, model, sc, path)
        ratio = float(bp.max() / np.abs(p64).max())
        print("%s %s: max bound_p / max |p64| = %.3g" % (path, dims, ratio))
        assert ratio <= lim, (path, ratio)


class _TapOff(Fp32Eval):
    """layer 1 reads its dx = +1 tap one voxel too far, only in the last ragged 32-wide x-tile"""

    def conv(self, h, li, w, b, dil):
        out = super().conv(h, li, w, b, dil)
        if li != 1:
            return out
        X = h.shape[-1]
        x0 = (X - 1) // 32 * 32
        assert 0 < X - x0 < 32
        wt = torch.from_numpy(np.asarray(w, np.float32)).to(torch.float64)
        fix = torch.zeros_like(out, dtype=torch.float64)
        for dz, dy, dx, g in self.taps(wt, dil):
            if dx != 1:
                continue
            d = (self.shifted(h, dz, dy, 2, dil) - self.shifted(h, dz, dy, 1, dil)).to(torch.float64)
            fix += torch.einsum("oc,bczyx->bozyx", g, d)
        out = out.clone()
        out[..., x0:] = f32(out[..., x0:].to(torch.float64) + fix[..., x0:])
        return out


class _FlipZ(Fp32Eval):
    def conv(self, h, li, w, b, dil):
        return super().conv(h, li, np.ascontiguousarray(w[:, :, ::-1]) if li == 1 else w, b, dil)


class _EarlyEdge(Fp32Eval):
    """layer 1 zero-pads its input one column early: x = X - 1 reads as outside the grid"""

    def conv(self, h, li, w, b, dil):
        if li == 1:
            h = h.clone()
            h[..., -1] = 0.0
        return super().conv(h, li, w, b, dil)


def test_mutants_exceed_the_bound(oracle):
    model = FluidNetModel.default_3d(seed=3)
    sc = scenes.rough_scene((5, 9, 63), seed=7, B=2)
    sc["U"][1] *= 4.0           # the two samples' scales 4x apart
    p64, U64, bp, bU, info = _forward64(oracle, model, sc, "mfma16")
    p, _ = _run(oracle, model, sc, Fp32Eval(model))
    assert CB.worst(p, p64, bp)[0] <= 1.0
    s = info["scale"]
    nin = 2        # the scaled channels of the default net input {pDiv, div, occupancy}

    def other_scale(x):
        x = x.copy()
        x[0, :nin] = (x[0, :nin].astype(np.float64) * s[0] / s[1]).astype(np.float32)
        return x
    for name, ev, mut in [("tap off in the last x-tile", _TapOff(model), None), ("kernel flipped in z", _FlipZ(model), None),
                          ("last x-column padded early", _EarlyEdge(model), None),
                          ("sample 0 with sample 1's scale", Fp32Eval(model), other_scale)]:
        pm, Um = _run(oracle, model, sc, ev, mut)
        r, _ = CB.worst(pm, p64, bp)
        print("%s: max err/bound %.3g" % (name, r))
        assert r > 1.0, name
    # the out-of-range branch (scale outside [2^-12, 2^21]) multiplying by inv_scale, which is 0 there, instead of dividing
    for target in (2.0 ** -13, 2.0 ** 22 * 1.01):
        sc2 = dict(sc)
        f = np.float32(target / info["scale"][0])
        sc2["U"] = (sc["U"] * f).astype(np.float32)
        sc2["p"] = (sc["p"] * f).astype(np.float32)
        p64, _, bp, _, info2 = _forward64(oracle, model, sc2, "mfma16")
        assert not (2.0 ** -12 <= info2["scale"][0] <= 2.0 ** 21)

        def zero_scaled(x):
            x = x.copy()
            x[0, :nin] = 0.0
            return x
        assert CB.worst(_run(oracle, model, sc2, Fp32Eval(model))[0], p64, bp)[0] <= 1.0
        r, _ = CB.worst(_run(oracle, model, sc2, Fp32Eval(model), zero_scaled)[0], p64, bp)
        print("out-of-range branch times inv_scale (scale %.3g): max err/bound %.3g" % (info2["scale"][0], r))
        assert r > 1.0


def witness(p, p_ref, p64):
    """the aggregate fp64 witness: rel-L2 of p against the fp64 net, over PyTorch-CPU fp32's"""
    return scenes.rel_l2(p, p64), scenes.rel_l2(p_ref, p64)


def test_witness_tells_split_operands_from_fp16_only(oracle):
    """A per-voxel worst-case bound cannot tell fp16-only operands (2^-11 relative) from the split pairs, but the aggregate
    witness can: the split emulation passes it at 1.0x PyTorch fp32's error (the claim for the default 3-D path), the
    fp16-only one fails it. Smooth scenes of test_model_forward_matches_restatement, B = 1."""
    model = FluidNetModel.default_3d(seed=3)
    for dims, seed in [((12, 16, 20), 43), ((9, 17, 33), 44)]:
        sc = scenes.make_scene(dims, seed=seed, vel_cells=0.4)
        p_ref, _ = S.model_forward(oracle, model.layers, sc["p"], sc["U"], sc["flags"])
        p64, _ = S.model_forward(oracle, model.layers, sc["p"], sc["U"], sc["flags"], conv_dtype="float64")
        e16, et = witness(_run(oracle, model, sc, M16Eval(model, lo=False))[0], p_ref, p64)
        es, _ = witness(_run(oracle, model, sc, M16Eval(model))[0], p_ref, p64)
        print("witness %s: split %.3e, fp16-only %.3e, PyTorch fp32 %.3e" % (dims, es, e16, et))
        assert es <= 1.0 * et + 1e-8
        assert e16 > 1.0 * et + 1e-8 and e16 > 4.0 * et
