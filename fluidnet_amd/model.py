"""The pressure-projection ConvNet: host mirror of torch/lib/model.lua's `default` model.

`FluidNetModel.forward({pDiv, UDiv, flags}) -> {p, U}` has the call shape of the reference's
`model:forward(torch.getModelInput(batch))` (lib/model.lua:398, 421-450; lib/simulate.lua:262-272).
The graph (SetWallBcs -> divergence -> std-normalise -> conv stack -> VelocityUpdate -> un-scale ->
SetWallBcs) runs inside libtfluids_hip.so (tfl_model_forward); this class only owns the weights'
host copy, the device handle and the scratch tensor.
"""
import ctypes
import json
import math
import os
import re

import numpy as np
import torch

from . import _lib, tfluids, torch7
from ._lib import TfluidsError


# the mconf switches that change the forward graph, with torch/lib/default_conf.lua:60-100's defaults
DEFAULT_OPTS = dict(inputChannels=dict(pDiv=True, UDiv=False, div=True, flags=True), normalizeInput=True,
                    normalizeInputChan="UDiv", normalizeInputFunc="std", nonlinType="relu", addPressureSkip=False)


def _resolve_opts(opts):
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULT_OPTS.items()}
    for k, v in (opts or {}).items():
        if k == "inputChannels":
            o[k].update(v)
        elif k in o:
            o[k] = v
        else:
            raise TfluidsError("unknown model option %r" % (k,))
    if not o["inputChannels"]["flags"]:
        raise TfluidsError("Are you sure you dont want flags?")                       # lib/model.lua:81
    for key, allowed in (("normalizeInputChan", ("UDiv", "pDiv", "div")), ("normalizeInputFunc", ("std", "norm")),
                         ("nonlinType", ("relu", "relu6", "sigmoid"))):
        if o[key] not in allowed:
            raise TfluidsError("bad %s %r (one of %s)" % (key, o[key], ", ".join(allowed)))
    return o


# the mconf switches of lib/model.lua:253-392 that add banks, batch norm or max pooling, with default_conf.lua:40-120's defaults
DEFAULT_GRAPH = dict(banksNum=1, banksType="mres", banksAggregateMethod="concat", banksSplitStage=1, banksJoinStage=3,
                     banksWeightShare=False, poolType="avg", addBatchNorm=False, batchNormAffine=True, batchNormEps=1e-4,
                     bn=None)

# lib/model.lua:163-236: (osize, ksize, psize, usize) of each modelType, 2-D / 3-D
_LAYER_TABLES = {
    ("default", False): ([16, 16, 16, 16, 1], [3, 3, 3, 3, 1], [1] * 5, [1] * 5),
    ("default", True): ([8, 8, 8, 8, 1], [3, 3, 3, 1, 1], [1] * 5, [1] * 5),
    ("yang", False): ([6, 6, 6, 1], [3, 1, 1, 1], [1] * 4, [1] * 4),
    ("yang", True): ([6, 6, 6, 1], [3, 1, 1, 1], [1] * 4, [1] * 4),
    ("tog", False): ([16, 32, 32, 64, 64, 32, 1], [5, 5, 5, 5, 1, 1, 3], [2, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 2]),
    ("tog", True): ([16, 16, 16, 16, 32, 32, 1], [3, 3, 3, 3, 1, 1, 3], [2, 2, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 2, 2]),
}


def _resolve_graph(graph):
    g = dict(DEFAULT_GRAPH)
    for k, v in (graph or {}).items():
        if k not in g:
            raise TfluidsError("unknown model graph field %r" % (k,))
        g[k] = v
    if g["banksWeightShare"]:
        raise TfluidsError("weight sharing not supported for dilated conv networks.")      # model.lua:326-328
    for key, allowed in (("banksType", ("mres", "dilate")), ("banksAggregateMethod", ("concat", "add")),
                         ("poolType", ("avg", "max"))):
        if g[key] not in allowed:
            raise TfluidsError("bad %s %r (one of %s)" % (key, g[key], ", ".join(allowed)))
    g["banksNum"] = int(g["banksNum"])
    return g


def conv_modules(nstages, graph):
    """(stage, bank) of every conv module in lib/model.lua's creation order (1-based stage, 0-based bank)."""
    n = graph["banksNum"]
    out = []
    for st in range(1, nstages + 1):
        nb = n if n > 1 and graph["banksSplitStage"] <= st < graph["banksJoinStage"] else 1
        out.extend((st, b) for b in range(nb))
    return out


class FluidNetModel:
    def __init__(self, layers, is3D, pool=None, up=None, opts=None, graph=None):
        """layers: [(weight[nOut, nIn, k(,k),k], bias[nOut])] in forward order (numpy float32),
        weight layout as cudnn.{Spatial,Volumetric}Convolution.weight. pool / up: per-layer psize / usize of
        lib/model.lua's layer tables (1 or 2; None = all 1): 2x average pooling after a layer, or the layer is an
        nn.{Spatial,Volumetric}ConvolutionUpsample (its weight then has nOut * 2^dim output channels).
        opts: mconf fields that change the forward graph (lib/model.lua:27-160, 356-387), defaults as
        default_conf.lua: inputChannels={pDiv,UDiv,div,flags}, normalizeInput, normalizeInputChan ('UDiv'|'pDiv'|'div'),
        normalizeInputFunc ('std'|'norm'), nonlinType ('relu'|'relu6'|'sigmoid'), addPressureSkip.
        graph: mconf's own fields for banks, batch norm and pooling (lib/model.lua:253-392): banksNum, banksType
        ('mres'|'dilate'), banksAggregateMethod ('concat'|'add'), banksSplitStage, banksJoinStage, poolType ('avg'|'max'),
        addBatchNorm, plus `bn`: one dict {running_mean, running_var, weight, bias, eps} per hidden conv module (weight /
        bias None when not affine). `layers`, `pool` and `up` then list the conv modules in the reference's creation order:
        the stages before the split, bank 1..banksNum of every banked stage, the rest (tfl_model_create_graph)."""
        self.opts = _resolve_opts(opts)
        self.graph = None if graph is None else _resolve_graph(graph)
        self.is3D = bool(is3D)
        self.layers = [(np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32))
                       for w, b in layers]
        n = len(self.layers)
        self.pool = [1] * n if pool is None else [int(v) for v in pool]
        self.up = [1] * n if up is None else [int(v) for v in up]
        if len(self.pool) != n or len(self.up) != n:
            raise TfluidsError("pool / up need one entry per layer")
        for w, _ in self.layers:
            if w.ndim != (5 if self.is3D else 4):
                raise TfluidsError("weight rank does not match is3D")
        self._handles = {}   # device index -> tfl_model*
        self._work = {}      # device index -> scratch tensor

    # -- constructors ------------------------------------------------------------------------
    @classmethod
    def from_torch7(cls, path):
        """Load a model saved by torch.saveModel (lib/model.lua:463-478), e.g. data/models/myModel2D. With the
        `path + "_mconf.bin"` that torch.saveModel writes beside it, this is load_model(path)[1]: the whole graph and the
        forward options. Without it, a graph holding batch norm, dilated, pooling, upsampling or banked nodes is refused
        (the bank layout is in the mconf); any other graph is its convolutions in node order."""
        if os.path.exists(path + "_mconf.bin"):
            return load_model(path)[1]
        gm = torch7.load(path)
        if torch7.needs_graph(gm):
            raise TfluidsError("%s holds batch-norm / dilated / pooling / banked nodes: its %s_mconf.bin is needed to "
                               "build it (fluidnet_amd.load_model)" % (path, os.path.basename(path)))
        layers = torch7.conv_layers(gm)
        if not layers:
            raise TfluidsError("no convolution layers found in " + path)
        return cls(layers, is3D=layers[0][0].ndim == 5)

    @classmethod
    def from_mconf(cls, mconf, is3D, seed=1):
        """Seeded stand-in for any defineModelGraph configuration (lib/model.lua:27-392): modelType 'default' | 'yang' |
        'tog' with any of the graph knobs (DEFAULT_GRAPH) and forward options (DEFAULT_OPTS) read from `mconf`. With one
        bank and no batch norm the weights are those of default_3d(seed) / tog(is3D, seed); the BN statistics are drawn
        after all convolutions."""
        mt = mconf.get("modelType", "default")
        if (mt, bool(is3D)) not in _LAYER_TABLES:
            raise TfluidsError("Incorrect modelType for %dD model." % (3 if is3D else 2))
        osize, ksize, psize, usize = _LAYER_TABLES[(mt, bool(is3D))]
        opts = {k: mconf[k] for k in DEFAULT_OPTS if k in mconf}
        graph = _resolve_graph({k: mconf[k] for k in DEFAULT_GRAPH if k in mconf})
        ic = _resolve_opts(opts)["inputChannels"]
        dim = 3 if is3D else 2
        in_c = int(ic["pDiv"]) + int(ic["UDiv"]) * dim + int(ic["div"]) + 1
        scale = 0.5 if mt == "tog" else 0.35
        rng = np.random.RandomState(seed)
        mods = conv_modules(len(osize), graph)
        layers, pool, up = [], [], []
        for st, _ in mods:
            i = st - 1
            if st == 1:
                ci = in_c
            else:
                ci = osize[i - 1] * (graph["banksNum"] if graph["banksNum"] > 1 and st == graph["banksJoinStage"]
                                     and graph["banksAggregateMethod"] == "concat" else 1)
                ci += 1 if (_resolve_opts(opts)["addPressureSkip"] and st == len(osize)) else 0
            co, k, u = osize[i], ksize[i], usize[i]
            fan = ci * k ** dim
            w = (rng.randn(co * u ** dim, ci, *([k] * dim)) * scale * math.sqrt(2.0 / fan)).astype(np.float32)
            b = (rng.randn(co * u ** dim) * 0.01).astype(np.float32)
            layers.append((w, b))
            pool.append(psize[i])
            up.append(usize[i])
        if graph["addBatchNorm"] and graph["bn"] is None:
            bn = []
            for st, _ in mods[:-1]:
                co = osize[st - 1]
                bn.append(dict(running_mean=(rng.randn(co) * 0.1).astype(np.float32),
                               running_var=rng.uniform(0.5, 1.5, co).astype(np.float32),
                               weight=(1.0 + rng.randn(co) * 0.1).astype(np.float32) if graph["batchNormAffine"] else None,
                               bias=(rng.randn(co) * 0.1).astype(np.float32) if graph["batchNormAffine"] else None,
                               eps=float(graph["batchNormEps"])))
            graph["bn"] = bn
        return cls(layers, is3D, pool=pool, up=up, opts=opts, graph=graph)

    @classmethod
    def from_npz(cls, path):
        """w0, b0, w1, b1, ... (cudnn layout) from an .npz. A file written by save_npz also holds `model_json`: is3D, pool / up,
        the forward options and the graph, so that a custom or banked model comes back as it was; a file without it is a
        linear model with the default options, its dimensionality read from the weights' rank."""
        z = np.load(path)
        n = len([k for k in z.files if re.fullmatch(r"w\d+", k)])
        layers = [(z["w%d" % i], z["b%d" % i]) for i in range(n)]
        if "model_json" not in z.files:
            return cls(layers, is3D=layers[0][0].ndim == 5)
        d = json.loads(str(z["model_json"]))
        graph = d.get("graph")
        if graph is not None and graph.get("bn") is not None:
            graph["bn"] = [{k: (None if v is None else float(v) if k == "eps" else np.asarray(v, np.float32)) for k, v in m.items()}
                           for m in graph["bn"]]
        return cls(layers, bool(d["is3D"]), pool=d.get("pool"), up=d.get("up"), opts=d.get("opts"), graph=graph)

    @staticmethod
    def npz_meta(path):
        """the caller's `meta` of a file written by save_npz (None where there is none)"""
        z = np.load(path)
        return json.loads(str(z["model_json"])).get("meta") if "model_json" in z.files else None

    def save_npz(self, path, meta=None, extra=None):
        """The counterpart of from_npz: weights and biases under the keys it reads, plus one JSON string `model_json` = {is3D,
        pool, up, opts, graph (batch-norm statistics included), meta}. meta: anything json can hold, kept for the caller
        (npz_meta). extra: further arrays under keys of their own (a checkpoint's optimiser moments; not w<i> / b<i>).
        Written to `path` exactly (no .npz is appended), through a temporary file beside it."""
        graph = None
        if self.graph is not None:
            graph = dict(self.graph)
            if graph.get("bn") is not None:
                graph["bn"] = [{k: (None if v is None else float(v) if k == "eps" else [float(x) for x in np.asarray(v, np.float32).ravel()])
                                for k, v in m.items()} for m in graph["bn"]]
        d = dict(is3D=self.is3D, pool=self.pool, up=self.up, opts=self.opts, graph=graph, meta=meta)
        arrays = {}
        for i, (w, b) in enumerate(self.layers):
            arrays["w%d" % i], arrays["b%d" % i] = w, b
        for k, v in (extra or {}).items():
            if re.fullmatch(r"[wb]\d+", k) or k == "model_json":
                raise TfluidsError("save_npz: extra key %r collides with the model's own" % (k,))
            arrays[k] = np.asarray(v)
        arrays["model_json"] = np.array(json.dumps(d, default=lambda o: o.tolist()))      # (numpy scalars / arrays in opts or meta)
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            np.savez(f, **arrays)
        os.replace(tmp, path)

    @classmethod
    def default_3d(cls, seed=1, scale=0.35):
        """Seeded stand-in for a trained 3-D `default` model (the reference ships none): topology of
        lib/model.lua:219-226 (3->8 k3, 8->8 k3, 8->8 k3, 8->8 k1, 8->1 k1)."""
        rng = np.random.RandomState(seed)
        layers = []
        for co, ci, k in [(8, 3, 3), (8, 8, 3), (8, 8, 3), (8, 8, 1), (1, 8, 1)]:
            fan = ci * k ** 3
            w = (rng.randn(co, ci, k, k, k) * scale * math.sqrt(2.0 / fan)).astype(np.float32)
            b = (rng.randn(co) * 0.01).astype(np.float32)
            layers.append((w, b))
        return cls(layers, True)

    @classmethod
    def tog(cls, is3D, seed=1, scale=0.5):
        """Seeded stand-in for a trained `tog` model (none is shipped), single bank: the layer tables of
        lib/model.lua:163-178 (2-D) / :211-218 (3-D) -- pooling after the first layer(s), ConvolutionUpsample at the end."""
        if is3D:
            osize, ksize = [16, 16, 16, 16, 32, 32, 1], [3, 3, 3, 3, 1, 1, 3]
            psize, usize = [2, 2, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 2, 2]
        else:
            osize, ksize = [16, 32, 32, 64, 64, 32, 1], [5, 5, 5, 5, 1, 1, 3]
            psize, usize = [2, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 2]
        dim = 3 if is3D else 2
        rng = np.random.RandomState(seed)
        layers, ci = [], 3
        for co, k, u in zip(osize, ksize, usize):
            fan = ci * k ** dim
            w = (rng.randn(co * u ** dim, ci, *([k] * dim)) * scale * math.sqrt(2.0 / fan)).astype(np.float32)
            b = (rng.randn(co * u ** dim) * 0.01).astype(np.float32)
            layers.append((w, b))
            ci = co
        return cls(layers, is3D, pool=psize, up=usize)

    # -- device handle -----------------------------------------------------------------------
    def _handle(self, lib, ctx, dev):
        h = self._handles.get(dev)
        if h is None:
            n = len(self.layers)
            I32 = ctypes.c_int32 * n
            dim = 3 if self.is3D else 2
            cin = I32(*[w.shape[1] for w, _ in self.layers])
            cout = I32(*[w.shape[0] // (u ** dim) for (w, _), u in zip(self.layers, self.up)])
            ks = I32(*[w.shape[-1] for w, _ in self.layers])
            FP = ctypes.POINTER(ctypes.c_float)
            ws = (FP * n)(*[w.ctypes.data_as(FP) for w, _ in self.layers])
            bs = (FP * n)(*[b.ctypes.data_as(FP) for _, b in self.layers])
            o, ic = self.opts, self.opts["inputChannels"]
            copts = _lib.tfl_model_opts(int(ic["pDiv"]), int(ic["UDiv"]), int(ic["div"]), int(o["normalizeInput"]),
                                        ("UDiv", "pDiv", "div").index(o["normalizeInputChan"]),
                                        ("std", "norm").index(o["normalizeInputFunc"]),
                                        ("relu", "relu6", "sigmoid").index(o["nonlinType"]), int(o["addPressureSkip"]))
            if self.graph is None:
                h = lib.tfl_model_create_opts(ctx, int(self.is3D), n, cin, cout, ks, I32(*self.pool), I32(*self.up), ws, bs,
                                              ctypes.byref(copts))
            else:
                g, keep = self.graph, []
                cg = _lib.tfl_model_graph(g["banksNum"], ("mres", "dilate").index(g["banksType"]),
                                          ("concat", "add").index(g["banksAggregateMethod"]), int(g["banksSplitStage"]),
                                          int(g["banksJoinStage"]), ("avg", "max").index(g["poolType"]), int(g["addBatchNorm"]))
                if g["addBatchNorm"]:
                    bn = g["bn"] or []
                    if len(bn) != n - 1:
                        raise TfluidsError("addBatchNorm: %d BN modules for %d hidden conv modules" % (len(bn), n - 1))

                    def arr(key):
                        a = [None if d.get(key) is None else np.ascontiguousarray(d[key], np.float32) for d in bn]
                        keep.append(a)
                        return (FP * len(a))(*[None if x is None else x.ctypes.data_as(FP) for x in a])
                    cg.bn_mean, cg.bn_var, cg.bn_weight, cg.bn_bias = arr("running_mean"), arr("running_var"), arr("weight"), arr("bias")
                    cg.bn_eps = (ctypes.c_double * len(bn))(*[float(d.get("eps", 1e-5)) for d in bn])
                    keep.append((cg.bn_mean, cg.bn_var, cg.bn_weight, cg.bn_bias, cg.bn_eps))
                h = lib.tfl_model_create_graph(ctx, int(self.is3D), n, cin, cout, ks, I32(*self.pool), I32(*self.up), ws, bs,
                                               ctypes.byref(copts), ctypes.byref(cg))
            if not h:
                raise TfluidsError(lib.tfl_last_error(ctx).decode())
            if getattr(self, "_multires_training", False):
                # ProjectionNet(multires=True): the training-side forms of a linear model with pooling / upsampling layers
                if lib.tfl_model_enable_multires_training(ctx, h) != 0:
                    why = lib.tfl_last_error(ctx).decode()
                    lib.tfl_model_destroy(ctx, h)
                    raise TfluidsError(why)
            self._handles[dev] = h
        return h

    def forward(self, inputs, out=None, UBC=None, UBCInvMask=None, clamp=None):
        """inputs = [pDiv, UDiv, flags] -> [p, U]. `out=[p, U]` writes into given tensors (they may
        be the inputs themselves: simulate() copies the prediction back into the state anyway).
        UBC/UBCInvMask/clamp fuse simulate()'s trailing setConstVals + clamp into the last kernel."""
        pDiv, UDiv, flags = inputs
        tfluids._dims(UDiv, flags)
        tfluids._check(pDiv.shape == flags.shape and pDiv.is_contiguous(), "Size mismatch")
        tfluids._check((UDiv.size(1) == 3) == self.is3D, "model / input dimensionality mismatch")
        lib, ctx = tfluids._context(UDiv)
        dev = UDiv.device.index
        h = self._handle(lib, ctx, dev)
        B, _, Z, Y, X = flags.shape
        need = lib.tfl_model_workspace_floats(h, B, Z, Y, X)
        work = self._work.get(dev)
        if work is None or work.numel() < need:
            work = torch.empty(need, dtype=torch.float32, device=UDiv.device)
            self._work[dev] = work
        if out is None:
            p, U = torch.empty_like(pDiv), torch.empty_like(UDiv)
        else:
            p, U = out
        lo, hi = clamp if clamp is not None else (0.0, 0.0)
        from .simulate import wall_plan
        wall_plan(lib, ctx, flags)      # (the context finds it again by the flags' address: include/tfluids_hip.h tfl_wall_plan)
        rc = lib.tfl_model_forward(ctx, h, tfluids._tt(pDiv), tfluids._tt(UDiv), tfluids._tt(flags),
                                   tfluids._tt(p), tfluids._tt(U), ctypes.c_void_p(work.data_ptr()),
                                   work.numel(), tfluids._tt(UBC) if UBC is not None else None,
                                   tfluids._tt(UBCInvMask) if UBCInvMask is not None else None,
                                   int(clamp is not None), lo, hi)
        tfluids._call(lib, ctx, rc)
        return [p, U]

    __call__ = forward

    def range_errors(self, like):
        """Thread blocks of the fp16-MFMA convolution path that clamped an activation at the fp16 range since the last
        call (tfl_model_range_errors; synchronises). 0 for any working simulation; always 0 on the fp32 paths."""
        lib, ctx = tfluids._context(like)
        h = self._handles.get(like.device.index)
        return 0 if h is None else int(lib.tfl_model_range_errors(ctx, h))

    def range_flag(self, like):
        """The same count as far as the device has reported it, WITHOUT a stream synchronisation and without resetting it
        (tfl_model_range_flag): non-zero means a forward pass clamped activations at the fp16 range, and the next
        forward / simulate step of this model is refused (TFL_ERANGE) until range_errors() has been called. The strict-fp32
        stack without a range limit is TFL_CONV_PATH=winograd at model creation."""
        lib, ctx = tfluids._context(like)
        h = self._handles.get(like.device.index)
        return 0 if h is None else int(lib.tfl_model_range_flag(ctx, h))

    # -- the same forward in two halves, for z-slab decomposition (fluidnet_amd.dist) --------------
    def _prep(self, flags):
        lib, ctx = tfluids._context(flags)
        dev = flags.device.index
        h = self._handle(lib, ctx, dev)
        B, _, Z, Y, X = flags.shape
        need = lib.tfl_model_workspace_floats(h, B, Z, Y, X)
        work = self._work.get(dev)
        if work is None or work.numel() < need:
            work = torch.empty(need, dtype=torch.float32, device=flags.device)
            self._work[dev] = work
        return lib, ctx, h, work

    def begin(self, U, flags, zlo, zhi, stats):
        """SetWallBcs(U) in place + divergence + {sum u, sum u^2} over z-planes [zlo, zhi) into
        `stats` (float64 tensor [B, 2] on the device) -- the caller all-reduces it across ranks."""
        tfluids._dims(U, flags)
        tfluids._check(stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() >= 2 * U.size(0),
                       "stats must be a contiguous float64 [B, 2] tensor")
        lib, ctx, h, work = self._prep(flags)
        from .simulate import wall_plan
        wall_plan(lib, ctx, flags)
        tfluids._call(lib, ctx, lib.tfl_model_begin(ctx, h, tfluids._tt(U), tfluids._tt(flags), tfluids._tt(U),
                                                    ctypes.c_void_p(work.data_ptr()), work.numel(), int(zlo),
                                                    int(zhi), ctypes.c_void_p(stats.data_ptr())))

    def finish(self, p, U, flags, stats, count, UBC=None, UBCInvMask=None, clamp=None):
        """Everything after the (all-reduced) statistics: net input, conv stack, velocity update,
        un-scale, wall BCs (+ the fused setConstVals/clamp tail); p and U are updated in place."""
        lib, ctx, h, work = self._prep(flags)
        lo, hi = clamp if clamp is not None else (0.0, 0.0)
        tfluids._call(lib, ctx, lib.tfl_model_finish(
            ctx, h, tfluids._tt(p), tfluids._tt(flags), tfluids._tt(p), tfluids._tt(U),
            ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(stats.data_ptr()), float(count),
            tfluids._tt(UBC) if UBC is not None else None,
            tfluids._tt(UBCInvMask) if UBCInvMask is not None else None, int(clamp is not None), lo, hi))


def load_model(path):
    """(mconf, model) = torch.loadModel(path) (lib/model.lua:480-494): the gModule at `path` and the mconf table at
    `path + "_mconf.bin"`, walked by the nodes' annotations (torch7.model_graph) into a FluidNetModel with the graph's
    banks, dilation, pooling, batch norm and forward options. Unsupported nodes are refused by name."""
    gm = torch7.load(path)
    mconf = torch7.load(path + "_mconf.bin")
    if not isinstance(mconf, dict):
        raise TfluidsError("%s_mconf.bin is not an mconf table" % path)
    try:
        g = torch7.model_graph(gm, mconf)
    except torch7.GraphError as e:
        raise TfluidsError("%s: %s" % (path, e)) from None
    is3D = g["layers"][0][0].ndim == 5
    if bool(mconf.get("is3D", is3D)) != is3D:
        raise TfluidsError("%s: mconf.is3D does not match the convolutions" % path)
    graph = {k: mconf[k] for k in DEFAULT_GRAPH if k in mconf and k != "bn"}
    graph["poolType"] = g["poolType"] if any(p > 1 for p in g["pool"]) else graph.get("poolType", "avg")
    n = int(graph.get("banksNum", 1))
    split, join = int(graph.get("banksSplitStage", 1)), int(graph.get("banksJoinStage", 3))
    mods = conv_modules(g["stages"], dict(banksNum=n, banksSplitStage=split, banksJoinStage=join))
    if len(mods) != len(g["layers"]):
        raise TfluidsError("%s: %d convolution modules, the mconf's banks need %d" % (path, len(g["layers"]), len(mods)))
    dilate = n > 1 and graph.get("banksType", "mres") == "dilate"
    for (st, bank), d in zip(mods, g["dilation"]):
        if d != (2 ** bank if dilate else 1):
            raise TfluidsError("%s: stage %d bank %d has dilation %d, not what banksType %r builds"
                               % (path, st, bank + 1, d, graph.get("banksType")))
    has_bn = [b is not None for b in g["bn"]]
    if any(has_bn) and not all(has_bn):
        raise TfluidsError("%s: batch norm after some hidden stages only" % path)
    if bool(mconf.get("addBatchNorm")) != all(has_bn):
        raise TfluidsError("%s: mconf.addBatchNorm does not match the graph's batch-norm nodes" % path)
    graph["addBatchNorm"] = all(has_bn)
    graph["bn"] = g["bn"] if all(has_bn) else None
    opts = {k: mconf[k] for k in DEFAULT_OPTS if k in mconf}
    if "inputChannels" in opts:
        opts["inputChannels"] = {k: bool(v) for k, v in opts["inputChannels"].items()}
    plain = n == 1 and not graph["addBatchNorm"] and graph["poolType"] == "avg"
    model = FluidNetModel(g["layers"], is3D, pool=g["pool"], up=g["up"], opts=opts, graph=None if plain else graph)
    return mconf, model
