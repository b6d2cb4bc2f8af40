"""A small torch7 serialisation WRITER (the inverse of fluidnet_amd/torch7.py's reader, format in SURVEY.md Appendix A) and
a builder of gModule-shaped model files with lib/model.lua's node annotations and module fields, for the loader tests.

write(path, obj)                         any object the reader returns (tables, torch objects, tensors, numbers ...)
write_model(path, model, mconf, ...)     an nn.gModule + path_mconf.bin as torch.saveModel writes them, for a
                                         FluidNetModel built with any of defineModelGraph's knobs
"""
import struct

import numpy as np

from fluidnet_amd.model import conv_modules
from fluidnet_amd.torch7 import TorchObject, _ObjKey

_TENSOR = {np.dtype(np.float32): "Float", np.dtype(np.float64): "Double", np.dtype(np.int64): "Long",
           np.dtype(np.int32): "Int", np.dtype(np.uint8): "Byte"}


class _Writer:
    def __init__(self):
        self.out = []
        self.memo = {}

    def i32(self, v):
        self.out.append(struct.pack("<i", v))

    def string(self, s):
        b = s.encode("latin-1")
        self.i32(len(b))
        self.out.append(b)

    def _index(self, o):
        """(index, seen before)"""
        k = id(o)
        if k in self.memo:
            return self.memo[k][0], True
        self.memo[k] = (len(self.memo) + 1, o)     # keep `o` alive: its id must not be reused
        return self.memo[k][0], False

    def obj(self, o):
        if o is None:
            self.i32(0)
        elif isinstance(o, (bool, np.bool_)):
            self.i32(5)
            self.i32(1 if o else 0)
        elif isinstance(o, (int, float, np.integer, np.floating)):
            self.i32(1)
            self.out.append(struct.pack("<d", float(o)))
        elif isinstance(o, str):
            self.i32(2)
            self.string(o)
        elif isinstance(o, dict):
            self.i32(3)
            idx, seen = self._index(o)
            self.i32(idx)
            if seen:
                return
            self.i32(len(o))
            for k, v in o.items():
                self.obj(k.obj if isinstance(k, _ObjKey) else k)
                self.obj(v)
        elif isinstance(o, TorchObject):
            self.i32(4)
            idx, seen = self._index(o)
            self.i32(idx)
            if seen:
                return
            self.string("V 1")
            self.string(o.typename)
            self.obj(o.fields)
        elif isinstance(o, np.ndarray):
            a = np.ascontiguousarray(o)
            kind = _TENSOR[a.dtype]
            self.i32(4)
            idx, seen = self._index(o)
            self.i32(idx)
            if seen:
                return
            self.string("V 1")
            self.string("torch.%sTensor" % kind)
            self.i32(a.ndim)
            for s in a.shape:
                self.out.append(struct.pack("<q", s))
            for s in a.strides:
                self.out.append(struct.pack("<q", s // a.itemsize))
            self.out.append(struct.pack("<q", 1))
            self.i32(4)
            self.i32(len(self.memo) + 1)
            self.memo[("storage", idx)] = (len(self.memo) + 1, None)
            self.string("V 1")
            self.string("torch.%sStorage" % kind)
            self.out.append(struct.pack("<q", a.size))
            self.out.append(a.tobytes())
        else:
            raise TypeError("cannot serialise %r" % type(o))


def write(path, obj):
    w = _Writer()
    w.obj(obj)
    with open(path, "wb") as f:
        f.write(b"".join(w.out))


def _conv_module(w, b, is3d, up=1, dil=1):
    dim = 3 if is3d else 2
    k = w.shape[-1]
    nout = w.shape[0] // up ** dim
    f = dict(nInputPlane=w.shape[1], nOutputPlane=w.shape[0], kW=k, kH=k, dW=1, dH=1,
             padW=dil * (k - 1) // 2, padH=dil * (k - 1) // 2, weight=np.asarray(w, np.float32).copy(),
             bias=np.asarray(b, np.float32).copy(), train=False)
    if is3d:
        f.update(kT=k, dT=1, padT=dil * (k - 1) // 2)
    kind = "Volumetric" if is3d else "Spatial"
    if dil > 1:
        f.update(dilationW=dil, dilationH=dil, **({"dilationT": dil} if is3d else {}))
        return TorchObject("nn.%sDilatedConvolution" % kind, f)
    conv = TorchObject("cudnn.%sConvolution" % kind, f)
    if up == 1:
        return conv
    g = dict(nInputPlane=w.shape[1], nOutputPlane=nout, kW=k, kH=k, scaleW=up, scaleH=up, modules={1: conv}, train=False)
    if is3d:
        g.update(kT=k, scaleT=up)
    return TorchObject("nn.%sConvolutionUpsample" % kind, g)


def write_model(path, model, mconf, bn_train=False, gated=False, low_rank=False):
    """Write `model` (a FluidNetModel, layers in creation order) as the nn.gModule lib/model.lua:253-392 builds, and
    `mconf` as path_mconf.bin. bn_train / gated / low_rank plant what the loader must refuse."""
    is3d = model.is3D
    kind = "Volumetric" if is3d else "Spatial"
    g = model.graph or dict(banksNum=1, banksType="mres", banksAggregateMethod="concat", banksSplitStage=1,
                            banksJoinStage=3, poolType="avg", addBatchNorm=False, bn=None)
    n = g["banksNum"]
    nstages = len(model.layers) - (n - 1) * (g["banksJoinStage"] - g["banksSplitStage"]) if n > 1 else len(model.layers)
    nodes = []

    def node(module, name, inputs):
        d = dict(module=module, forwardNodeId=len(nodes) + 1, annotations={} if name is None else dict(name=name),
                 mapindex={i + 1: nodes[j - 1]["data"] for i, j in enumerate(inputs)})
        nodes.append(TorchObject("nngraph.Node", dict(data=d, id=len(nodes) + 1)))
        return len(nodes)

    hl = [node(TorchObject("nn.Identity", {}), "pModelInput", [])]
    pool_cls = "cudnn.%s%sPooling" % (kind, "Max" if g["poolType"] == "max" else "Average")
    for mi, (st, bank) in enumerate(conv_modules(nstages, g)):
        if bank == 0 and n > 1 and st == g["banksSplitStage"]:
            for i in range(1, n):
                if g["banksType"] == "mres":
                    hl.append(node(TorchObject("nn.%sAveragePooling" % kind, dict(kW=2, kH=2, dW=2, dH=2)),
                                   "Bank %d: downsample" % (i + 1), [hl[i - 1]]))
                else:
                    hl.append(hl[0])
        if bank == 0 and n > 1 and st == g["banksJoinStage"]:
            if g["banksType"] == "mres":
                for i in range(1, n):
                    up = TorchObject("nn.SpatialUpSamplingNearest" if not is3d else "tfluids.VolumetricUpSamplingNearest",
                                     dict(scale_factor=2 ** i))
                    hl[i] = node(up, "Bank %d: Upsample" % (i + 1), [hl[i]])
            concat = g["banksAggregateMethod"] == "concat"
            hl = [node(TorchObject("nn.JoinTable" if concat else "nn.CAddTable", {}),
                       "Concat Feats" if concat else "Add Feats", hl)]
        w, b = model.layers[mi]
        last = mi + 1 == len(model.layers)
        dil = 2 ** bank if (n > 1 and g["banksType"] == "dilate") else 1
        conv = _conv_module(w, b, is3d, model.up[mi], dil)
        if low_rank and mi == 0:
            conv = TorchObject("nn.Sequential", dict(modules={1: conv}))
        x = node(conv, "pPred" if last else "Bank %d: conv stage %d" % (bank + 1, st), [hl[bank]])
        if gated and mi == 0:
            gate = node(_conv_module(w, b, is3d), None, [hl[bank]])
            x = node(TorchObject("nn.CMulTable", {}), None, [x, gate])
        if not last:
            x = node(TorchObject("nn.ReLU", {}), "Bank %d: non-linearity" % (bank + 1), [x])
            if model.pool[mi] > 1:
                p = model.pool[mi]
                x = node(TorchObject(pool_cls, dict(kW=p, kH=p, dW=p, dH=p)), None, [x])
            if g["addBatchNorm"]:
                d = g["bn"][mi]
                f = dict(running_mean=np.asarray(d["running_mean"], np.float32), running_var=np.asarray(d["running_var"], np.float32),
                         eps=float(d["eps"]), momentum=0.1, affine=d.get("weight") is not None, train=bool(bn_train))
                if d.get("weight") is not None:
                    f.update(weight=np.asarray(d["weight"], np.float32), bias=np.asarray(d["bias"], np.float32))
                x = node(TorchObject("nn.%sBatchNormalization" % kind, f), None, [x])
            hl[bank] = x
    gm = TorchObject("nn.gModule", dict(forwardnodes={i + 1: nd for i, nd in enumerate(nodes)}, train=False))
    write(path, gm)
    write(path + "_mconf.bin", mconf)
