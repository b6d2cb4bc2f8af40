"""Minimal reader for torch7 binary serialisation (enough for FluidNet model files such as
data/models/myModel2D and *_mconf.bin). Host-side plumbing on the "data formats either side of the
path" (SURVEY.md 8f-3); format notes in SURVEY.md Appendix A.

Little-endian stream of typed objects: 0 nil, 1 number(f64), 2 string, 3 table, 4 torch object,
5 boolean, 6/7/8 function. Tables and torch objects are memoised by an int32 index.
"""
import struct

import numpy as np

_STORAGE_DTYPES = {
    "torch.FloatStorage": np.float32, "torch.CudaStorage": np.float32,
    "torch.DoubleStorage": np.float64, "torch.CudaDoubleStorage": np.float64,
    "torch.LongStorage": np.int64, "torch.CudaLongStorage": np.int64,
    "torch.IntStorage": np.int32, "torch.ByteStorage": np.uint8, "torch.CharStorage": np.int8,
    "torch.ShortStorage": np.int16, "torch.HalfStorage": np.float16,
    "torch.CudaHalfStorage": np.float16,
}


class _ObjKey:
    """Hashable wrapper for table-valued table keys."""

    def __init__(self, obj):
        self.obj = obj


class TorchObject:
    """A non-tensor torch class instance (nn.*, cudnn.*, nngraph.Node, tfluids.*): its field table."""

    def __init__(self, typename, fields):
        self.typename = typename
        self.fields = fields

    def __getitem__(self, k):
        return self.fields[k]

    def get(self, k, default=None):
        return self.fields.get(k, default) if isinstance(self.fields, dict) else default

    def __repr__(self):
        return "TorchObject(%s)" % self.typename


class _Reader:
    def __init__(self, data):
        self.b = data
        self.o = 0
        self.memo = {}

    def _unpack(self, fmt, n):
        v = struct.unpack_from(fmt, self.b, self.o)
        self.o += n
        return v[0]

    def i32(self):
        return self._unpack("<i", 4)

    def i64(self):
        return self._unpack("<q", 8)

    def f64(self):
        return self._unpack("<d", 8)

    def string(self):
        n = self.i32()
        s = self.b[self.o:self.o + n]
        self.o += n
        return s.decode("latin-1")

    def obj(self):
        t = self.i32()
        if t == 0:
            return None
        if t == 1:
            v = self.f64()
            return int(v) if (v == v and abs(v) < 2 ** 53 and v == int(v)) else v
        if t == 2:
            return self.string()
        if t == 5:
            return self.i32() == 1
        if t == 3:
            idx = self.i32()
            if idx in self.memo:
                return self.memo[idx]
            out = {}
            self.memo[idx] = out
            n = self.i32()
            for _ in range(n):
                k = self.obj()
                if isinstance(k, (dict, list, np.ndarray)):  # nngraph keys tables by node
                    k = _ObjKey(k)
                out[k] = self.obj()
            return out
        if t == 4:
            idx = self.i32()
            if idx in self.memo:
                return self.memo[idx]
            version = self.string()
            cls = self.string() if version.startswith("V ") else version
            if cls.endswith("Tensor"):
                nd = self.i32()
                size = [self.i64() for _ in range(nd)]
                stride = [self.i64() for _ in range(nd)]
                off = self.i64() - 1
                holder = [None]
                self.memo[idx] = holder  # placeholder (tensors are never self-referential)
                storage = self.obj()
                if storage is None or nd == 0:
                    arr = np.zeros(size, np.float32)
                else:
                    arr = np.lib.stride_tricks.as_strided(
                        storage[off:], shape=size,
                        strides=[s * storage.itemsize for s in stride]).copy()
                self.memo[idx] = arr
                return arr
            if cls.endswith("Storage"):
                n = self.i64()
                dt = np.dtype(_STORAGE_DTYPES[cls])
                arr = np.frombuffer(self.b, dt, n, self.o).copy()
                self.o += n * dt.itemsize
                self.memo[idx] = arr
                return arr
            ob = TorchObject(cls, None)
            self.memo[idx] = ob
            ob.fields = self.obj()
            return ob
        if t in (6, 7, 8):  # functions: (index, bytecode, upvalues) -- skipped
            idx = self.i32()
            if idx in self.memo:
                return self.memo[idx]
            n = self.i32()
            self.o += n
            self.memo[idx] = "<function>"
            self.obj()
            return "<function>"
        raise ValueError("unknown torch7 type tag %d at offset %d" % (t, self.o))


def load(path):
    import sys
    with open(path, "rb") as f:
        data = f.read()
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 20000))  # nngraph models nest deeply
    try:
        return _Reader(data).obj()
    finally:
        sys.setrecursionlimit(old)


def conv_layers(model):
    """Walk an nn.gModule (lib/model.lua) in forward order and return its convolution layers as
    [(weight[nOut, nIn, k...], bias[nOut])] -- `Bank 1: conv stage N` nodes, then the output conv."""
    nodes = model["forwardnodes"]
    out = []
    for i in sorted(nodes):
        data = nodes[i]["data"]
        mod = data.get("module") if isinstance(data, dict) else None
        if isinstance(mod, TorchObject) and "Convolution" in mod.typename:
            w = np.asarray(mod["weight"], np.float32)
            b = np.asarray(mod["bias"], np.float32)
            nout, nin = int(mod["nOutputPlane"]), int(mod["nInputPlane"])
            if "Volumetric" in mod.typename:
                w = w.reshape(nout, nin, int(mod["kT"]), int(mod["kH"]), int(mod["kW"]))
            else:
                w = w.reshape(nout, nin, int(mod["kH"]), int(mod["kW"]))
            out.append((w, b))
    return out


class GraphError(ValueError):
    """A node of the gModule that the library does not build (raised with the node's name)."""


def _nodes(model):
    """forwardNodeId -> (module, annotation name, [input ids in mapindex order]) of an nn.gModule's forward graph."""
    out = {}
    for nd in model["forwardnodes"].values():
        d = nd["data"]
        if not isinstance(d, dict):
            continue
        ann = d.get("annotations")
        name = ann.get("name") if isinstance(ann, dict) else None
        mi = d.get("mapindex") or {}
        ins = [mi[k]["forwardNodeId"] for k in sorted(k for k in mi if isinstance(k, int)) if isinstance(mi[k], dict)]
        out[d["forwardNodeId"]] = (d.get("module"), name, ins)
    return out


def _conv_arrays(mod):
    """(weight [nOut(*up^dim), nIn, k..], bias, up, dilation) of a convolution module."""
    tn = mod.typename
    up, dil = 1, 1
    if tn.endswith("ConvolutionUpsample"):       # lib/modules/*_convolution_upsample.lua: the inner conv is modules[1]
        up = int(mod["scaleW"])
        if int(mod["scaleH"]) != up or int(mod.get("scaleT", up)) != up:
            raise GraphError("%s with unequal scales" % tn)
        inner = mod["modules"][1]
        return _conv_arrays(inner)[:2] + (up, 1)
    if "Dilated" in tn:
        dil = int(mod["dilationW"])
        if int(mod["dilationH"]) != dil or int(mod.get("dilationT", dil)) != dil:
            raise GraphError("%s with unequal dilations" % tn)
    w = np.asarray(mod["weight"], np.float32)
    b = np.asarray(mod["bias"], np.float32)
    nout, nin = int(mod["nOutputPlane"]), int(mod["nInputPlane"])
    if "Volumetric" in tn:
        w = w.reshape(nout, nin, int(mod["kT"]), int(mod["kH"]), int(mod["kW"]))
    else:
        w = w.reshape(nout, nin, int(mod["kH"]), int(mod["kW"]))
    if len(set(w.shape[2:])) != 1:
        raise GraphError("%s with a non-cubic kernel" % tn)
    return w, b, up, dil


def _is_conv(mod):
    return isinstance(mod, TorchObject) and "Convolution" in mod.typename


def model_graph(model, mconf):
    """Walk an nn.gModule built by lib/model.lua:defineModelGraph (with its `_mconf.bin` table) by the nodes' annotations
    (`Bank i: conv stage N`, `Bank i: downsample`, `Bank i: Upsample`, `Concat Feats` / `Add Feats`) and their inputs
    (mapindex). Returns dict(layers, pool, up, dilation, bn, poolType, stages) with the conv modules in the reference's
    creation order. Refuses, by name, what the library does not build: gated (CMulTable) and low-rank (Sequential of
    convolutions) convolutions, a batch norm in training mode, weight sharing."""
    nodes = _nodes(model)
    users = {}
    for nid, (_, _, ins) in nodes.items():
        for i in ins:
            users.setdefault(i, []).append(nid)
    if mconf.get("banksWeightShare"):
        raise GraphError("banksWeightShare: weight sharing is not supported (model.lua:326-328)")
    for nid, (mod, name, _) in nodes.items():
        tn = getattr(mod, "typename", "")
        if tn == "nn.CMulTable":
            raise GraphError("node %r: gated convolutions (CMulTable) are not supported" % (name or nid,))
        if tn == "nn.Sequential" and any(_is_conv(m) for m in (mod.get("modules") or {}).values()):
            raise GraphError("node %r: low-rank convolutions (Sequential of convolutions) are not supported" % (name or nid,))
    convs = []        # (stage, bank, node id)
    last = None
    for nid, (mod, name, _) in nodes.items():
        if not _is_conv(mod):
            continue
        if name and name.startswith("Bank ") and ": conv stage " in name:
            bank, stage = name[len("Bank "):].split(": conv stage ")
            convs.append((int(stage), int(bank) - 1, nid))
        elif last is None:
            last = nid
        else:
            raise GraphError("node %r: a convolution outside the layer stages" % (name or nid,))
    if last is None or not convs:
        raise GraphError("no convolution stages found")
    convs.sort()
    nstages = convs[-1][0] + 1
    convs.append((nstages, 0, last))
    out = dict(layers=[], pool=[], up=[], dilation=[], bn=[], poolType="avg", stages=nstages)
    pool_types = set()
    for st, bank, nid in convs:
        w, b, up, dil = _conv_arrays(nodes[nid][0])
        out["layers"].append((w, b))
        out["up"].append(up)
        out["dilation"].append(dil)
        # conv -> non-linearity -> [pooling] -> [batch norm]: follow the single consumer chain
        pool, bn, cur = 1, None, nid
        if nid != last:
            chain = []
            while len(users.get(cur, [])) == 1:
                cur = users[cur][0]
                m = nodes[cur][0]
                tn = getattr(m, "typename", "")
                if _is_conv(m) or "Table" in tn or "UpSampling" in tn or tn.endswith("Unsqueeze") or m is None:
                    break
                chain.append((cur, m, tn))
            for cid, m, tn in chain:
                if "MaxPooling" in tn or "AveragePooling" in tn:
                    if nodes[cid][1] and "downsample" in nodes[cid][1]:
                        break                      # the next bank's pyramid level, not this stage's pooling
                    pool = int(m["kW"])
                    pool_types.add("max" if "MaxPooling" in tn else "avg")
                elif "BatchNormalization" in tn:
                    if m.get("train"):
                        raise GraphError("node %r: batch norm in training mode (call model:evaluate() before saving)" % (nodes[cid][1] or cid,))
                    wgt, bia = m.get("weight"), m.get("bias")
                    bn = dict(running_mean=np.asarray(m["running_mean"], np.float32),
                              running_var=np.asarray(m["running_var"], np.float32),
                              weight=None if wgt is None or isinstance(wgt, str) else np.asarray(wgt, np.float32),
                              bias=None if bia is None or isinstance(bia, str) else np.asarray(bia, np.float32),
                              eps=float(m["eps"]))
        out["pool"].append(pool)
        if nid != last:
            out["bn"].append(bn)
    if len(pool_types) > 1:
        raise GraphError("both average and max pooling layers")
    if pool_types:
        out["poolType"] = pool_types.pop()
    return out


# node types the flat conv walk (conv_layers) would drop or misread
_GRAPH_NODE_HINTS = ("BatchNormalization", "Dilated", "Pooling", "UpSampling", "ConvolutionUpsample", "CAddTable",
                     "CMulTable")


def needs_graph(model):
    """True when the gModule holds nodes conv_layers() would drop or misread: batch norm, dilated convolutions, pooling,
    upsampling, bank joins, gates, or more than one bank."""
    for mod, name, _ in _nodes(model).values():
        tn = getattr(mod, "typename", "")
        if any(h in tn for h in _GRAPH_NODE_HINTS) or (name or "").startswith(("Bank 2", "Concat Feats", "Add Feats")):
            return True
    return False
