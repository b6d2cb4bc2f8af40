"""The projection ConvNet as a torch.nn.Module whose parameters can be fitted: the two ends of the reference's training
closure (model:forward ... model:backward, torch/lib/run_epoch.lua:207-235, 269-293) over tfl_model_forward_train /
tfl_model_backward; fluidnet_amd.FluidCriterion is the middle. Parameter gradients only: the reference computes a gradInput
and run_epoch.lua throws it away, so gradients to pDiv, UDiv and flags are not built, and asking for one raises.
Optimisers are torch.optim's.
"""
import ctypes

import numpy as np
import torch

from . import tfluids
from ._lib import TfluidsError
from .model import FluidNetModel


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _ForwardTrain(torch.autograd.Function):
    """(p, U) = net(pDiv, UDiv, flags) on the exact fp32 kernels, keeping the tape; backward = the parameter gradients."""

    @staticmethod
    def forward(ctx, module, pDiv, UDiv, flags, *params):
        p, U, tape = module.forward_train(pDiv, UDiv, flags)
        ctx.module, ctx.flags, ctx.tape, ctx.pushes = module, flags, tape, module._pushes
        return p, U

    @staticmethod
    def backward(ctx, gradP, gradU):
        # the data gradient reads the native model's weights as they are NOW; the tape was taken with them as they were then
        if ctx.module._pushes != ctx.pushes:
            raise TfluidsError("ProjectionNet: the parameters were pushed to the native model between this forward and its "
                               "backward (an in-place update followed by another forward or push_parameters()): the gradient "
                               "would mix two sets of weights. Run backward before the parameters change")
        gw, gb = ctx.module.backward(ctx.flags, gradP, gradU, ctx.tape)
        return (None, None, None, None) + tuple(gw) + tuple(gb)


class ProjectionNet(torch.nn.Module):
    """A FluidNetModel with its weights and biases as nn.Parameters on the device (cudnn layout, one pair per layer).

    train(): forward(pDiv, UDiv, flags) -> (p, U) runs tfl_model_forward_train under autograd; .backward() of anything built on
    p and U (FluidCriterion's loss) accumulates the parameters' .grad. eval(): FluidNetModel.forward, the inference path.
    The native model holds its own re-laid-out copy of the weights: it is refreshed (tfl_model_set_weights) whenever a
    parameter's version counter has moved since the last push -- every optimiser step moves it -- or by push_parameters().
    Accepted wherever simulate() takes a model. Linear models without pooling / upsampling layers can be trained; the others
    run in eval mode only (training raises, naming the reason)."""

    def __init__(self, net, device="cuda"):
        super().__init__()
        if not isinstance(net, FluidNetModel):
            raise TfluidsError("ProjectionNet wraps a FluidNetModel")
        self.net = net
        dev = torch.device(device)
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(w.copy()).to(dev)) for w, _ in net.layers])
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(b.copy()).to(dev)) for _, b in net.layers])
        self._pushed = self._versions()      # the native model is created from net.layers = these values
        self._pushes = 0                     # times the native model's weights have changed (a backward checks its forward's count)
        self._bwd_work = None

    # -- the FluidNetModel surface simulate() and the z-slab step use ------------------------------------------------
    is3D = property(lambda self: self.net.is3D)
    layers = property(lambda self: self.net.layers)
    opts = property(lambda self: self.net.opts)
    _work = property(lambda self: self.net._work)
    _handles = property(lambda self: self.net._handles)

    def _handle(self, lib, ctx, dev):
        self._sync()
        return self.net._handle(lib, ctx, dev)

    def begin(self, *a, **k):
        self._sync()
        return self.net.begin(*a, **k)

    def finish(self, *a, **k):
        return self.net.finish(*a, **k)

    def range_errors(self, like):
        return self.net.range_errors(like)

    def range_flag(self, like):
        return self.net.range_flag(like)

    # -- parameters -> native model ----------------------------------------------------------------------------------
    def _versions(self):
        return tuple((p._version, p.device) for p in self.parameters())

    def _sync(self):
        if self._versions() != self._pushed:
            self.push_parameters()

    def push_parameters(self):
        """Copy the parameters into the native model (synchronous). Called by itself when a parameter's version has moved; call
        it after changing parameter storage behind autograd's back (p.data.copy_ does move the counter; a raw pointer write
        does not). A z-slab step graph recorded on this model must be re-recorded afterwards."""
        host = [(w.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy())
                for w, b in zip(self.weights, self.biases)]
        for (w, b), (w0, b0) in zip(host, self.net.layers):
            if w.shape != w0.shape or b.shape != b0.shape or w.dtype != np.float32:
                raise TfluidsError("parameter shapes / dtype no longer match the model's layers")
        self.net.layers = host                 # a handle created later (another device) starts from these
        dev = self.weights[0].device.index
        for d in [d for d in self.net._handles if d != dev]:      # re-created from net.layers on next use
            lib, ctx = tfluids._context(torch.empty(0, device="cuda:%d" % d))
            lib.tfl_model_destroy(ctx, self.net._handles.pop(d))
        h = self.net._handles.get(dev)
        if h is not None:
            lib, ctx = tfluids._context(self.weights[0])
            FP = ctypes.POINTER(ctypes.c_float)
            n = len(host)
            ws = (FP * n)(*[w.ctypes.data_as(FP) for w, _ in host])
            bs = (FP * n)(*[b.ctypes.data_as(FP) for _, b in host])
            tfluids._call(lib, ctx, lib.tfl_model_set_weights(ctx, h, ws, bs))
        self._pushed = self._versions()
        self._pushes += 1

    # -- forward -----------------------------------------------------------------------------------------------------
    def forward(self, pDiv, UDiv=None, flags=None, **kw):
        """forward(pDiv, UDiv, flags) -> (p, U). Also forward([pDiv, UDiv, flags], out=..., UBC=..., ...) -> [p, U]: the call
        shape of FluidNetModel.forward that simulate() uses (inference path, whatever the mode)."""
        if UDiv is None:
            self._sync()
            return self.net.forward(pDiv, **kw)
        for name, t in (("pDiv", pDiv), ("UDiv", UDiv), ("flags", flags)):
            if t.requires_grad:
                raise TfluidsError("ProjectionNet: %s requires grad, but input gradients are not built (parameter gradients "
                                   "only): detach it" % name)
        if not (self.training and torch.is_grad_enabled()):
            self._sync()
            p, U = self.net.forward([pDiv, UDiv, flags])
            return p, U
        return _ForwardTrain.apply(self, pDiv, UDiv, flags, *self.weights, *self.biases)

    def forward_train(self, pDiv, UDiv, flags):
        """(p, U, tape) = tfl_model_forward_train: the forward on the shape-generic fp32 kernels and what backward() reads."""
        self._sync()
        tfluids._dims(UDiv, flags)
        tfluids._check(pDiv.shape == flags.shape and pDiv.is_contiguous(), "Size mismatch")
        tfluids._check((UDiv.size(1) == 3) == self.net.is3D, "model / input dimensionality mismatch")
        lib, ctx, h, work = self.net._prep(flags)
        B, _, Z, Y, X = flags.shape
        n = lib.tfl_model_tape_floats(h, B, Z, Y, X)
        # (a model without a training pass: the call below says which kind it is)
        tape = torch.empty(max(int(n), 2), dtype=torch.float64, device=flags.device).view(torch.float32)[:max(int(n), 0)]
        p, U = torch.empty_like(pDiv), torch.empty_like(UDiv)
        from .simulate import wall_plan
        wall_plan(lib, ctx, flags)
        tfluids._call(lib, ctx, lib.tfl_model_forward_train(
            ctx, h, tfluids._tt(pDiv), tfluids._tt(UDiv), tfluids._tt(flags), tfluids._tt(p), tfluids._tt(U),
            ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(tape.data_ptr()), tape.numel()))
        return p, U, tape

    def backward(self, flags, gradP, gradU, tape, out=None, accumulate=False):
        """tfl_model_backward: ([gradWeight], [gradBias]) in the parameters' layout from gradP / gradU (None = zero) at the
        model's outputs. out=(gw, gb): write into (accumulate: add onto) these tensors instead of fresh ones."""
        lib, ctx, h, _ = self.net._prep(flags)
        B, _, Z, Y, X = flags.shape
        need = lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X)
        if self._bwd_work is None or self._bwd_work.numel() < need or self._bwd_work.device != flags.device:
            self._bwd_work = torch.empty(max(int(need), 2), dtype=torch.float64, device=flags.device).view(torch.float32)
        if out is None:
            gw, gb = [torch.empty_like(w) for w in self.weights], [torch.empty_like(b) for b in self.biases]
            tfluids._check(not accumulate, "accumulate needs out=(gradWeights, gradBiases)")
        else:
            gw, gb = out
        gP = None if gradP is None else gradP.contiguous()
        gU = None if gradU is None else gradU.contiguous()
        tfluids._call(lib, ctx, lib.tfl_model_backward(
            ctx, h, tfluids._tt(flags), None if gP is None else tfluids._tt(gP), None if gU is None else tfluids._tt(gU),
            ctypes.c_void_p(tape.data_ptr()), tape.numel(), ctypes.c_void_p(self._bwd_work.data_ptr()), self._bwd_work.numel(),
            _ptr_array(gw), _ptr_array(gb), int(bool(accumulate))))
        return gw, gb
