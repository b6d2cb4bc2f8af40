"""The projection ConvNet as a torch.nn.Module whose parameters can be fitted: the two ends of the reference's training
closure (model:forward ... model:backward, torch/lib/run_epoch.lua:207-235, 269-293) over tfl_model_forward_train /
tfl_model_backward; fluidnet_amd.FluidCriterion is the middle. By default parameter gradients only: the reference computes a
gradInput and run_epoch.lua throws it away, and asking for a gradient to pDiv, UDiv or flags raises. ProjectionNet(net,
input_grad=True) also builds the gradients to pDiv and UDiv (tfl_model_backward_input), so that the net can be chained or put
behind differentiable torch code; there is no gradient to flags.
Optimisers: torch.optim's, or the fused device step of fluidnet_amd.optim (clip + Adam / RMSprop + refresh in one call).
"""
import ctypes

import torch

from . import tfluids
from ._lib import TfluidsError
from .model import FluidNetModel


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _ForwardTrain(torch.autograd.Function):
    """(p, U) = net(pDiv, UDiv, flags) on the exact fp32 kernels, keeping the tape; backward = the parameter gradients and,
    for a module built with input_grad=True, the gradients to pDiv and UDiv where autograd asks for them."""

    @staticmethod
    def forward(ctx, module, pDiv, UDiv, flags, *params):
        p, U, tape = module.forward_train(pDiv, UDiv, flags)
        ctx.module, ctx.flags, ctx.tape, ctx.pushes = module, flags, tape, module._pushes
        if module.input_grad:
            # (through autograd's own store: an in-place edit of an input or of U before backward trips its version check)
            ctx.save_for_backward(pDiv, UDiv, U)
        return p, U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gradP, gradU):
        # the data gradient reads the native model's weights as they are NOW; the tape was taken with them as they were then
        if ctx.module._pushes != ctx.pushes:
            raise TfluidsError("ProjectionNet: the parameters were pushed to the native model between this forward and its "
                               "backward (an in-place update followed by another forward or push_parameters()): the gradient "
                               "would mix two sets of weights. Run backward before the parameters change")
        if not ctx.module.input_grad:
            gw, gb = ctx.module.backward(ctx.flags, gradP, gradU, ctx.tape)
            return (None, None, None, None) + tuple(gw) + tuple(gb)
        pDiv, UDiv, U = ctx.saved_tensors
        gw, gb, gp, gu = ctx.module.backward_input(ctx.flags, pDiv, UDiv, U, gradP, gradU, ctx.tape,
                                                   want=(ctx.needs_input_grad[1], ctx.needs_input_grad[2]))
        return (None, gp, gu, None) + tuple(gw) + tuple(gb)


class ProjectionNet(torch.nn.Module):
    """A FluidNetModel with its weights and biases as nn.Parameters on the device (cudnn layout, one pair per layer).

    train(): forward(pDiv, UDiv, flags) -> (p, U) runs tfl_model_forward_train under autograd; .backward() of anything built on
    p and U (FluidCriterion's loss) accumulates the parameters' .grad. eval(): FluidNetModel.forward, the inference path.
    The native model holds its own re-laid-out copy of the weights: it is refreshed on the device, from the parameters where
    they lie (tfl_model_set_weights_device: no host copy, no synchronisation), whenever a parameter's version counter has moved
    since the last push -- every torch.optim step moves it -- or by push_parameters(). The host copy `layers` follows lazily:
    when something reads it, or when a handle is created on a device that has none.
    Accepted wherever simulate() takes a model. Linear models without pooling / upsampling layers can be trained, and so can
    banked models ('mres' / 'dilate' banks, 'concat' / 'add' joins) without batch norm and without pooling / upsampling stages; the
    others run in eval mode only (training raises, naming the reason) -- unless they are linear and the module is created with
    multires=True (below).
    multires=True: a linear model with 2x average pooling / ConvolutionUpsample layers (`tog`, custom layer tables) gets its
    training pass when its native model is created (tfl_model_enable_multires_training). Nothing changes for a model that can be
    trained anyway; a model the call does not take (banked `tog`, max pooling, batch norm) raises the library's refusal.
    input_grad=True: pDiv and UDiv may require grad, and backward returns their gradients (tfl_model_backward_input) -- two
    passes can be chained, net(*net(pDiv, UDiv, flags), flags), or torch code put in front. flags never gets a gradient."""

    def __init__(self, net, device="cuda", input_grad=False, multires=False):
        super().__init__()
        self.input_grad = bool(input_grad)
        self.multires = bool(multires)
        if not isinstance(net, FluidNetModel):
            raise TfluidsError("ProjectionNet wraps a FluidNetModel")
        self.net = net
        if self.multires:
            if net._handles and not getattr(net, "_multires_training", False):
                raise TfluidsError("ProjectionNet(multires=True): this FluidNetModel has a native model already; wrap a fresh one")
            net._multires_training = True
        dev = torch.device(device)
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(w.copy()).to(dev)) for w, _ in net.layers])
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(b.copy()).to(dev)) for _, b in net.layers])
        self._pushed = self._versions()      # the native model is created from net.layers = these values
        self._pushes = 0                     # times the native model's weights have changed (a backward checks its forward's count)
        self._host_stale = False             # net.layers is older than the parameters (brought up to date by _host_sync)
        self._bwd_work = None

    # -- the FluidNetModel surface simulate() and the z-slab step use ------------------------------------------------
    is3D = property(lambda self: self.net.is3D)

    @property
    def layers(self):
        self._host_sync()
        return self.net.layers

    opts = property(lambda self: self.net.opts)
    _work = property(lambda self: self.net._work)
    _handles = property(lambda self: self.net._handles)

    def _handle(self, lib, ctx, dev):
        self._sync(dev)
        return self.net._handle(lib, ctx, dev)

    def begin(self, U, *a, **k):
        self._sync(U.device.index)
        return self.net.begin(U, *a, **k)

    def finish(self, *a, **k):
        return self.net.finish(*a, **k)

    def range_errors(self, like):
        return self.net.range_errors(like)

    def range_flag(self, like):
        return self.net.range_flag(like)

    # -- parameters -> native model ----------------------------------------------------------------------------------
    def _versions(self):
        return tuple((p._version, p.device) for p in self.parameters())

    def _sync(self, dev=None):
        """the native model up to date with the parameters; dev: the device the caller is about to run on -- a handle created
        there starts from the host copy, so that is brought up to date first"""
        if self._versions() != self._pushed:
            self._push_device()
        if dev is not None and dev not in self.net._handles:
            self._host_sync()

    def _param_arrays(self):
        for p, (w0, b0) in zip(self.weights, self.net.layers):
            if tuple(p.shape) != w0.shape or p.dtype != torch.float32 or not p.is_contiguous():
                raise TfluidsError("parameter shapes / dtype no longer match the model's layers")
        for p, (w0, b0) in zip(self.biases, self.net.layers):
            if tuple(p.shape) != b0.shape or p.dtype != torch.float32 or not p.is_contiguous():
                raise TfluidsError("parameter shapes / dtype no longer match the model's layers")
        return _ptr_array(list(self.weights)), _ptr_array(list(self.biases))

    def _drop_other_handles(self, dev):
        """the native models on devices other than the parameters' own hold the old weights: destroyed here, re-created from
        the host copy (brought up to date first: _sync) on next use"""
        for d in [d for d in self.net._handles if d != dev]:
            lib, ctx = tfluids._context(torch.empty(0, device="cuda:%d" % d))
            lib.tfl_model_destroy(ctx, self.net._handles.pop(d))

    def _push_device(self):
        """tfl_model_set_weights_device on the current stream: every weight form of the native model rebuilt from the
        parameters where they lie. (The 3-D default model on its fp16 MFMA path ends with a 12-byte read-back: see the header.)"""
        ws, bs = self._param_arrays()
        dev = self.weights[0].device.index
        self._host_stale = True
        self._drop_other_handles(dev)
        h = self.net._handles.get(dev)
        if h is not None:
            lib, ctx = tfluids._context(self.weights[0])
            tfluids._call(lib, ctx, lib.tfl_model_set_weights_device(ctx, h, ws, bs))
        self._pushed = self._versions()
        self._pushes += 1

    def _host_sync(self):
        """net.layers = the parameters' values (a device-to-host copy: synchronises), if they have changed since it was taken"""
        if not self._host_stale:
            return
        self.net.layers = [(w.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy())
                           for w, b in zip(self.weights, self.biases)]
        self._host_stale = False

    def _stepped_on_device(self):
        """fluidnet_amd.optim: a fused step has rewritten the parameters behind autograd's version counters and refreshed the
        native model on the parameters' device from them itself: no second push is due there, but a backward whose forward saw the
        old weights is refused, and a native model on any other device is dropped as after a push. (A captured step REPLAYED by
        its graph does not come through here: see fluidnet_amd.optim.)"""
        self._drop_other_handles(self.weights[0].device.index)
        self._pushed = self._versions()
        self._pushes += 1
        self._host_stale = True

    def push_parameters(self):
        """Copy the parameters into the native model and into the host copy, and wait for it (synchronous). Call it after
        changing parameter storage behind autograd's back (p.data.copy_ does move the counter, and the next forward pushes by
        itself; a raw pointer write does not). A z-slab step graph recorded on this model must be re-recorded afterwards."""
        self._push_device()
        self._host_sync()
        torch.cuda.current_stream(self.weights[0].device).synchronize()

    # -- forward -----------------------------------------------------------------------------------------------------
    def forward(self, pDiv, UDiv=None, flags=None, **kw):
        """forward(pDiv, UDiv, flags) -> (p, U). Also forward([pDiv, UDiv, flags], out=..., UBC=..., ...) -> [p, U]: the call
        shape of FluidNetModel.forward that simulate() uses (inference path, whatever the mode)."""
        if UDiv is None:
            self._sync(pDiv[0].device.index)
            return self.net.forward(pDiv, **kw)
        for name, t in (("pDiv", pDiv), ("UDiv", UDiv), ("flags", flags)):
            if t.requires_grad and not (self.input_grad and name != "flags"):
                raise TfluidsError("ProjectionNet: %s requires grad, but input gradients are not built (parameter gradients "
                                   "only) unless the module is created with input_grad=True, and never for flags: detach it" % name)
        if not (self.training and torch.is_grad_enabled()):
            self._sync(pDiv.device.index)
            p, U = self.net.forward([pDiv, UDiv, flags])
            return p, U
        return _ForwardTrain.apply(self, pDiv, UDiv, flags, *self.weights, *self.biases)

    def forward_train(self, pDiv, UDiv, flags):
        """(p, U, tape) = tfl_model_forward_train: the forward on the shape-generic fp32 kernels and what backward() reads."""
        self._sync(flags.device.index)
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

    def _bwd_scratch(self, need, device):
        if self._bwd_work is None or self._bwd_work.numel() < need or self._bwd_work.device != device:
            self._bwd_work = torch.empty(max(int(need), 2), dtype=torch.float64, device=device).view(torch.float32)
        return self._bwd_work

    def backward_input(self, flags, pDiv, UDiv, U, gradP, gradU, tape, out=None, accumulate=False, want=(True, True), params=True):
        """tfl_model_backward_input: ([gradWeight], [gradBias], gradPDiv, gradUDiv) from gradP / gradU (None = zero) at the
        model's outputs; pDiv, UDiv: what forward_train was given, U: what it returned. want: which of the two input gradients to
        build (the other is None). params=False: the input gradients only (the two lists are None). out / accumulate: as backward()."""
        lib, ctx, h, _ = self.net._prep(flags)
        B, _, Z, Y, X = flags.shape
        work = self._bwd_scratch(lib.tfl_model_backward_input_workspace_floats(h, B, Z, Y, X), flags.device)
        if not params:
            gw = gb = None
            tfluids._check(out is None and not accumulate, "params=False builds no parameter gradients")
        elif out is None:
            gw, gb = [torch.empty_like(w) for w in self.weights], [torch.empty_like(b) for b in self.biases]
            tfluids._check(not accumulate, "accumulate needs out=(gradWeights, gradBiases)")
        else:
            gw, gb = out
        gP = None if gradP is None else gradP.contiguous()
        gU = None if gradU is None else gradU.contiguous()
        pDiv, UDiv, U = pDiv.contiguous(), UDiv.contiguous(), U.contiguous()
        gp = torch.empty_like(pDiv) if want[0] else None
        gu = torch.empty_like(UDiv) if want[1] else None
        tt = lambda t: None if t is None else tfluids._tt(t)
        tfluids._call(lib, ctx, lib.tfl_model_backward_input(
            ctx, h, tfluids._tt(flags), tfluids._tt(pDiv), tfluids._tt(UDiv), tfluids._tt(U), tt(gP), tt(gU),
            ctypes.c_void_p(tape.data_ptr()), tape.numel(), ctypes.c_void_p(work.data_ptr()), work.numel(),
            None if gw is None else _ptr_array(gw), None if gb is None else _ptr_array(gb), int(bool(accumulate)), tt(gp), tt(gu)))
        return gw, gb, gp, gu

    def backward(self, flags, gradP, gradU, tape, out=None, accumulate=False):
        """tfl_model_backward: ([gradWeight], [gradBias]) in the parameters' layout from gradP / gradU (None = zero) at the
        model's outputs. out=(gw, gb): write into (accumulate: add onto) these tensors instead of fresh ones."""
        lib, ctx, h, _ = self.net._prep(flags)
        B, _, Z, Y, X = flags.shape
        self._bwd_scratch(lib.tfl_model_backward_workspace_floats(h, B, Z, Y, X), flags.device)
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
