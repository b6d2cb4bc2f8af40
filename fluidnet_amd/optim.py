"""The optimiser step of the reference's training closure on the device (tfl_optim_*): the gradient clip of
torch/lib/run_epoch.lua:304-312, weight decay, torch/lib/adam.lua or torch/lib/rmsprop.lua, and the refresh of the native model
from the updated parameters -- one asynchronous call per step over a ProjectionNet's parameters and their .grad, capturable
(except on the 3-D default model's fp16 MFMA path: include/tfluids_hip.h tfl_model_set_weights_device). The moments and the
step counter live on the device. optim.sgd is Torch's own and not in the reference tree: torch.optim.SGD serves that.

A step captured into a graph and replayed changes the parameters and the native model without any Python running: the
ProjectionNet's guard against a backward whose forward saw older weights (its push count) does not see replays, and neither do
native models on other devices. Whoever replays a captured step orders forward, backward and step themselves, and calls
net.push_parameters() before using the net on another device.

    net = ProjectionNet(model).train()
    opt = fluidnet_amd.optim.from_mconf(net, mconf)        # or Adam(net, learningRate=..., gradNormThreshold=1)
    loss.backward(); opt.step(); opt.zero_grad()
"""
import ctypes

import torch

from . import _lib, tfluids
from ._lib import TfluidsError
from .train import ProjectionNet, _ptr_array

ADAM, RMSPROP = 0, 1
# the reference's own defaults (adam.lua:28-34, rmsprop.lua:28-32); gradNormThreshold <= 0: no clip
_DEFAULTS = {
    ADAM: dict(learningRate=0.001, learningRateDecay=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, weightDecay=0.0),
    RMSPROP: dict(learningRate=1e-2, alpha=0.99, epsilon=1e-8, weightDecay=0.0, initialMean=0.0),
}


class _Fused:
    method = None

    def __init__(self, net, gradNormThreshold=0.0, **config):
        if not isinstance(net, ProjectionNet):
            raise TfluidsError("fluidnet_amd.optim steps the parameters of a ProjectionNet")
        self.net = net
        self.config = dict(_DEFAULTS[self.method])
        self._opt = None
        self.set_config(gradNormThreshold=gradNormThreshold, **config)
        p = net.weights[0]
        self._lib, ctx = tfluids._context(p)
        self._dev = p.device
        h = net._handle(self._lib, ctx, p.device.index)
        self._opt = self._lib.tfl_optim_create(ctx, h, ctypes.byref(self._cconfig()))
        if not self._opt:
            raise TfluidsError(self._lib.tfl_last_error(ctx).decode())

    def _cconfig(self):
        c = dict(learningRate=0.0, learningRateDecay=0.0, beta1=0.0, beta2=0.0, epsilon=0.0, weightDecay=0.0, alpha=0.0,
                 initialMean=0.0, gradNormThreshold=0.0)
        c.update(self.config)
        return _lib.tfl_optim_config(self.method, *[float(c[k]) for k in (
            "learningRate", "learningRateDecay", "beta1", "beta2", "epsilon", "weightDecay", "alpha", "initialMean", "gradNormThreshold")])

    def set_config(self, **config):
        """new hyper-parameters from the next step on (the names of adam.lua / rmsprop.lua, and gradNormThreshold)"""
        known = set(_DEFAULTS[self.method]) | {"gradNormThreshold"}
        for k in config:
            if k not in known:
                raise TfluidsError("%s: unknown hyper-parameter %r (takes %s)" % (type(self).__name__, k, ", ".join(sorted(known))))
        self.config.update(config)
        if self._opt:
            lib, ctx = tfluids._context(self.net.weights[0])
            tfluids._call(lib, ctx, lib.tfl_optim_set_config(ctx, self._opt, ctypes.byref(self._cconfig())))

    def step(self, guard=None):
        """clip, decay, update and refresh the native model from the parameters' .grad, in place, on the current stream; the
        .grad tensors hold the clipped and decayed gradients afterwards. guard (tfl_optim_step_guarded): an int32 device tensor
        the update kernels read when they run; where its first word is non-zero the step changes nothing (parameters, moments,
        gradients and the counter stay; the refresh rebuilds the same weight forms)"""
        net = self.net
        params = list(net.weights) + list(net.biases)
        for p in params:
            if p.grad is None:
                raise TfluidsError("optim.step: a parameter has no .grad (run backward first)")
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous() or p.grad.device != p.device:
                raise TfluidsError("optim.step: parameters and gradients must be contiguous float32 tensors on one device")
        lib, ctx = tfluids._context(net.weights[0])
        if guard is not None and not (torch.is_tensor(guard) and guard.dtype == torch.int32 and guard.numel() >= 1 and
                                      guard.is_contiguous() and guard.device == self._dev):
            raise TfluidsError("optim.step: guard must be a contiguous int32 tensor on the parameters' device")
        tfluids._call(lib, ctx, lib.tfl_optim_step_guarded(
            ctx, self._opt, _ptr_array(list(net.weights)), _ptr_array(list(net.biases)),
            _ptr_array([p.grad for p in net.weights]), _ptr_array([p.grad for p in net.biases]),
            None if guard is None else ctypes.c_void_p(guard.data_ptr())))
        net._stepped_on_device()

    def zero_grad(self):
        """zero the gradients in place (the tensors stay where they are, so a captured step keeps finding them)"""
        for p in self.net.parameters():
            if p.grad is not None:
                p.grad.zero_()

    @property
    def steps(self):
        """the step counter t on the device (reads it back: synchronises; for logging)"""
        lib, ctx = tfluids._context(self.net.weights[0])
        return int(lib.tfl_optim_steps(ctx, self._opt))

    def state(self):
        """(m, v) as lists of tensors shaped like the parameters, weights then biases per layer interleaved as the native
        state holds them: [w0, b0, w1, b1, ...]; v is None for RMSprop. Copies (for checkpoints and tests)."""
        lib, ctx = tfluids._context(self.net.weights[0])
        n = int(lib.tfl_optim_get_state(ctx, self._opt, None, None))
        m = torch.empty(n, dtype=torch.float32, device=self._dev)
        v = torch.empty(n, dtype=torch.float32, device=self._dev) if self.method == ADAM else None
        got = lib.tfl_optim_get_state(ctx, self._opt, ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(v.data_ptr()) if v is not None else None)
        if got != n:
            raise TfluidsError("tfl_optim_get_state failed")
        shapes = [t.shape for wb in zip(self.net.weights, self.net.biases) for t in wb]

        def split(flat):
            out, o = [], 0
            for s in shapes:
                out.append(flat[o:o + s.numel()].view(s).clone())
                o += s.numel()
            return out
        return split(m), (split(v) if v is not None else None)

    def close(self):
        if self._opt:
            lib, ctx = tfluids._context(self.net.weights[0])
            lib.tfl_optim_destroy(ctx, self._opt)
            self._opt = None

    def __del__(self):
        try:
            if self._opt and not torch.cuda.is_current_stream_capturing():      # (the frees would invalidate a capture)
                self.close()
        except Exception:
            pass


class Adam(_Fused):
    """lib/adam.lua: learningRate, learningRateDecay, beta1, beta2, epsilon (outside the root), weightDecay; gradNormThreshold"""
    method = ADAM


class RMSprop(_Fused):
    """lib/rmsprop.lua: learningRate, alpha, epsilon, weightDecay, initialMean; gradNormThreshold"""
    method = RMSPROP


def from_mconf(net, mconf):
    """the optimiser mconf names (default_conf.lua:68-71, 107-119): optimizationMethod 'adam' | 'rmsprop', its optimState and
    gradNormThreshold; optimState entries the method does not read (momentum, dampening, nesterov, bestPerf) are left out"""
    method = mconf.get("optimizationMethod", "adam")
    cls = {"adam": Adam, "rmsprop": RMSprop}.get(method)
    if cls is None:
        raise TfluidsError("optimizationMethod %r is not built here (adam, rmsprop; torch.optim.SGD serves 'sgd')" % (method,))
    state = mconf.get("optimState", {})
    config = {k: state[k] for k in _DEFAULTS[cls.method] if k in state}
    return cls(net, gradNormThreshold=mconf.get("gradNormThreshold", 1), **config)
