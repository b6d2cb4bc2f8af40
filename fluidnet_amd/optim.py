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

Data parallel (tfl_optim_step_reduced): N ranks, each with its own net, optimiser and mini-batch, and a transport of
fluidnet_amd.dist between them. opt.step(guard, comm) averages the gradients over the ranks inside the step -- one all-reduce of
P + 1 doubles, g = float(sum of the ranks' g in fp64 / N) -- so that every rank takes the step of the N-fold batch and all end
with the same bits; opt.sync_parameters(comm) first gives every rank rank 0's parameters. A guard set on one rank holds the
step back on all of them (opt.reduced_guard()).
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


def comm_world(comm):
    """the number of ranks behind a transport of fluidnet_amd.dist (ThreadComm keeps it on its hub)"""
    world = getattr(comm, "world", None)
    if world is None and getattr(comm, "hub", None) is not None:
        world = comm.hub.world
    if world is None or int(world) < 1:
        raise TfluidsError("optim: the transport does not say how many ranks it joins (comm.world)")
    return int(world)


class _Fused:
    method = None

    def __init__(self, net, gradNormThreshold=0.0, **config):
        if not isinstance(net, ProjectionNet):
            raise TfluidsError("fluidnet_amd.optim steps the parameters of a ProjectionNet")
        self.net = net
        self.config = dict(_DEFAULTS[self.method])
        self._opt = None
        self._reduce = None      # the fp64 reduce buffer of the data-parallel step, as the float tensor a transport binds
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

    def _reduce_for(self, comm):
        """(pointer, doubles) of the reduce buffer, with comm bound to it: dist._CommBase resolves the pointers its callbacks
        receive inside the tensor it is bound to"""
        if not hasattr(comm, "struct"):
            raise TfluidsError("optim: comm must be a transport of fluidnet_amd.dist (DistComm, RcclComm, ThreadComm)")
        lib, ctx = tfluids._context(self.net.weights[0])
        if self._reduce is None:
            n = int(lib.tfl_optim_reduce_doubles(ctx, self._opt))
            if n < 1:
                raise TfluidsError("tfl_optim_reduce_doubles failed")
            self._reduce = torch.zeros(2 * n, dtype=torch.float32, device=self._dev)
        comm.bind(self._reduce)
        comm.error = None
        return ctypes.c_void_p(self._reduce.data_ptr()), self._reduce.numel() // 2

    @staticmethod
    def _comm_call(lib, ctx, comm, rc):
        if rc != 0:
            if comm.error is not None:
                raise comm.error
            raise TfluidsError(lib.tfl_last_error(ctx).decode())

    def step(self, guard=None, comm=None):
        """clip, decay, update and refresh the native model from the parameters' .grad, in place, on the current stream; the
        .grad tensors hold the clipped and decayed gradients afterwards. guard (tfl_optim_step_guarded): an int32 device tensor
        the update kernels read when they run; where its first word is non-zero the step changes nothing (parameters, moments,
        gradients and the counter stay; the refresh rebuilds the same weight forms).
        comm (tfl_optim_step_reduced): a DistComm, RcclComm or ThreadComm; every rank of its world calls step() together. The
        gradients are summed over the ranks in fp64 by ONE all-reduce and divided by the world size, rounded once; the guards
        travel with them, and a guard set on any rank holds every rank's step back (reduced_guard()). The .grad tensors hold the
        averaged (clipped, decayed) gradients afterwards -- under a set reduced guard, the local ones still."""
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
        args = (ctx, self._opt, _ptr_array(list(net.weights)), _ptr_array(list(net.biases)),
                _ptr_array([p.grad for p in net.weights]), _ptr_array([p.grad for p in net.biases]),
                None if guard is None else ctypes.c_void_p(guard.data_ptr()))
        if comm is None:
            tfluids._call(lib, ctx, lib.tfl_optim_step_guarded(*args))
        else:
            buf, n = self._reduce_for(comm)
            self._comm_call(lib, ctx, comm, lib.tfl_optim_step_reduced(*args, ctypes.byref(comm.struct), comm_world(comm), buf, n))
        net._stepped_on_device()

    def reduced_guard(self, out=None):
        """the guard word the last step(comm=...) acted on -- non-zero: some rank's guard was set and no rank stepped -- as an
        int32 device tensor [1] (out: written in place). A copy enqueued on the current stream; nothing waits."""
        if out is None:
            out = torch.empty(1, dtype=torch.int32, device=self._dev)
        if not (torch.is_tensor(out) and out.dtype == torch.int32 and out.numel() >= 1 and out.is_contiguous() and out.device == self._dev):
            raise TfluidsError("optim.reduced_guard: out must be a contiguous int32 tensor on the parameters' device")
        lib, ctx = tfluids._context(self.net.weights[0])
        tfluids._call(lib, ctx, lib.tfl_optim_reduced_guard(ctx, self._opt, ctypes.c_void_p(out.data_ptr())))
        return out

    def sync_parameters(self, comm):
        """rank 0's parameters into the parameters of every rank of comm's world, bit for bit (tfl_optim_sync_parameters: one
        all-reduce), and the native model refreshed from them. Collective. The moments and the step counter stay."""
        net = self.net
        for p in net.parameters():
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise TfluidsError("optim.sync_parameters: parameters must be contiguous float32 tensors")
        lib, ctx = tfluids._context(net.weights[0])
        buf, n = self._reduce_for(comm)
        self._comm_call(lib, ctx, comm, lib.tfl_optim_sync_parameters(
            ctx, self._opt, _ptr_array(list(net.weights)), _ptr_array(list(net.biases)), ctypes.byref(comm.struct), int(comm.rank), buf, n))
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

    def load_state(self, m, v, steps):
        """the inverse of state() and .steps (tfl_optim_set_state), for resuming from a checkpoint: m, v as state() returns them
        (lists of tensors or arrays in its order, or one flat tensor each; v is ignored for RMSprop), and the step counter.
        Enqueued on the current stream; nothing waits."""
        lib, ctx = tfluids._context(self.net.weights[0])
        n = int(lib.tfl_optim_get_state(ctx, self._opt, None, None))

        def flat(x, name):
            if x is None:
                return None
            parts = [x] if torch.is_tensor(x) or not isinstance(x, (list, tuple)) else list(x)
            t = torch.cat([torch.as_tensor(p, dtype=torch.float32).reshape(-1).to(self._dev) for p in parts]).contiguous()
            if t.numel() != n:
                raise TfluidsError("optim.load_state: %s holds %d floats, the optimiser's state %d" % (name, t.numel(), n))
            return t
        fm, fv = flat(m, "m"), (flat(v, "v") if self.method == ADAM else None)
        if self.method == ADAM and (fm is None) != (fv is None):
            raise TfluidsError("optim.load_state: Adam restores m and v together")
        tfluids._call(lib, ctx, lib.tfl_optim_set_state(ctx, self._opt, None if fm is None else ctypes.c_void_p(fm.data_ptr()),
                                                        None if fv is None else ctypes.c_void_p(fv.data_ptr()), int(steps)))
        for t in (fm, fv):      # the copies read these on the stream: keep the caching allocator from handing them out before
            if t is not None:
                t.record_stream(torch.cuda.current_stream(self._dev))

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
