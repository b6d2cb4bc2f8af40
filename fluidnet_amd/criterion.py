"""nn.FluidCriterion (torch/lib/modules/fluid_criterion.lua) as a torch.nn.Module on the HIP operators: the figure the
reference scores a projection net with (pressure, velocity and divergence MSE terms, optionally weighted towards the cells
next to obstacles) and its gradient to the model's outputs.

The reference composes the criterion from three (Weighted)MSECriterions, tfluids.signedDistanceField and the
VelocityDivergence module, and reads three losses back to the host. Here one call of tfluids.fluidCriterion (two launches,
include/tfluids_hip.h tfl_fluidCriterion) forms the three losses, their total and -- when an input requires grad -- both
gradients; every loss stays a 0-d float64 tensor on the device, so nothing is read back. Everything is fp32 on an MI355X; there
is no CPU fallback."""
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import tfluids
from ._lib import TfluidsError


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


class _FluidCriterionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pPred, UPred, pTarget, UTarget, flags, weight, pLambda, uLambda, divLambda, sizeAverage):
        pPred, UPred = _c(pPred), _c(UPred)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss = torch.empty(4, dtype=torch.float64, device=UPred.device)
        gradP = torch.empty_like(pPred) if need else None
        gradU = torch.empty_like(UPred) if need else None
        tfluids.fluidCriterion(pPred, UPred, _c(pTarget), _c(UTarget), _c(flags), weight, pLambda, uLambda, divLambda,
                               sizeAverage, loss, gradP, gradU)
        if need:
            ctx.save_for_backward(gradP, gradU)
        return loss                                   # {pLoss, uLoss, divLoss, total}: the gradients are the total's

    @staticmethod
    @once_differentiable                              # gradP / gradU are plain buffers: there is no second derivative
    def backward(ctx, grad_loss):
        gradP, gradU = ctx.saved_tensors
        g = grad_loss[3].to(gradP.dtype)
        return ((gradP * g) if ctx.needs_input_grad[0] else None, (gradU * g) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None, None)


class FluidCriterion(torch.nn.Module):
    """nn.FluidCriterion(pLambda, uLambda, divLambda, borderWeight, borderWidth): forward((pPred, UPred), (pTarget, UTarget,
    flags)) -> the total loss, a 0-d float64 DEVICE tensor with autograd to pPred and UPred (none to the targets or flags).
    After a forward .pLoss / .uLoss / .divLoss hold the three terms (0-d device tensors). The lambdas and sizeAverage are plain
    attributes the caller may change between calls (lib/run_epoch.lua:276-298 does); a term whose lambda is <= 0 is 0 and adds
    nothing to the gradients. borderWeight = None (or 1) disables the weighting, as in the reference."""

    def __init__(self, pLambda, uLambda, divLambda, borderWeight=None, borderWidth=None):
        super().__init__()
        self.pLambda, self.uLambda, self.divLambda = pLambda, uLambda, divLambda
        if borderWeight is not None:
            if borderWidth is None:
                raise TfluidsError("you must specify borderWidth with borderWeight")
            if not (borderWidth > 1 and int(borderWidth) == borderWidth):
                raise TfluidsError("borderWidth must a positive integer > 1")
            if borderWeight != 1 and not borderWeight > 1:
                raise TfluidsError("borderWeight must be > 1 (or 1 / None to disable)")
            self.borderWeight, self.borderWidth = borderWeight, int(borderWidth)
        else:
            self.borderWeight, self.borderWidth = 1, 2      # disabled; the width is a dummy, as in the reference
        self.sizeAverage = True
        self.pLoss = self.uLoss = self.divLoss = None
        self._weight_of, self._weight_key, self._weight = None, None, None

    def weight(self, flags):
        """the border weight of `flags` (None when disabled): computed once per flags tensor and content version. The cache
        holds for THIS tensor object (a weak reference: a new tensor that the allocator puts at a freed tensor's address is a
        miss) at this (data_ptr, _version, borderWidth, borderWeight); new content reaches it as an in-place update (which
        bumps _version) or as a new tensor. A miss writes a NEW weight tensor: one returned earlier never changes."""
        if self.borderWeight == 1:
            return None
        key = (flags.data_ptr(), flags._version, self.borderWidth, self.borderWeight)
        held = self._weight_of() if self._weight_of is not None else None
        if held is not flags or key != self._weight_key:
            self._weight = tfluids.criterionWeight(_c(flags.detach()), self.borderWidth, self.borderWeight)
            self._weight_of, self._weight_key = weakref.ref(flags), key
        return self._weight

    def forward(self, input, target):
        tfluids._check(isinstance(input, (list, tuple)) and len(input) == 2, "input must be (pPred, UPred)")
        tfluids._check(isinstance(target, (list, tuple)) and len(target) == 3, "target must be (pTarget, UTarget, flags)")
        pPred, UPred = input
        pTarget, UTarget, flags = target
        for t in (pPred, UPred, pTarget, UTarget, flags):
            tfluids._check(torch.is_tensor(t) and t.dim() == 5, "Dimension mismatch")
            tfluids._check(t.is_cuda and t.device == UPred.device,
                           "FluidCriterion needs every tensor on one MI355X (got a CPU tensor or two devices); there is no CPU fallback")
        weight = self.weight(flags)                   # (keyed on the caller's tensor, not on a contiguous temporary of it)
        flags = _c(flags.detach())
        loss = _FluidCriterionFn.apply(pPred, UPred, pTarget.detach(), UTarget.detach(), flags, weight,
                                       float(self.pLambda), float(self.uLambda), float(self.divLambda), bool(self.sizeAverage))
        terms = loss.detach()
        self.pLoss, self.uLoss, self.divLoss = terms[0], terms[1], terms[2]
        return loss[3]

    def extra_repr(self):
        return "pLambda=%.2f, uLambda=%.2f, divLambda=%.2f, borderWeight=%.1f, borderWidth=%d" % (
            self.pLambda, self.uLambda, self.divLambda, self.borderWeight, self.borderWidth)
