"""Host mirror of the rollout in torch/lib/calc_stats.lua:98-118: the divergence norm of the projected velocity over time,
the figure the reference judges a projection by (ConvNet against Jacobi against PCG).

The reference reads `div[i]:norm()` back per sample and per step (one host synchronisation each). Here every step's norms
go into a row of one device tensor (tfluids.velocityDivergenceNorm: two launches, no divergence field) and the host reads
that tensor once, after the last step."""
import torch

from . import tfluids
from ._lib import TfluidsError
from .simulate import getPUFlagsDensityReference, simulate, simulate_native


def calcStats(mconf, batch, model, nSteps, native=True):
    """calc_stats.lua:98-118 for one batch: column 0 of `normDiv` is ||velocityDivergence(U, flags)[b]||_2 of the state as
    given, columns 1 .. nSteps-1 follow one simulate() each (the state in `batch` advances in place, as in the reference).
    The steps run with gravityScale = 0 (calc_stats.lua:105). The reference writes that into the caller's mconf; this
    function works on a COPY and leaves the caller's mconf as it was. native: step through tfl_simulate_step
    (simulate_native) or through the operator-by-operator mirror (simulate). The dataset loop, pErr and UErr of
    calc_stats.lua are not part of this. Returns {"normDiv": float64 CPU tensor [B, nSteps]}; one host read in all."""
    if int(nSteps) != nSteps or nSteps < 1:
        raise TfluidsError("calcStats: nSteps must be a positive integer")
    _, U, flags, _ = getPUFlagsDensityReference(batch)
    if not (torch.is_tensor(U) and U.is_cuda and flags.is_cuda):
        raise TfluidsError("calcStats needs the batch on an MI355X (got CPU tensors); there is no CPU fallback")
    conf = dict(mconf)
    conf["gravityScale"] = 0
    step = simulate_native if native else simulate
    rows = torch.empty(int(nSteps), U.size(0), dtype=torch.float64, device=U.device)
    tfluids.velocityDivergenceNorm(U, flags, out=rows[0])
    for j in range(1, int(nSteps)):
        step(None, conf, batch, model, False)
        _, U, flags, _ = getPUFlagsDensityReference(batch)
        tfluids.velocityDivergenceNorm(U, flags, out=rows[j])
    return {"normDiv": rows.cpu().t().contiguous()}       # the one host read
