"""Helper of tests/test_data_parallel_cpu.py and tests/test_hip_data_parallel.py: the inputs of the fp64 yardstick of the
data-parallel step and a restatement of its protocol in torch on the CPU.

N ranks with B items each compute the gradient of the mean over N B items: FluidCriterion averages over the batch, the net
treats every item by itself (its input scale is per item), so the mean of the ranks' gradients is the whole-batch gradient.
rank_inputs() are the mini-batches of the ranks (the scenes of tests/test_hip_run_epoch.py: 2-D 1 x 16 x 32 and 3-D 8 x 8 x 32,
B = 2), loss_grads() the parameter gradients of the criterion's loss through the net of tests/model_grad_ref.py in the dtype
asked for, and restated_step() the protocol -- both passes locally, then the mean over the ranks and the reduced guard, then one
update -- with the four mistakes tests/test_hip_data_parallel.py makes in its hand sequence (MISTAKES)."""
import numpy as np
import torch

import model_grad_ref as R
import scenes

DIMS = {False: (1, 16, 32), True: (8, 8, 32)}
B = 2
LAMBDAS = (1.0, 1.0, 1.0)
LONG_TERM_DIV_LAMBDA = 1.0
MISTAKES = ("sum-instead-of-mean", "guard-left-local", "reduce-before-the-long-term-pass", "rank-0-only")


def rank_inputs(is3D, rank, seed=31):
    """rank's mini-batch as numpy arrays: pDiv, UDiv, flags, density, and (manta) targets that are a damped copy of the inputs"""
    sc = scenes.make_scene(DIMS[is3D], seed=seed + rank, B=B, vel_cells=0.6)
    sc["U"][1] *= 0.4
    return dict(pDiv=sc["p"], UDiv=sc["U"], flags=sc["flags"], densityDiv=sc["density"],
                pTarget=sc["p"] * np.float32(0.5), UTarget=sc["U"] * np.float32(0.9))


def whole_batch(parts):
    """the ranks' mini-batches as one batch of N B items"""
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def loss_grads(model, inp, lambdas=LAMBDAS, dtype=torch.float64):
    """[(gradWeight, gradBias)] as float64 numpy arrays: d/dparams of nn.FluidCriterion's loss (sizeAverage, no border weight)
    on the net's outputs for the batch `inp`"""
    p, U, params = R.forward(model.layers, inp["pDiv"], inp["UDiv"], inp["flags"], model.opts, dtype)
    loss = R.criterion_loss(p, U, inp["pTarget"], inp["UTarget"], inp["flags"], lambdas)
    flat = [t for wb in params for t in wb]
    g = torch.autograd.grad(loss, flat)
    return [(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(len(params))]


def mean_of(grads_per_rank):
    """the rule of the reduced step in fp64: the ranks' gradients added in rank order, divided by their number"""
    n = len(grads_per_rank)
    out = []
    for l in range(len(grads_per_rank[0])):
        pair = []
        for j in (0, 1):
            acc = np.zeros_like(grads_per_rank[0][l][j])
            for g in grads_per_rank:
                acc = acc + g[l][j]
            pair.append(acc / n)
        out.append(tuple(pair))
    return out


def worst_rel_l2(got, want):
    return max(max(pair) for pair in R.rel_l2_per_tensor(got, want))


def restated_step(model, main, future, guards, lr=0.01, mistake=None, rank=0, dtype=torch.float64):
    """One data-parallel iteration as rank `rank` sees it, plain SGD standing in for the update: main[r] / future[r] = rank r's
    batch of the first pass and of the long-term pass (the rollout is not restated: a second scene stands for the advanced
    batch; it is scored with the divergence term alone, as the manta configuration scores it), guards[r] = its local guard.
    Returns (the reduced gradient, the parameters afterwards) as lists of (weight, bias) float64 arrays."""
    n = len(main)
    first = [loss_grads(model, main[r], LAMBDAS, dtype) for r in range(n)]
    second = [loss_grads(model, future[r], (0.0, 0.0, LONG_TERM_DIV_LAMBDA), dtype) for r in range(n)]
    local = [[(a[0] + b[0], a[1] + b[1]) for a, b in zip(first[r], second[r])] for r in range(n)]
    if mistake == "reduce-before-the-long-term-pass":
        local = first
    g = mean_of(local)
    if mistake == "sum-instead-of-mean":
        g = [(w * n, b * n) for w, b in g]
    if mistake == "rank-0-only":
        g = local[0]
    held = any(guards) if mistake != "guard-left-local" else bool(guards[rank])
    layers = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in model.layers]
    if not held:
        layers = [(w - lr * gw, b - lr * gb) for (w, b), (gw, gb) in zip(layers, g)]
    return g, layers
