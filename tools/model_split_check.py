#!/usr/bin/env python3
"""Bits and launches of the ConvNet host code, for comparing two builds of the library (TFL_LIBRARY=... picks one per process).

For every case of tests/model_grad_ref.py NAMES, tests/model_input_grad_ref.py EXTRA and tests/model_bank_grad_ref.py NAMES, on
that module's own make_inputs(name): the inference forward, forward_train, backward, backward_input, one fused Adam step and one
RMSprop step each followed by a forward. Prints, per call, the SHA-256 of every output array (p, U, tape, every gradient, the
parameters after the step, the optimiser state) and the per-kernel call counts from tfluids.profile. Two builds that do the
same thing print the same lines:

    TFL_LIBRARY=ab/parent.so python tools/model_split_check.py > parent.txt
    python tools/model_split_check.py > branch.txt && diff parent.txt branch.txt
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]

import model_bank_grad_ref as K      # noqa: E402
import model_grad_ref as R           # noqa: E402
import model_input_grad_ref as G     # noqa: E402
from fluidnet_amd import optim, tfluids  # noqa: E402
from fluidnet_amd._lib import TfluidsError  # noqa: E402
from fluidnet_amd.train import ProjectionNet  # noqa: E402

DEV = "cuda:0"


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def shas(ts):
    return "none" if ts is None else " ".join(sha(t) for t in ts)


def call(name, what, like, fn):
    """run fn under the library's profiler; print its arrays' sums and its launches (or the refusal); return what fn returned"""
    out = None
    try:
        with tfluids.profile(like) as prof:
            out = fn()
        print("%s %s launches %s" % (name, what, " ".join("%s:%d" % (k, v["calls"]) for k, v in sorted(prof.kernels.items()))))
    except TfluidsError as e:
        print("%s %s refused: %s" % (name, what, e))
    return out


def run(name, model, inputs):
    up = lambda a: torch.from_numpy(a.copy()).to(DEV)
    pDiv, UDiv, flags, gP, gU = (up(a) for a in inputs)
    net = ProjectionNet(model, device=DEV).eval()
    fwd = lambda: net(pDiv, UDiv, flags)
    out = call(name, "forward", flags, fwd)
    print(name, "forward p U", shas(out))
    out = call(name, "forward_train", flags, lambda: net.forward_train(pDiv, UDiv, flags))
    print(name, "forward_train p U tape", shas(out))
    if out is None:
        return
    p, U, tape = out
    g = call(name, "backward", flags, lambda: net.backward(flags, gP, gU, tape))
    if g is not None:
        print(name, "backward gradWeights", shas(g[0]), "gradBiases", shas(g[1]))
    gi = call(name, "backward_input", flags, lambda: net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape))
    if gi is not None:
        print(name, "backward_input gradWeights", shas(gi[0]), "gradBiases", shas(gi[1]), "gradPDiv", sha(gi[2]), "gradUDiv", sha(gi[3]))
    if g is None:
        return
    for cls in (optim.Adam, optim.RMSprop):
        for prm, grad in zip(list(net.weights) + list(net.biases), list(g[0]) + list(g[1])):
            prm.grad = grad.clone()
        opt = cls(net, gradNormThreshold=1.0)
        call(name, cls.__name__ + ".step", flags, opt.step)
        m, v = opt.state()
        print(name, cls.__name__, "parameters", shas(list(net.weights) + list(net.biases)), "m", shas(m), "v", shas(v))
        out = call(name, cls.__name__ + " forward", flags, fwd)
        print(name, cls.__name__, "forward p U", shas(out))
        opt.close()


def main():
    for name in R.NAMES + list(G.EXTRA):
        kind, is3D, opts = G.spec(name)
        run(name, R.make_model(kind, is3D, opts), G.make_inputs(name))
    for name in K.NAMES:
        run(name, K.make_model(name), K.make_inputs(name))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
