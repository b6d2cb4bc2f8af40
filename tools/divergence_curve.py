"""The divergence norm of the projected velocity over time (stats.calcStats, the rollout of lib/calc_stats.lua:98-118) for three
projections on BASELINE config 2's scene (2-D 128^2 plume; the ConvNet is the reference's shipped myModel2D, the only trained
model this repository has): ConvNet, Jacobi with 20 iterations, PCG. 64 steps each from the same start state. Prints one JSON
line per method with the normDiv curve and writes the table to profiles/divergence_curve.md. A record; it asserts nothing.
usage: python tools/divergence_curve.py [--steps 64] [--out profiles/divergence_curve.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_amd import FluidNetModel, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "divergence_curve.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "myModel2D_weights.npz"))
    model = FluidNetModel([(z["w%d" % i], z["b%d" % i]) for i in range(5)], False)
    base = dict(dt=4 / 60, advectionMethod="maccormackOurs", maccormackStrength=0.75, buoyancyScale=1.0, gravityScale=0,
                vorticityConfinementAmp=0)
    methods = [("convnet (myModel2D)", dict(base, simMethod="convnet"), model),
               ("jacobi, 20 iterations", dict(base, simMethod="jacobi", maxIter=20), None),
               ("pcg", dict(base, simMethod="pcg"), None)]
    curves = {}
    for name, mconf, m in methods:
        batch = bench._plume_scene((1, 128, 128), 0.05, 10.0, dev)
        curve = stats.calcStats(mconf, batch, m, a.steps)["normDiv"][0].tolist()
        curves[name] = curve
        print(json.dumps({"method": name, "steps": a.steps, "normDiv": curve}), flush=True)
    names = [n for n, _, _ in methods]
    lines = ["# Divergence norm over time, BASELINE config 2 (2-D 128x128 plume)", "",
             "`python tools/divergence_curve.py`: `stats.calcStats` (the rollout of `lib/calc_stats.lua:98-118`), %d steps from the same" % a.steps,
             "start state, `||velocityDivergence(U, flags)||_2` after every step (column 0: the state as given). Device: %s." % torch.cuda.get_device_name(0),
             "A record of what the three projections give here; nothing is asserted about it.", "",
             "| step | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]
    for j in range(a.steps):
        lines.append("| %d | " % j + " | ".join("%.6e" % curves[n][j] for n in names) + " |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
