"""Times the divergence norm (divnorm.hip: k_divnorm_planes + k_divnorm_finish) against the k_divergence launch of
tfl_velocityDivergenceForward on the same arrays, in one process, with the library's own per-kernel HIP-event timing
(tfluids.profile): 20 calls after 3 warm-ups at 128^3 and 256^3, the two operators interleaved round by round. Also a 64-step
rollout on BASELINE config 2 (2-D 128^2, the shipped myModel2D weights): stats.calcStats (one host read) against the
reference's way (velocityDivergenceForward, norm(), .item() per sample and step). Prints one JSON line per measurement.
usage: python tools/divnorm_bench.py [--sizes 128,256]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_amd import FluidNetModel, stats, tfluids  # noqa: E402
from fluidnet_amd.simulate import simulate_native  # noqa: E402


def kernels(n):
    dev = torch.device("cuda:0")
    batch, mconf = bench.build_scene(n, n, None, dev)
    model = FluidNetModel.default_3d(seed=1)
    for _ in range(3):
        simulate_native(None, mconf, batch, model)
    U, flags = batch["UDiv"], batch["flags"]
    div = torch.empty_like(flags)
    for _ in range(3):
        tfluids.velocityDivergenceForward(U, flags, div)
        tfluids.velocityDivergenceNorm(U, flags)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(4):               # 4 rounds x 5 calls = 20 calls each, interleaved
        with tfluids.profile(U) as prof:
            for _ in range(5):
                tfluids.velocityDivergenceForward(U, flags, div)
                tfluids.velocityDivergenceNorm(U, flags)
        rounds.append({k: v["ms"] / v["calls"] * 1e3 for k, v in prof.kernels.items()})
    us = {k: float(np.mean([r[k] for r in rounds])) for k in rounds[0]}
    both = us["k_divnorm_planes"] + us["k_divnorm_finish"]
    cells = float(n) ** 3
    print(json.dumps({"what": "divnorm kernels", "grid": "%d^3" % n, "us": us, "rounds_us": rounds, "divnorm_us": both,
                      "ratio_to_k_divergence": both / us["k_divergence"],
                      "k_divnorm_planes_TBps": 16 * cells / us["k_divnorm_planes"] / 1e6,
                      "k_divergence_TBps": 20 * cells / us["k_divergence"] / 1e6}), flush=True)


def rollout(steps=64):
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "myModel2D_weights.npz"))
    model = FluidNetModel([(z["w%d" % i], z["b%d" % i]) for i in range(5)], False)
    mconf = dict(dt=4 / 60, advectionMethod="maccormackOurs", maccormackStrength=0.75, buoyancyScale=1.0, gravityScale=0,
                 vorticityConfinementAmp=0, simMethod="convnet")

    def reference_way(b):
        U, flags = b["UDiv"], b["flags"]
        div = torch.empty_like(flags)
        out = np.zeros((U.size(0), steps))
        for j in range(steps):
            if j:
                simulate_native(None, mconf, b, model)
            tfluids.velocityDivergenceForward(U, flags, div)
            for i in range(U.size(0)):
                out[i, j] = div[i].norm().item()
        return out
    res = {}
    for name, fn in (("calcStats", lambda b: stats.calcStats(mconf, b, model, steps)["normDiv"].numpy()), ("reference_way", reference_way)):
        times = []
        for rep in range(4):         # the first repetition warms up
            b = bench._plume_scene((1, 128, 128), 0.05, 10.0, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            curve = fn(b)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"ms_per_rollout": float(np.median(times[1:])), "all_ms": times, "last": float(curve[0, -1])}
    print(json.dumps({"what": "64-step rollout, config 2 (2-D 128^2)", "steps": steps, **res}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    a = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip}), flush=True)
    for n in a.sizes.split(","):
        kernels(int(n))
    rollout()
