"""Per-rank compute of the z-slab step estimated on ONE GPU: W virtual ranks (threads, ThreadComm: halos move by device
copies) advance the bench scene; all ranks share one stream, so wall time / W ~ the kernel time one real rank spends per
step (no RCCL, no overlap). Also prints rank 0's per-kernel table.
usage: slab_virtual_bench.py [res] [world] [steps] [--sim jacobi [--iters N]] [--advection METHOD] [--density-channels N]
                             [--model default|tog|yang]
--sim jacobi: the Jacobi projection (no model, N sweeps per step, default 34 -- the 3-D driver's count), with the un-cut
single-GPU Jacobi step at the same size printed beside it.
--advection: any method of tfl_simulate_step (default maccormackOurs, the bench's); --density-channels: the plume's density
carried in N channels (default 1). Either option also prints the un-cut single-GPU step of the same configuration.
--model: the projection net (default: the 3-D default topology; tog / yang: lib/model.lua's layer tables on the shape-generic
kernels, laid out with the model halo); tog / yang also print the un-cut step and, per layer, the planes a middle
rank computes over the planes it owns."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fluidnet_amd import FluidNetModel, tfluids  # noqa: E402
from fluidnet_amd.dist import SlabLayout, SlabSimulation, ThreadComm, run_virtual_ranks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("res", nargs="?", type=int, default=128)
ap.add_argument("world", nargs="?", type=int, default=8)
ap.add_argument("steps", nargs="?", type=int, default=20)
ap.add_argument("--sim", default="convnet", choices=("convnet", "jacobi"))
ap.add_argument("--iters", type=int, default=34)
ap.add_argument("--advection", default="maccormackOurs",
                choices=("euler", "maccormack", "eulerOurs", "rk2Ours", "rk3Ours", "maccormackOurs"))
ap.add_argument("--density-channels", type=int, default=1)
ap.add_argument("--model", default="default", choices=("default", "tog", "yang"))
ap.add_argument("--no-uncut", action="store_true", help="skip the un-cut comparison (a kernel trace of the rank-steps alone)")
args = ap.parse_args()
res, world, steps = args.res, args.world, args.steps
dev = torch.device("cuda:0")
model = None
if args.sim == "convnet":
    model = {"default": lambda: FluidNetModel.default_3d(seed=1), "tog": lambda: FluidNetModel.tog(True, seed=1),
             "yang": lambda: FluidNetModel.from_mconf(dict(modelType="yang"), True, seed=1)}[args.model]()


def scene(lay):
    batch, mconf = bench.build_scene(res, res, lay, dev)
    if args.sim == "jacobi":
        mconf = dict(mconf, simMethod="jacobi", maxIter=args.iters)
    mconf = dict(mconf, advectionMethod=args.advection)
    if args.density_channels > 1:
        n = args.density_channels
        batch["density"] = [batch["density"].clone() for _ in range(n)]
        for k in ("densityBC", "densityBCInvMask"):
            if batch.get(k) is not None:
                batch[k] = [batch[k].clone() for _ in range(n)]
    return batch, mconf


if not args.no_uncut and (args.sim == "jacobi" or args.advection != "maccormackOurs" or args.density_channels > 1 or args.model != "default"):
    # the un-cut single-GPU step on the same scene, for comparison
    from fluidnet_amd.simulate import simulate_native
    batch, mconf = scene(None)
    for _ in range(3):
        simulate_native(None, mconf, batch, model)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        simulate_native(None, mconf, batch, model)
    torch.cuda.synchronize()
    print("res %d un-cut %s (%s), %s, %d density channel(s)%s: %.3f ms per step"
          % (res, args.sim, args.model, args.advection, args.density_channels,
             " (%d sweeps)" % args.iters if args.sim == "jacobi" else "", (time.time() - t0) / steps * 1e3))
    if args.model != "default":
        with tfluids.profile(batch["UDiv"]) as prof:
            for _ in range(5):
                simulate_native(None, mconf, batch, model)
        print("  un-cut kernels: %.1f us/step" % (sum(rec["ms"] for rec in prof.kernels.values()) / 5 * 1e3))
    del batch
if model is not None and args.model != "default" and world > 1:
    from fluidnet_amd.dist import model_cone
    cone, per = model_cone(model), res // world
    print("  planes computed / owned on a middle rank (%d owned), per layer:" % per)
    for i, L in enumerate(cone["layers"]):
        own = per // L["d"]
        print("    layer %d (grid/%d): conv %s -> %.2f%s" % (i + 1, L["d"], L["conv"], (own + sum(L["conv"])) / own,
                                                         ", pool %s" % (L["pool"],) if L["pool"] else ""))
hub = ThreadComm.Hub(world)
sims = []
for r in range(world):
    lay = SlabLayout(res, world, r, model=model if args.model != "default" else None)
    batch, mconf = scene(lay)
    sims.append(SlabSimulation(batch, mconf, model, lay, ThreadComm(hub, r), own_context=True))
run_virtual_ranks(sims, 6)
torch.cuda.synchronize()
t0 = time.time()
run_virtual_ranks(sims, steps)
torch.cuda.synchronize()
dt = (time.time() - t0) / steps
print("[%s %s, %s, %d ch] res %d, %d virtual ranks: %.3f ms per step for all ranks = %.3f ms per rank-step (single GPU un-split: see bench.py)"
      % (args.sim, args.model, args.advection, args.density_channels, res, world, dt * 1e3, dt * 1e3 / world))
with tfluids.profile(sims[0].batch["UDiv"]) as prof:
    run_virtual_ranks(sims, 5)
tot = 0.0
for name, rec in sorted(prof.kernels.items(), key=lambda kv: -kv[1]["ms"]):
    print("  %-28s %7.1f us/step  (%.1f launches)" % (name, rec["ms"] / 5 * 1e3, rec["calls"] / 5))
    tot += rec["ms"] / 5
print("  rank 0 kernels: %.1f us/step" % (tot * 1e3))
