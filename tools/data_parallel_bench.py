"""Times what the data-parallel step adds to the guarded step on ONE GPU: pack + all-reduce + unpack of tfl_optim_step_reduced
over the native RCCL transport in a world of one, for the parameter sets of the 2-D default, the 3-D default and the 2-D `tog`
net. A world of one measures launch and RCCL call latency only: nothing crosses a link, and no step between two real GPUs is
measured here.
Forms, on twin nets with the same seeded gradients (Adam, clip at 1, a zero guard word):
  guarded          optim.step(guard)                       = tfl_optim_step_guarded
  reduced_inline   optim.step(guard, comm), the communicator issuing on the step's own stream (tfl_rccl_comm_set_inline 1)
  reduced_stream   the same with the communicator's own stream: two event hops per all-reduce
The protocol of tools/optim_step_bench.py: one process, the forms alternated round by round, a round = `calls` steps between two
device events after a synchronise, medians over the rounds, the host's wall time beside them; the library's event profile gives
the launches and the device time of the pack / unpack kernels by themselves. One JSON line per net.
usage: python tools/data_parallel_bench.py [--rounds 8] [--calls 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fluidnet_amd import FluidNetModel, ProjectionNet, dist, optim, tfluids  # noqa: E402


def measure(kind, is3D, rounds, calls):
    dev = torch.device("cuda:0")
    os.environ.pop("TFL_CONV_PATH", None)
    names = ("guarded", "reduced_inline", "reduced_stream")
    nets, opts = {}, {}
    for name in names:
        net = ProjectionNet(FluidNetModel.from_mconf(dict(modelType=kind), is3D, seed=3), device=dev)
        rng = np.random.RandomState(1)
        for p in net.parameters():
            p.grad = torch.from_numpy((rng.randn(*p.shape) * 0.01).astype(np.float32)).to(dev)
        nets[name], opts[name] = net, optim.Adam(net, gradNormThreshold=1.0, learningRate=0.0025, epsilon=1e-4)
    lib, ctx = tfluids._context(nets["guarded"].weights[0])
    if not lib.tfl_rccl_available(ctx):
        raise SystemExit("no RCCL could be bound: " + lib.tfl_last_error(ctx).decode())
    comms = {}
    for name, inline in (("reduced_inline", True), ("reduced_stream", False)):
        comms[name] = dist.RcclComm(ctx, dist.RcclComm.unique_id(ctx), 0, 1)
        comms[name].set_inline(inline)
    guard = torch.zeros(1, dtype=torch.int32, device=dev)
    forms = [(name, (lambda n=name: opts[n].step(guard=guard, comm=comms.get(n)))) for name in names]
    try:
        for _ in range(3):
            for _, fn in forms:
                fn()
        dev_us = {k: [] for k in names}
        host_us = {k: [] for k in names}
        for _ in range(rounds):
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                host_us[name].append((time.perf_counter() - t0) / calls * 1e6)
                dev_us[name].append(e0.elapsed_time(e1) / calls * 1e3)
        kernels = {}
        for name, fn in forms[:2]:
            with tfluids.profile(guard) as prof:
                for _ in range(calls):
                    fn()
            kernels[name] = {k: {"calls_per_step": v["calls"] / calls, "us_per_call": v["ms"] / v["calls"] * 1e3} for k, v in prof.kernels.items()}
    finally:
        torch.cuda.synchronize()
        for c in comms.values():
            c.close()
    med = {k: float(np.median(v)) for k, v in dev_us.items()}
    return {"what": "guarded step against the reduced step over RCCL in a world of one, %s %s net" % ("3-D" if is3D else "2-D", kind),
            "parameters": sum(p.numel() for p in nets["guarded"].parameters()), "device": torch.cuda.get_device_name(0),
            "hip": torch.version.hip, "rccl": lib.tfl_rccl_comm_origin(ctx).decode(), "rounds": rounds, "calls_per_round": calls,
            "us_per_step_median": med, "us_per_step_min_max": {k: [float(min(v)), float(max(v))] for k, v in dev_us.items()},
            "host_us_per_step_median": {k: float(np.median(v)) for k, v in host_us.items()},
            "pack_reduce_unpack_us": {k: med[k] - med["guarded"] for k in names[1:]},
            "kernels": kernels,
            "note": "a world of one: launch and RCCL call latency only; no link traffic and no step between two real GPUs is measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_parallel_bench needs an MI355X: nothing is measured without one")
    for kind, is3D in (("default", False), ("default", True), ("tog", False)):
        print(json.dumps(measure(kind, is3D, a.rounds, a.calls)), flush=True)


if __name__ == "__main__":
    main()
