"""Times what follows the backward pass of a training iteration -- the optimiser step and getting the new parameter values into
the native model -- for the 2-D default net and the 3-D default net at 32^3, in three forms:
  (a) torch.optim.Adam + the host push: parameters copied to the host, re-laid out there, tfl_model_set_weights (a stream
      synchronise and one synchronous copy per weight form) -- what ProjectionNet.push_parameters did before the device refresh
      existed, driven here through the same library function in the same order
  (b) torch.optim.Adam + the device push: tfl_model_set_weights_device from the parameters where they lie
  (c) the fused step: fluidnet_amd.optim.Adam = clip + Adam + the device refresh in one call
The protocol of profiles/model_backward.md: one process, the forms alternated round by round, a round = `calls` iterations
between two device events after a synchronise (the events see the stalls of a synchronous push too), medians over the rounds;
the host's wall time per iteration beside them. Launch counts from the library's event profile. Prints one JSON line per net
and, with --md, writes the record kept as profiles/optim_step.md.
usage: python tools/optim_step_bench.py [--rounds 8] [--calls 20] [--md PATH]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
from fluidnet_amd import FluidNetModel, ProjectionNet, optim, tfluids  # noqa: E402


def host_push(net):
    """the parent's ProjectionNet.push_parameters"""
    host = [(w.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy()) for w, b in zip(net.weights, net.biases)]
    lib, ctx = tfluids._context(net.weights[0])
    FP = ctypes.POINTER(ctypes.c_float)
    n = len(host)
    ws = (FP * n)(*[w.ctypes.data_as(FP) for w, _ in host])
    bs = (FP * n)(*[b.ctypes.data_as(FP) for _, b in host])
    tfluids._call(lib, ctx, lib.tfl_model_set_weights(ctx, net.net._handles[0], ws, bs))


def measure(is3D, dims, rounds, calls):
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(dims, seed=5, B=1, vel_cells=0.4)
    pDiv, UDiv, flags = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    cfg = dict(learningRate=0.0025, epsilon=1e-4)
    nets = {}
    for name in ("host", "device", "fused"):
        net = ProjectionNet(FluidNetModel.from_mconf(dict(modelType="default"), is3D, seed=3), device=dev).train()
        net.eval()(pDiv, UDiv, flags)                     # the native model exists
        rng = np.random.RandomState(1)
        for p in net.parameters():
            p.grad = torch.from_numpy((rng.randn(*p.shape) * 0.01).astype(np.float32)).to(dev)
        nets[name] = net
    topt = {k: torch.optim.Adam(nets[k].parameters(), lr=cfg["learningRate"], eps=cfg["epsilon"]) for k in ("host", "device")}
    fused = optim.Adam(nets["fused"], gradNormThreshold=1.0, **cfg)

    def a():
        topt["host"].step()
        host_push(nets["host"])

    def b():
        topt["device"].step()
        nets["device"]._sync()

    def c():
        fused.step()

    forms = (("adam+host_push", a), ("adam+device_push", b), ("fused_step", c))
    for _ in range(3):
        for _, fn in forms:
            fn()
    dev_us = {k: [] for k, _ in forms}
    host_us = {k: [] for k, _ in forms}
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
    launches = {}
    for name, fn in (("device_push", lambda: nets["device"]._push_device()), ("fused_step", c)):
        with tfluids.profile(pDiv) as prof:
            fn()
        launches[name] = {k: v["calls"] for k, v in prof.kernels.items()}
    nparam = sum(p.numel() for p in nets["fused"].parameters())
    return {"what": "optimiser step + weight push, %s default net" % ("3-D" if is3D else "2-D"), "grid": "x".join(map(str, dims)),
            "parameters": nparam, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rounds": rounds,
            "calls_per_round": calls, "us_per_iteration_median": {k: float(np.median(v)) for k, v in dev_us.items()},
            "us_per_iteration_min_max": {k: [float(min(v)), float(max(v))] for k, v in dev_us.items()},
            "host_us_per_iteration_median": {k: float(np.median(v)) for k, v in host_us.items()},
            "library_launches": launches,
            "note": "3-D default (fp16 MFMA path): the device push and the fused step end with a 12-byte read-back of the three "
                    "post-scales and the wait it implies" if is3D else "fully asynchronous"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench needs an MI355X: nothing is measured without one")
    res = [measure(False, (1, 128, 128), a.rounds, a.calls), measure(True, (32, 32, 32), a.rounds, a.calls)]
    for r in res:
        m = r["us_per_iteration_median"]
        r["device_paths_not_slower_than_host_push"] = bool(m["adam+device_push"] <= m["adam+host_push"] and m["fused_step"] <= m["adam+host_push"])
        print(json.dumps(r))
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("# Optimiser step and weight push (tools/optim_step_bench.py)\n\n")
            fh.write("What follows the backward pass of one training iteration, per iteration, medians over %d alternated rounds of %d "
                     "iterations between two device events (min .. max in brackets); host wall time beside it. %s, HIP %s.\n\n"
                     % (a.rounds, a.calls, res[0]["device"], res[0]["hip"]))
            fh.write("(a) torch.optim.Adam + the host push (parameters to the host, re-laid out there, tfl_model_set_weights: what a push "
                     "was before the device refresh). (b) torch.optim.Adam + tfl_model_set_weights_device. (c) fluidnet_amd.optim.Adam: "
                     "clip + Adam + refresh, one call.\n\n")
            for r in res:
                fh.write("## %s, grid %s, %d parameters\n\n" % (r["what"], r["grid"], r["parameters"]))
                fh.write("| form | device us / iteration | host us / iteration |\n|---|---|---|\n")
                for k in r["us_per_iteration_median"]:
                    lo, hi = r["us_per_iteration_min_max"][k]
                    fh.write("| %s | %.1f [%.1f .. %.1f] | %.1f |\n" % (k, r["us_per_iteration_median"][k], lo, hi,
                                                                        r["host_us_per_iteration_median"][k]))
                m = r["us_per_iteration_median"]
                fh.write("\nAgainst the host push: the device push takes %.2f of its time, the fused step %.2f (the condition: neither above 1).\n"
                         % (m["adam+device_push"] / m["adam+host_push"], m["fused_step"] / m["adam+host_push"]))
                fh.write("\nLibrary launches: device push %s; fused step %s. %s.\n\n"
                         % (json.dumps(r["library_launches"]["device_push"]), json.dumps(r["library_launches"]["fused_step"]), r["note"]))
    if not all(r["device_paths_not_slower_than_host_push"] for r in res):
        raise SystemExit("a device path is slower than the host push")


if __name__ == "__main__":
    main()
