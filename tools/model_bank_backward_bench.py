"""Times the training pass of banked projection nets -- tfl_model_forward_train + tfl_model_backward through
fluidnet_amd.ProjectionNet -- for `mres3_add` and `dilate3_concat` (three banks on the default layer table) at
128^3 (B = 1) and at 2-D 128^2 (B = 16), beside the linear default net's pass on the same grid in the same process (the code path
of the linear models: the yardstick). The three are alternated round by round; a round is `calls` passes between two device
events after a synchronise. Per-kernel times come from the library's event profile; the three bank kernels' share of the pass
(k_join_bwd, k_pyr_pool_bwd, k_bank_sum) is reported, not asserted. Prints one JSON line per grid and, with --md, writes the
record kept as profiles/model_bank_backward.md (--accuracy FILE: lines "bank ... witness" of the GPU tests' output, summarised
into the same record).
usage: python tools/model_bank_backward_bench.py [--rounds 8] [--calls 10] [--md PATH] [--accuracy LOG]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
from fluidnet_amd import FluidNetModel, ProjectionNet, tfluids  # noqa: E402

NETS = (("linear", dict(modelType="default")),
        ("mres3_add", dict(modelType="default", banksNum=3, banksType="mres", banksAggregateMethod="add")),
        ("dilate3_concat", dict(modelType="default", banksNum=3, banksType="dilate", banksAggregateMethod="concat")))
BANK_KERNELS = ("k_join_bwd", "k_pyr_pool_bwd", "k_bank_sum")


def measure(is3D, dims, B, rounds, calls):
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(dims, seed=5, B=B, vel_cells=0.4)
    pDiv, UDiv, flags = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    gP, gU = torch.randn_like(pDiv), torch.randn_like(UDiv)
    passes = {}
    for name, mconf in NETS:
        net = ProjectionNet(FluidNetModel.from_mconf(mconf, is3D, seed=3), device=dev).train()
        state = {}

        def one(net=net, state=state):
            _, _, tape = net.forward_train(pDiv, UDiv, flags)
            state["g"] = net.backward(flags, gP, gU, tape, out=state.get("g"))
        passes[name] = one
    for _ in range(3):
        for fn in passes.values():
            fn()
    times = {k: [] for k in passes}
    for _ in range(rounds):
        for name, fn in passes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    kern = {}
    for name, fn in passes.items():
        with tfluids.profile(pDiv) as prof:
            for _ in range(5):
                fn()
        kern[name] = {k: v["ms"] / 5 * 1e3 for k, v in prof.kernels.items()}      # us per pass, all launches of the kernel
    share = {name: sum(kern[name].get(k, 0.0) for k in BANK_KERNELS) / max(sum(kern[name].values()), 1e-9) for name in passes}
    return {"what": "forward_train + backward, %s default table" % ("3-D" if is3D else "2-D"), "grid": "x".join(map(str, dims)), "B": B,
            "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rounds": rounds, "calls_per_round": calls,
            "us_per_pass_median": {k: float(np.median(v)) for k, v in times.items()},
            "us_per_pass_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "kernel_us_per_pass": kern, "bank_kernels_share_of_kernel_time": share}


def accuracy(path):
    """(worst rel-L2, worst witness ratio, lines) per kind from the GPU tests' printed witnesses"""
    out = {}
    pat = {"parameter gradients": re.compile(r"bank grad witness (\S+) (\S+): ours (\S+), PyTorch fp32 (\S+), ratio (\S+)"),
           "input gradients": re.compile(r"bank input-grad witness (\S+) (\S+): gradPDiv ours (\S+) PyTorch fp32 \S+, gradUDiv ours (\S+) "
                                         r"PyTorch fp32 \S+, ratio (\S+)")}
    for line in open(path):
        for kind, rx in pat.items():
            m = rx.search(line)
            if not m:
                continue
            ours = float(m.group(3)) if kind == "parameter gradients" else max(float(m.group(3)), float(m.group(4)))
            o = out.setdefault(kind, {"worst": (0.0, ""), "ratio": (0.0, ""), "n": 0})
            o["n"] += 1
            o["worst"] = max(o["worst"], (ours, "%s %s" % (m.group(1), m.group(2))))
            o["ratio"] = max(o["ratio"], (float(m.group(5)), "%s %s" % (m.group(1), m.group(2))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--md", default=None)
    ap.add_argument("--accuracy", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_bank_backward_bench needs an MI355X: nothing is measured without one")
    res = [measure(True, (128, 128, 128), 1, a.rounds, a.calls), measure(False, (1, 128, 128), 16, a.rounds, a.calls)]
    for r in res:
        print(json.dumps(r), flush=True)
    if not a.md:
        return
    with open(a.md, "w") as fh:
        fh.write("# Training pass of banked projection nets (tools/model_bank_backward_bench.py)\n\n")
        fh.write("%s, HIP %s. %d rounds of %d passes each, the three nets alternated round by round, device events around a round after "
                 "a synchronise; medians of the rounds. A pass = ProjectionNet.forward_train + .backward (tfl_model_forward_train + "
                 "tfl_model_backward), gradP and gradU given. No time bar was set: this records what was measured.\n\n"
                 % (res[0]["device"], res[0]["hip"], a.rounds, a.calls))
        fh.write("Yardstick: `linear`, the default net without banks on the same grid in the same session -- the linear models' code "
                 "path (k_conv_direct data gradients, k_conv_wgrad at tap spacing 1). `mres3_add` and `dilate3_concat` run the default "
                 "table with three banks over stages 1 and 2: seven more conv modules than `linear`, so more work by construction.\n\n")
        fh.write("| grid | net | us per pass | min .. max | / linear | k_join_bwd + k_pyr_pool_bwd + k_bank_sum, share of kernel time |\n"
                 "|---|---|---|---|---|---|\n")
        for r in res:
            m, mm = r["us_per_pass_median"], r["us_per_pass_min_max"]
            for name in m:
                fh.write("| %s, B = %d | %s | %.0f | %.0f .. %.0f | %.2f | %.1f %% |\n"
                         % (r["grid"], r["B"], name, m[name], mm[name][0], mm[name][1], m[name] / m["linear"],
                            100 * r["bank_kernels_share_of_kernel_time"][name]))
        for r in res:
            for name, k in r["kernel_us_per_pass"].items():
                fh.write("\n%s, B = %d, %s: kernel time per pass from the library's per-kernel event timing (5 passes, every launch of a "
                         "kernel added up): %s.\n" % (r["grid"], r["B"], name,
                                                      ", ".join("%s %.0f us" % kv for kv in sorted(k.items(), key=lambda kv: -kv[1]))))
        fh.write("\nThe event timing adds a few microseconds to every kernel it brackets, which weighs most on the short bank kernels: "
                 "their share above is an upper estimate. The per-pass medians are taken without it. No counter pass was taken.\n")
        fh.write("\nWhat the table shows. The three bank kernels stay a small fraction of the pass. k_pyr_pool_bwd and k_bank_sum do not appear: both nets split at the first stage (banksSplitStage = 1, the default), where the split's backward only runs for the input gradients (tfl_model_backward_input); tests/test_hip_model_bank_backward.py runs them. The long pole of `dilate3_concat` in 3-D is k_conv_wgrad itself: at tap spacing 4 the halo tile is (32 + 8) x (8 + 8) x 9 floats per channel, two input channels fit the 48 KB tile where eight fit at spacing 1, so a layer takes four times the chunks, each staging the tile and the gradient again. A tile shape chosen for the dilated halo is the lead; it was not tried here.\n")
        if a.accuracy:
            fh.write("\n## Accuracy (tests/test_hip_model_bank_backward.py, same machine)\n\n"
                     "Per-tensor rel-L2 against the fp64 restatement (tests/model_bank_grad_ref.py), bar 1e-5; witness ratio = our error over "
                     "PyTorch-CPU-fp32 autograd's on the same inputs.\n\n")
            for kind, o in accuracy(a.accuracy).items():
                fh.write("- %s, %d case x mode runs: worst rel-L2 %.3e (%s); worst witness ratio %.2f (%s).\n"
                         % (kind, o["n"], o["worst"][0], o["worst"][1], o["ratio"][0], o["ratio"][1]))


if __name__ == "__main__":
    main()
