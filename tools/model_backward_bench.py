"""Times the training pass of the projection net -- tfl_model_forward_train + tfl_model_backward through
fluidnet_amd.ProjectionNet -- for the 3-D default net at 128^3 (B = 1) and the 2-D default net at 128^2 (B = 16), beside
torch.nn.functional.conv{2,3}d autograd (MIOpen) of the same convolution stack on the same GPU in the same process. The torch
side is the stack alone (net input given, gradient given at the last layer's output, weight and bias gradients only); ours also
forms the net input, the velocity update, its backward and the tape. One process; the two are alternated round by round; a
round is `calls` calls between two device events after a synchronise. Per-kernel times come from the library's event
profile. Prints one JSON line per net and, with --md, writes the record kept as profiles/model_backward.md.
usage: python tools/model_backward_bench.py [--rounds 8] [--calls 10] [--md PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scenes  # noqa: E402
from fluidnet_amd import FluidNetModel, ProjectionNet, tfluids  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12      # MI355X spec, FLOP/s


def measure(is3D, dims, B, rounds, calls):
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(dims, seed=5, B=B, vel_cells=0.4)
    pDiv, UDiv, flags = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    model = FluidNetModel.from_mconf(dict(modelType="default"), is3D, seed=3)
    net = ProjectionNet(model, device=dev).train()
    gP, gU = torch.randn_like(pDiv), torch.randn_like(UDiv)
    state = {}

    def ours():
        p, U, tape = net.forward_train(pDiv, UDiv, flags)
        state["g"] = net.backward(flags, gP, gU, tape, out=state.get("g"))

    conv = F.conv3d if is3D else F.conv2d
    ws = [torch.from_numpy(w).to(dev).requires_grad_(True) for w, _ in model.layers]
    bs = [torch.from_numpy(b).to(dev).requires_grad_(True) for _, b in model.layers]
    x = torch.randn(B, model.layers[0][0].shape[1], *(dims if is3D else dims[1:]), device=dev)
    gy = torch.randn(B, 1, *(dims if is3D else dims[1:]), device=dev)

    def theirs():
        h = x
        for l, (w, b) in enumerate(zip(ws, bs)):
            h = conv(h, w, b, padding=(w.shape[-1] - 1) // 2)
            if l + 1 < len(ws):
                h = torch.relu(h)
        return torch.autograd.grad(h, ws + bs, gy)

    for _ in range(3):
        ours(), theirs()
    times = {"ours": [], "torch": []}
    for _ in range(rounds):
        for name, fn in (("ours", ours), ("torch", theirs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    with tfluids.profile(pDiv) as prof:
        for _ in range(5):
            ours()
    kern = {k: v["ms"] / 5 * 1e3 for k, v in prof.kernels.items()}       # us per training pass, all launches of the kernel
    vox = float(B) * dims[0] * dims[1] * dims[2]
    flop = sum(2.0 * (w.shape[1] * int(np.prod(w.shape[2:])) + 1) * w.shape[0] * vox for w, _ in model.layers)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"what": "forward_train + backward, %s default net" % ("3-D" if is3D else "2-D"), "grid": "x".join(map(str, dims)), "B": B,
            "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rounds": rounds, "calls_per_round": calls,
            "us_per_call_median": med, "us_per_call_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "kernel_us_per_pass": kern, "wgrad_flop": flop,
            "k_conv_wgrad_frac_of_fp32_vector_peak": flop / (kern["k_conv_wgrad"] * 1e-6) / FP32_VECTOR_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_backward_bench needs an MI355X: nothing is measured without one")
    res = [measure(True, (128, 128, 128), 1, a.rounds, a.calls), measure(False, (1, 128, 128), 16, a.rounds, a.calls)]
    for r in res:
        print(json.dumps(r), flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("# Training pass of the projection net (tools/model_backward_bench.py)\n\n")
            fh.write("%s, HIP %s. %d rounds of %d calls each, ours and torch alternated round by round, device events around a round "
                     "after a synchronise; medians of the rounds. No bar was set for this: it records what was measured.\n\n"
                     % (res[0]["device"], res[0]["hip"], a.rounds, a.calls))
            fh.write("(a) ours: ProjectionNet.forward_train + .backward = tfl_model_forward_train + tfl_model_backward (wall BCs, divergence, "
                     "input scale, net input, the conv stack on the shape-generic fp32 kernels, velocity update; then its backward, "
                     "per layer the weight / bias gradient and the data gradient), gradP and gradU given.\n"
                     "(b) torch: F.conv%s autograd (MIOpen) of the convolution stack alone -- forward with ReLU, then "
                     "torch.autograd.grad to the weights and biases from a given gradient at the last layer's output. It does less "
                     "than (a): no head, no tail, no tape copy.\n\n" % "{2,3}d")
            fh.write("| net | (a) us per pass | min .. max | (b) us per pass | min .. max | (a) / (b) |\n|---|---|---|---|---|---|\n")
            for r in res:
                m, mm = r["us_per_call_median"], r["us_per_call_min_max"]
                # (no ratio for the 3-D row: F.conv3d autograd takes most of a second on this stack, which is no yardstick)
                ratio = "not comparable (see below)" if r["grid"].count("x") == 2 and not r["grid"].startswith("1x") else "%.2f" % (m["ours"] / m["torch"])
                fh.write("| %s, %s, B = %d | %.0f | %.0f .. %.0f | %.0f | %.0f .. %.0f | %s |\n"
                         % (r["what"].split(", ")[1], r["grid"], r["B"], m["ours"], mm["ours"][0], mm["ours"][1], m["torch"], mm["torch"][0],
                            mm["torch"][1], ratio))
            fh.write("\nThe time of (b) on the 3-D net is what F.conv3d autograd took on this stack (k = 3 and k = 1 layers of 3 - 8 channels) "
                     "in this process, round after round; which MIOpen solver it ran was not looked into, it says nothing about a "
                     "tuned MIOpen, and no speed claim is made against it. (b) also does less work than (a). What matters for "
                     "follow-up work is below: k_conv_wgrad's fraction of the fp32 vector peak, and k_conv_wgrad_finish, which at "
                     "2-D costs as much as the data-gradient convolutions.\n")
            for r in res:
                fh.write("\n%s, %s: kernel time per pass from the library's per-kernel event timing (5 passes, every launch of a kernel "
                         "added up): %s.\n" % (r["what"].split(", ")[1], r["grid"],
                                               ", ".join("%s %.0f us" % kv for kv in sorted(r["kernel_us_per_pass"].items(), key=lambda kv: -kv[1]))))
                fh.write("k_conv_wgrad: %.2f GFLOP of fmaf per pass over the five layers (2 (cin taps + 1) cout per voxel) = %.1f %% of the "
                         "157.3 TFLOP/s fp32 vector peak (spec).\n" % (r["wgrad_flop"] / 1e9, 100 * r["k_conv_wgrad_frac_of_fp32_vector_peak"]))
            fh.write("\nThe event timing adds a few microseconds to every kernel it brackets; the per-pass medians above are taken "
                     "without it. No counter pass was taken: what bounds k_conv_wgrad (LDS reads per fmaf, or the one-row-per-thread "
                     "mapping that leaves threads idle on the narrow layers) was not measured.\n")


if __name__ == "__main__":
    main()
