"""Times what the input gradients of the projection net cost: tfl_model_forward_train + tfl_model_backward_input beside
tfl_model_forward_train + tfl_model_backward, through fluidnet_amd.ProjectionNet, for the 2-D default net at 128^2 (B = 16) and
the 3-D default net at 64^3 and 128^3 (B = 1). The protocol of tools/model_backward_bench.py: one process, the two sides
alternated round by round, a round is `calls` calls between two device events after a synchronise, medians of the rounds with
min .. max; per-kernel times from the library's event profile.

--parent-root PATH: also holds tfl_model_backward of this build against another build's (a built checkout of the parent commit at
PATH), in child processes started alternately, one at a time. The child of the other build imports ITS fluidnet_amd package with
its library: this build's loader refuses a library that lacks a symbol it declares, so TFL_LIBRARY alone cannot select a
library from before tfl_model_backward_input.
--accuracy-log PATH: the -s output of tests/test_hip_model_input_grad.py; its witness lines become the accuracy table.
Prints one JSON line per measurement and, with --md, writes the record kept as profiles/model_input_grad.md.
usage: python tools/model_input_grad_bench.py [--rounds 8] [--calls 10] [--parent-root PATH] [--accuracy-log PATH] [--md PATH]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(False, (1, 128, 128), 16), (True, (64, 64, 64), 1), (True, (128, 128, 128), 1)]
NEW_KERNELS = ("k_input_grad_sums", "k_input_grad_sums_finish", "k_input_grad_head")
HEAD_KERNELS = ("k_net_input", "k_project", "k_bcs_div_stats")


def _setup(root, is3D, dims, B):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import torch
    import scenes
    from fluidnet_amd import FluidNetModel, ProjectionNet
    dev = torch.device("cuda:0")
    sc = scenes.make_scene(dims, seed=5, B=B, vel_cells=0.4)
    pDiv, UDiv, flags = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    net = ProjectionNet(FluidNetModel.from_mconf(dict(modelType="default"), is3D, seed=3), device=dev).train()
    torch.manual_seed(7)
    return torch, net, pDiv, UDiv, flags, torch.randn_like(pDiv), torch.randn_like(UDiv)


def _rounds(torch, fns, rounds, calls):
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return times


def measure(is3D, dims, B, rounds, calls):
    torch, net, pDiv, UDiv, flags, gP, gU = _setup(ROOT, is3D, dims, B)
    from fluidnet_amd import tfluids
    state = {}

    def with_input():
        p, U, tape = net.forward_train(pDiv, UDiv, flags)
        r = net.backward_input(flags, pDiv, UDiv, U, gP, gU, tape, out=state.get("gi"))
        state["gi"] = (r[0], r[1])

    def without():
        p, U, tape = net.forward_train(pDiv, UDiv, flags)
        state["g"] = net.backward(flags, gP, gU, tape, out=state.get("g"))

    times = _rounds(torch, {"backward_input": with_input, "backward": without}, rounds, calls)
    kern = {}
    for name, fn in (("backward_input", with_input), ("backward", without)):
        with tfluids.profile(pDiv) as prof:
            for _ in range(5):
                fn()
        kern[name] = {k: v["ms"] / 5 * 1e3 for k, v in prof.kernels.items()}
    return {"what": "forward_train + backward_input | backward, %s default net" % ("3-D" if is3D else "2-D"), "grid": "x".join(map(str, dims)),
            "B": B, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rounds": rounds, "calls_per_round": calls,
            "us_per_call": times, "kernel_us_per_pass": kern}


def child_backward(root, is3D, dims, B, rounds, calls):
    """one build's forward_train + backward, `rounds` rounds: the unit the A/B alternates"""
    torch, net, pDiv, UDiv, flags, gP, gU = _setup(root, is3D, dims, B)
    state = {}

    def fn():
        p, U, tape = net.forward_train(pDiv, UDiv, flags)
        state["g"] = net.backward(flags, gP, gU, tape, out=state.get("g"))

    print(json.dumps(_rounds(torch, {"backward": fn}, rounds, calls)["backward"]), flush=True)


def ab(parent_root, rounds, calls):
    out = []
    for is3D, dims, B in SIZES:
        sides = {"this": [], "parent": []}
        for turn in range(4):      # this, parent, this, parent: half the rounds per turn
            side = "this" if turn % 2 == 0 else "parent"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", ROOT if side == "this" else parent_root,
                   "--size", "%d,%d,%d,%d,%d" % ((1 if is3D else 0,) + tuple(dims) + (B,)), "--rounds", str(max(rounds // 2, 1)), "--calls", str(calls)]
            env = dict(os.environ)
            env.pop("TFL_LIBRARY", None)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:
                raise SystemExit("A/B child failed (%s): %s" % (side, r.stderr[-2000:]))
            sides[side] += json.loads(r.stdout.strip().splitlines()[-1])
        out.append({"what": "forward_train + backward, this build | parent build", "grid": "x".join(map(str, dims)), "B": B, "us_per_call": sides})
    return out


def _stat(v):
    import numpy as np
    return float(np.median(v)), float(min(v)), float(max(v))


def accuracy(path):
    """worst rel-L2 per gradient mode, and the witness ratios, from the test's printed lines"""
    pat = re.compile(r"input-grad witness (\S+) (\S+): gradPDiv ours (\S+) PyTorch fp32 (\S+), gradUDiv ours (\S+) PyTorch fp32 (\S+), ratio (\S+)")
    rows = {}
    for line in open(path):
        m = pat.search(line)
        if m:
            name, mode = m.group(1), m.group(2)
            op, tp, ou, tu, ratio = (float(x.rstrip(",")) for x in m.groups()[2:])
            rows.setdefault(mode, []).append((name, op, tp, ou, tu, ratio))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--md", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--accuracy-log", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--size", default=None)
    a = ap.parse_args()
    if a.child:
        s = [int(v) for v in a.size.split(",")]
        return child_backward(a.child, bool(s[0]), tuple(s[1:4]), s[4], a.rounds, a.calls)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("model_input_grad_bench needs an MI355X: nothing is measured without one")
    # (the A/B first: its children each open the GPU on their own, one at a time, before this process does)
    abres = ab(a.parent_root, a.rounds, a.calls) if a.parent_root else []
    res = [measure(is3D, dims, B, a.rounds, a.calls) for is3D, dims, B in SIZES]
    for r in res + abres:
        print(json.dumps(r), flush=True)
    acc = accuracy(a.accuracy_log) if a.accuracy_log else {}
    if not a.md:
        return
    with open(a.md, "w") as fh:
        fh.write("# Input gradients of the projection net (tools/model_input_grad_bench.py)\n\n")
        fh.write("%s, HIP %s. %d rounds of %d calls each, the two sides alternated round by round, device events around a round after "
                 "a synchronise; medians of the rounds with min .. max. No bar was set for the cost: this records what was measured.\n\n"
                 % (res[0]["device"], res[0]["hip"], a.rounds, a.calls))
        fh.write("## 1. forward_train + backward_input against forward_train + backward\n\n"
                 "Both sides get gradP and gradU and write every parameter gradient; backward_input also writes gradPDiv and gradUDiv.\n\n"
                 "| net | backward_input, us per pass | min .. max | backward, us per pass | min .. max | difference |\n|---|---|---|---|---|---|\n")
        for r in res:
            wi, wo = _stat(r["us_per_call"]["backward_input"]), _stat(r["us_per_call"]["backward"])
            fh.write("| %s, B = %d | %.0f | %.0f .. %.0f | %.0f | %.0f .. %.0f | %+.0f us (%+.1f %%) |\n"
                     % (r["grid"], r["B"], wi[0], wi[1], wi[2], wo[0], wo[1], wo[2], wi[0] - wo[0], 100 * (wi[0] / wo[0] - 1)))
        for r in res:
            ki, ko = r["kernel_us_per_pass"]["backward_input"], r["kernel_us_per_pass"]["backward"]
            fh.write("\n%s, B = %d, kernel time per pass from the library's per-kernel event timing (5 passes, every launch of a kernel added "
                     "up; `with input gradients / without`): %s.\n"
                     % (r["grid"], r["B"], ", ".join("%s %.0f / %.0f us" % (k, ki[k], ko.get(k, 0.0)) for k in sorted(ki, key=lambda k: -ki[k]))))
            new = sum(ki.get(k, 0.0) for k in NEW_KERNELS)
            head = sum(ki.get(k, 0.0) for k in HEAD_KERNELS)
            fh.write("The new elementwise kernels (%s) together: %.0f us; k_net_input + k_project + k_bcs_div_stats of the same pass: %.0f us "
                     "(ratio %.2f). k_conv_direct grows by %.0f us (the first layer's data gradient, and the skip's where there is one).\n"
                     % (" + ".join(NEW_KERNELS), new, head, new / max(head, 1e-9), ki.get("k_conv_direct", 0.0) - ko.get("k_conv_direct", 0.0)))
        fh.write("\nThe event timing adds a few microseconds to every kernel it brackets; the per-pass medians above are taken without it.\n")
        if abres:
            fh.write("\n## 2. tfl_model_backward of this build against the parent commit's\n\n"
                     "forward_train + backward, each build in child processes of its own (its own Python package and library), started "
                     "alternately in one session: this, parent, this, parent, %d rounds of %d calls per child.\n\n"
                     "| net | this build, us per pass | min .. max | parent build, us per pass | min .. max | ranges overlap |\n|---|---|---|---|---|---|\n"
                     % (max(a.rounds // 2, 1), a.calls))
            for r in abres:
                t, p = _stat(r["us_per_call"]["this"]), _stat(r["us_per_call"]["parent"])
                fh.write("| %s, B = %d | %.0f | %.0f .. %.0f | %.0f | %.0f .. %.0f | %s |\n"
                         % (r["grid"], r["B"], t[0], t[1], t[2], p[0], p[1], p[2], "yes" if t[1] <= p[2] and p[1] <= t[2] else "NO"))
        if acc:
            fh.write("\n## 3. Accuracy: rel-L2 against float64 autograd of the restatement, %d cases per gradient mode\n\n" % len(next(iter(acc.values()))) +
                     "From tests/test_hip_model_input_grad.py (the bar is 1e-5 for each tensor); the witness is PyTorch-CPU fp32 autograd of "
                     "the same graph, the ratio is our worse tensor over its worse tensor, case by case.\n\n"
                     "| mode | worst gradPDiv (case) | worst gradUDiv (case) | PyTorch fp32 worst gradPDiv | worst gradUDiv | witness ratio, min .. max |\n"
                     "|---|---|---|---|---|---|\n")
            for mode, rows in acc.items():
                wp, wu = max(rows, key=lambda r: r[1]), max(rows, key=lambda r: r[3])
                fh.write("| %s | %.2e (%s) | %.2e (%s) | %.2e | %.2e | %.2f .. %.2f |\n"
                         % (mode, wp[1], wp[0], wu[3], wu[0], max(r[2] for r in rows), max(r[4] for r in rows), min(r[5] for r in rows),
                            max(r[5] for r in rows)))


if __name__ == "__main__":
    main()
