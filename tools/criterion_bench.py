"""Times the fused criterion (criterion.hip: k_criterion_planes + k_criterion_finish behind tfl_fluidCriterion) against the
composition a caller had before it: torch element-wise operations + velocityDivergenceForward / velocityDivergenceBackward +
three .sum()s. 128^3, B = 1, weighted (borderWeight 2, borderWidth 3), all three lambdas on, with gradients; the weight is
precomputed for both. One process; the two are alternated round by round; each round is `calls` calls between two device
events after a synchronise. Prints one JSON line and, with --md, writes the record kept as profiles/criterion.md.
usage: python tools/criterion_bench.py [--size 128] [--rounds 10] [--calls 50] [--md PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
from fluidnet_amd import tfluids  # noqa: E402

HBM_PEAK_GBS = 8000.0         # HBM3E, 8.0 TB/s spec
BYTES_PER_CELL = 56           # reads p, pTarget, flags, weight (16) + U, UTarget (24); writes gradP (4) + gradU (12)
LAMBDAS = (0.7, 1.3, 2.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("criterion_bench needs an MI355X: nothing is measured without one")
    dev = torch.device("cuda:0")
    n = a.size
    sa = scenes.make_scene((n, n, n), seed=5, vel_cells=0.4)
    sb = scenes.make_scene((n, n, n), seed=6, vel_cells=0.4)
    pP, UP, flags = (torch.from_numpy(sa[k]).to(dev) for k in ("p", "U", "flags"))
    pT, UT = (torch.from_numpy(sb[k]).to(dev) for k in ("p", "U"))
    w = tfluids.criterionWeight(flags, 3, 2.0)
    loss = torch.zeros(4, dtype=torch.float64, device=dev)
    gP, gU = torch.empty_like(pP), torch.empty_like(UP)
    lp, lu, ld = LAMBDAS
    n_p, n_u = float(pP.numel()), float(UP.numel())
    div, dU = torch.empty_like(flags), torch.empty_like(UP)

    def fused():
        tfluids.fluidCriterion(pP, UP, pT, UT, flags, w, lp, lu, ld, True, loss, gP, gU)
        return loss, gP, gU

    def composed():
        zp = w * pP - w * pT
        l_p = lp * ((zp * zp).sum() / n_p)
        g_p = ((2.0 / n_p) * zp) * w * lp
        zu = w * UP - w * UT
        l_u = lu * ((zu * zu).sum() / n_u)
        g_u = ((2.0 / n_u) * zu) * w * lu
        tfluids.velocityDivergenceForward(UP, flags, div)
        zd = w * div
        l_d = ld * ((zd * zd).sum() / n_p)
        go = ((2.0 / n_p) * zd) * w * ld
        tfluids.velocityDivergenceBackward(UP, flags, go, dU)
        g_u = g_u + dU
        return torch.stack([l_p, l_u, l_d, l_p + l_u + l_d]), g_p, g_u

    def rel(x, y):
        return float((x.double() - y.double()).norm() / y.double().norm())
    for _ in range(3):
        f, c = fused(), composed()
    agree = {"loss": rel(f[0], c[0].double()), "gradP": rel(f[1], c[1]), "gradU": rel(f[2], c[2])}
    assert max(agree.values()) < 1e-5, agree       # the two compute the same thing (fp32 sums on the composed side)
    times = {"fused": [], "composed": []}
    for _ in range(a.rounds):
        for name, fn in (("fused", fused), ("composed", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
    with tfluids.profile(pP) as prof:
        for _ in range(10):
            fused()
    kern = {k: v["ms"] / v["calls"] * 1e3 for k, v in prof.kernels.items()}
    cells = float(n) ** 3
    med = {k: float(np.median(v)) for k, v in times.items()}
    planes_us = kern["k_criterion_planes"]
    res = {"what": "fluidCriterion, weighted, three lambdas, with gradients", "grid": "%d^3" % n, "device": torch.cuda.get_device_name(0),
           "hip": torch.version.hip, "rounds": a.rounds, "calls_per_round": a.calls, "us_per_call_median": med,
           "us_per_call_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()}, "kernel_us": kern,
           "bytes_per_cell": BYTES_PER_CELL, "k_criterion_planes_GBps": BYTES_PER_CELL * cells / planes_us / 1e3,
           "k_criterion_planes_frac_of_hbm_peak": BYTES_PER_CELL * cells / planes_us / 1e3 / HBM_PEAK_GBS,
           "fused_over_composed": med["fused"] / med["composed"], "agreement_rel_l2": agree}
    print(json.dumps(res), flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("# Fused criterion against the composed one (tools/criterion_bench.py)\n\n")
            fh.write("%s, HIP %s. Grid %s, B = 1, weighted (borderWeight 2, borderWidth 3), lambdas %s, sizeAverage, with gradients; "
                     "the weight is precomputed for both.\n%d rounds of %d calls each, the two alternated round by round, device "
                     "events around a round after a synchronise.\n\n" % (res["device"], res["hip"], res["grid"], LAMBDAS, a.rounds, a.calls))
            fh.write("| | us per call (median of rounds) | min .. max |\n|---|---|---|\n")
            fh.write("| (a) tfl_fluidCriterion: k_criterion_planes + k_criterion_finish | %.1f | %.1f .. %.1f |\n" % (med["fused"], min(times["fused"]), max(times["fused"])))
            fh.write("| (b) torch element-wise + velocityDivergenceForward / Backward + three .sum()s | %.1f | %.1f .. %.1f |\n\n" % (med["composed"], min(times["composed"]), max(times["composed"])))
            fh.write("(a) / (b) = %.3f. The two agree to rel-L2 %.1e (loss), %.1e (gradP), %.1e (gradU).\n\n" % (res["fused_over_composed"], agree["loss"], agree["gradP"], agree["gradU"]))
            fh.write("Kernel time from the library's per-kernel event timing (10 calls): " + ", ".join("%s %.1f us" % kv for kv in sorted(kern.items())) + ".\n")
            fh.write("Algorithmic traffic of k_criterion_planes: %d B/cell (reads p, pTarget, flags, weight 16 B and U, UTarget 24 B; writes gradP 4 B and "
                     "gradU 12 B) = %.1f MB per call: %.0f GB/s, %.1f %% of the 8.0 TB/s HBM peak, the bound such a streaming pass would have. The -y / -z "
                     "neighbour rows the gradient recomputes are not in this count; whether they are served from cache was not measured "
                     "(no counter pass was taken).\n" % (BYTES_PER_CELL, BYTES_PER_CELL * cells / 1e6, res["k_criterion_planes_GBps"], 100 * res["k_criterion_planes_frac_of_hbm_peak"]))
            fh.write("One block per (batch item, z-plane): %d blocks of 1024 threads on this grid, fewer than the chip has compute units; "
                     "presumably that, not HBM, is what limits the kernel here -- not measured.\n" % n)


if __name__ == "__main__":
    main()
