"""Times a mini-batch of the resident frame store (tfl_frames_gather, fluidnet_amd.data.FrameStore) against the obvious
alternatives it replaces, at the reference's shapes -- 2-D 128 x 128 with B = 16 and 64, 3-D 64^3 with B = 16 -- and writes
profiles/data_gather.md. Forms, each filling the same seven batch tensors from randomly drawn frames:
  (a)        the one-launch gather, every slot device-resident
  (b)        the same gather, every slot in pinned, device-mapped host memory
  (c)-device torch.index_select(frames, 0, idx, out=batch) per tensor from device-resident frame tensors: the index upload and
             seven launches
  (c)-host   hipMemcpyAsync from pinned host memory into the batch: one copy per plane (2 C + 5 per item), and -- a stricter
             yardstick, since the C velocity planes of an item are contiguous on both sides -- one copy per tensor and item (7)
and, in the same run, a plain hipMemcpyAsync of the batch's byte count, device to device and pinned host to device: (a) and (b)
are stated as fractions of those two rates. Then one closure call (run_epoch.Closure, four future steps) on a gathered batch,
for the gather's share of a training iteration.
Protocol of profiles/model_backward.md: one process, the forms alternated round by round, a round = `calls` mini-batches between
two device events after a synchronise, FIVE rounds, the median of the rounds; the spread of a form is max - min of its five.
THE ONE CONDITION: the tool fails (exit status 1) if (a) is slower than (c)-device or (b) slower than the faster (c)-host form by
more than the run's own spread (the larger of the two forms' spreads). (c) is the yardstick, not the code under test.
usage: python tools/data_gather_bench.py [--out profiles/data_gather.md] [--calls 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fluidnet_amd import FluidCriterion, FluidNetModel, ProjectionNet, optim, tfluids  # noqa: E402
from fluidnet_amd.data import FrameStore  # noqa: E402
from fluidnet_amd.run_epoch import Closure  # noqa: E402

ROUNDS = 5
KEYS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")
DEV = torch.device("cuda:0")


def _frames(is3D, dims, n, seed):
    """n records [2 C + 5][cells] (cells a multiple of 4 at these shapes): small velocities over an empty domain"""
    rng = np.random.RandomState(seed)
    C, cells = (3 if is3D else 2), dims[0] * dims[1] * dims[2]
    flags = torch.empty(1, 1, *dims, device=DEV)
    tfluids.emptyDomain(flags, is3D)
    rec = (rng.randn(n, 2 * C + 5, cells) * 0.05).astype(np.float32)
    rec[:, C + 1] = flags.cpu().numpy().reshape(-1)
    return rec


def _timed(forms, calls):
    """{name: [us per call, one figure per round]}: the forms alternated round by round"""
    for _, fn in forms:
        for i in range(3):
            fn(i)
    out = {name: [] for name, _ in forms}
    k = 0
    for _ in range(ROUNDS):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(calls):
                fn(k + i)
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / calls * 1e3)
        k += calls
    return out


def measure(is3D, dims, B, nframes, calls, with_closure):
    C, cells = (3 if is3D else 2), dims[0] * dims[1] * dims[2]
    chans = {k: (C if k in ("UDiv", "UTarget") else 1) for k in KEYS}
    first = dict(zip(KEYS, np.cumsum([0] + [chans[k] for k in KEYS[:-1]])))
    rec = _frames(is3D, dims, nframes, seed=cells % 97 + B)
    stores = {"device": FrameStore(DEV, is3D, *dims, nframes, nframes), "host": FrameStore(DEV, is3D, *dims, nframes, 0)}
    for st in stores.values():
        for s in range(nframes):
            st.put(s, rec[s])
        st.flush()
    # the yardstick's frames: one tensor per output, [nframes][chans][Z][Y][X], on the device and in pinned host memory
    host = {k: torch.from_numpy(rec[:, first[k]:first[k] + chans[k]].reshape(nframes, chans[k], *dims).copy()).pin_memory() for k in KEYS}
    devt = {k: v.to(DEV) for k, v in host.items()}
    batch = {k: torch.zeros(B, chans[k], *dims, device=DEV) for k in KEYS}
    draws = np.random.RandomState(5).randint(0, nframes, size=(64, B))
    nbytes = 4 * B * (2 * C + 5) * cells
    flat_src, flat_dst = torch.empty(nbytes // 4, device=DEV), torch.empty(nbytes // 4, device=DEV)
    flat_pin = torch.empty(nbytes // 4).pin_memory()

    def ids(i):
        return draws[i % len(draws)].tolist()

    def c_device(i):
        idx = torch.tensor(ids(i), dtype=torch.int64).to(DEV, non_blocking=True)
        for k in KEYS:
            torch.index_select(devt[k], 0, idx, out=batch[k])

    def c_host_planes(i):
        for b, s in enumerate(ids(i)):
            for k in KEYS:
                for c in range(chans[k]):
                    batch[k][b, c].copy_(host[k][s, c], non_blocking=True)

    def c_host_tensors(i):
        for b, s in enumerate(ids(i)):
            for k in KEYS:
                batch[k][b].copy_(host[k][s], non_blocking=True)

    forms = [("a_gather_device", lambda i: stores["device"].gather(ids(i), batch)),
             ("b_gather_host", lambda i: stores["host"].gather(ids(i), batch)),
             ("c_device_index_select", c_device),
             ("c_host_copy_per_plane", c_host_planes),
             ("c_host_copy_per_tensor", c_host_tensors),
             ("memcpy_d2d", lambda i: flat_dst.copy_(flat_src, non_blocking=True)),
             ("memcpy_h2d", lambda i: flat_dst.copy_(flat_pin, non_blocking=True))]
    try:
        us = _timed(forms, calls)
        # both gathers deliver what the yardstick delivers
        want = {k: devt[k][ids(0)] for k in KEYS}
        for name in ("device", "host"):
            stores[name].gather(ids(0), batch)
            assert all(torch.equal(batch[k], want[k]) for k in KEYS), name
        closure_us = None
        if with_closure:
            mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=0, gravityScale=0,
                         vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], simMethod="convnet", trainTargetSource="manta",
                         lossPLambda=0, lossULambda=1.0, lossDivLambda=1.0, longTermDivLambda=0.25, longTermDivNumSteps=[4, 16],
                         longTermDivProbability=0.9, timeScaleSigma=1, optimizationMethod="adam", gradNormThreshold=1,
                         optimState=dict(learningRate=0.0025, epsilon=0.0001, beta1=0.9, beta2=0.999))
            net = ProjectionNet(FluidNetModel.from_mconf(dict(modelType="default"), is3D, seed=1), device=DEV).train()
            closure = Closure(net, FluidCriterion(0, 1.0, 1.0), optim.from_mconf(net, mconf), None, mconf)
            plan = dict(buoyancyScale=0, gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0], dt=0.1, numFutureSteps=4)

            def iteration(i):
                stores["device"].gather(ids(i), batch)
                closure(batch, plan)
            t = _timed([("gather_and_closure", iteration)], max(calls // 4, 2))
            closure_us = t["gather_and_closure"]
    finally:
        torch.cuda.synchronize()
        for st in stores.values():
            st.close()
    med = {k: float(np.median(v)) for k, v in us.items()}
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    c_host = min(("c_host_copy_per_plane", "c_host_copy_per_tensor"), key=lambda k: med[k])
    verdict = {
        "a_vs_c_device": dict(a=med["a_gather_device"], c=med["c_device_index_select"],
                              margin=max(spread["a_gather_device"], spread["c_device_index_select"])),
        "b_vs_c_host": dict(b=med["b_gather_host"], c=med[c_host], c_form=c_host, margin=max(spread["b_gather_host"], spread[c_host])),
    }
    verdict["a_vs_c_device"]["ok"] = verdict["a_vs_c_device"]["a"] <= verdict["a_vs_c_device"]["c"] + verdict["a_vs_c_device"]["margin"]
    verdict["b_vs_c_host"]["ok"] = verdict["b_vs_c_host"]["b"] <= verdict["b_vs_c_host"]["c"] + verdict["b_vs_c_host"]["margin"]
    out = dict(shape="%s %s, B = %d" % ("3-D" if is3D else "2-D", "x".join(str(d) for d in dims), B), bytes=nbytes, frames=nframes,
               calls_per_round=calls, rounds=ROUNDS, us_median=med, us_min_max={k: [float(min(v)), float(max(v))] for k, v in us.items()},
               spread_us=spread, gb_per_s={k: nbytes / med[k] * 1e-3 for k in med},
               a_fraction_of_d2d_rate=med["memcpy_d2d"] / med["a_gather_device"],
               b_fraction_of_h2d_rate=med["memcpy_h2d"] / med["b_gather_host"], verdict=verdict)
    if closure_us is not None:
        it = float(np.median(closure_us))
        out["iteration_us_median"] = it
        out["gather_share_of_iteration"] = med["a_gather_device"] / it
    return out


def report(results, path):
    lines = ["# One mini-batch from the resident frame store (tools/data_gather_bench.py)", "",
             "%s, HIP %s. %d rounds of %d mini-batches each, the forms alternated round by round, device events around a round after "
             "a synchronise; medians of the rounds, min .. max beside them. The frames of a batch are drawn at random from %s; all "
             "forms fill the same seven batch tensors, and both gathers are checked against the yardstick's result in the run."
             % (torch.cuda.get_device_name(0), torch.version.hip, ROUNDS, results[0]["calls_per_round"],
                " / ".join("%d" % r["frames"] for r in results) + " resident frames"), "",
             "(a) tfl_frames_gather, slots in HBM. (b) the same launch, slots in pinned device-mapped host memory. (c)-device: "
             "torch.index_select(out=) per tensor from device-resident frame tensors (index upload + 7 launches). (c)-host: "
             "hipMemcpyAsync from pinned host memory, one per plane / one per tensor and item. memcpy: ONE hipMemcpyAsync of the "
             "batch's byte count.", "",
             "| shape | bytes | (a) us | (b) us | (c)-device us | (c)-host per plane us | (c)-host per tensor us | memcpy D2D us | memcpy H2D us |",
             "|---|---|---|---|---|---|---|---|---|"]
    cols = ("a_gather_device", "b_gather_host", "c_device_index_select", "c_host_copy_per_plane", "c_host_copy_per_tensor", "memcpy_d2d", "memcpy_h2d")
    for r in results:
        lines.append("| %s | %d | " % (r["shape"], r["bytes"]) +
                     " | ".join("%.1f (%.1f .. %.1f)" % (r["us_median"][c], r["us_min_max"][c][0], r["us_min_max"][c][1]) for c in cols) + " |")
    lines += ["", "| shape | (a) GB/s | (a) / D2D memcpy rate | (b) GB/s | (b) / H2D memcpy rate | (a) over (c)-device | (b) over faster (c)-host |", "|---|---|---|---|---|---|---|"]
    for r in results:
        v = r["verdict"]
        lines.append("| %s | %.0f | %.2f | %.1f | %.2f | %.2f (margin %.1f us: %s) | %.2f (margin %.1f us: %s) |"
                     % (r["shape"], r["gb_per_s"]["a_gather_device"], r["a_fraction_of_d2d_rate"], r["gb_per_s"]["b_gather_host"],
                        r["b_fraction_of_h2d_rate"], v["a_vs_c_device"]["a"] / v["a_vs_c_device"]["c"], v["a_vs_c_device"]["margin"],
                        "ok" if v["a_vs_c_device"]["ok"] else "SLOWER", v["b_vs_c_host"]["b"] / v["b_vs_c_host"]["c"],
                        v["b_vs_c_host"]["margin"], "ok" if v["b_vs_c_host"]["ok"] else "SLOWER"))
    lines += ["", "GB/s counts the bytes written into the batch once (the same number are read). The condition of the tool: (a) not "
              "slower than (c)-device and (b) not slower than the faster (c)-host form, by more than the larger of the two forms' max - min "
              "over the five rounds.", ""]
    for r in results:
        if "iteration_us_median" in r:
            lines.append("%s: one iteration (gather + run_epoch.Closure with the default net, four future steps, Adam) %.0f us; the "
                         "gather (a) is %.2f %% of it." % (r["shape"], r["iteration_us_median"], 100 * r["gather_share_of_iteration"]))
    lines += ["", "Not measured: a store partly in HBM and partly on the host under a real epoch's access pattern, host-mapped reads "
              "while another process loads the host link, and anything on more than one GPU."]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_gather.md"))
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_gather_bench needs an MI355X: nothing is measured without one")
    results = []
    for is3D, dims, B, nframes, with_closure in ((False, (1, 128, 128), 16, 512, True), (False, (1, 128, 128), 64, 512, False),
                                                 (True, (64, 64, 64), 16, 48, True)):
        r = measure(is3D, dims, B, nframes, a.calls, with_closure)
        print(json.dumps(r), flush=True)
        results.append(r)
    report(results, a.out)
    bad = [(r["shape"], k) for r in results for k, v in r["verdict"].items() if not v["ok"]]
    if bad:
        print("FAILED: slower than the yardstick: %s" % bad, file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
