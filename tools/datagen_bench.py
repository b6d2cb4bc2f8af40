"""Times the data-set generator (fluidnet_amd.datagen) at the reference's shapes -- 2-D 128 x 128 and 3-D 64^3 -- and writes
profiles/datagen.md. Per saved frame:
  put_device    one frame pair from the simulation's tensors into a slot (tfl_frames_put_device, all seven tensors, one launch),
                into an HBM slot and into a host-mapped slot
  host route    what it replaces: the seven tensors .cpu() -> data.frame_record -> FrameStore.put (+ flush)
  memcpy D2D    one plain device-to-device copy of the record's byte count
Per step, on the same state (restored from a snapshot before every round; both forms leave the same bits):
  generator     simulate(outputDiv=True) + simulate.project + the two half-puts of a saved step
  two-call      the same without the puts
  plain         one simulate() with simMethod = 'pcg', as the parent commit steps
and one whole run of the paper's recipe (256 steps, every 4th saved; scene set-up included) by the wall clock, as runs per minute.
Protocol of profiles/data_gather.md: one process, the forms alternated round by round, a round = `calls` calls between two
device events after a synchronise, FIVE rounds, the median of the rounds, min .. max beside it. Nothing is asserted but that the
forms agree bit for bit.
--pcgPrecond names the preconditioner of every PCG solve (default 'ic0'; profiles/pcg_mg.md has the 'mg' rows).
--batchRuns R[,R...] measures the generator's batched form instead (generate(batch_runs=R)) and prints one JSON
line per shape: per R the time of one generator step of a wave of R runs (the plans 0 .. R - 1 of the seed, after 8 steps; R = 1:
the serial generator's step, averaged over the plans 0 .. 3) per run, and the runs per minute of the paper's recipe by the wall
clock (generate() of max(R, 4) runs, scene set-up and divergence check included). Nothing is written: profiles/datagen_batched.md
is put together from these lines and those of the same tool at the parent commit, taken in the same session.
usage: python tools/datagen_bench.py [--out profiles/datagen.md] [--calls 20] [--pcgPrecond ic0] [--batchRuns 1,4,16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fluidnet_amd import data, datagen  # noqa: E402
from fluidnet_amd.data import FrameStore, frame_record  # noqa: E402
from fluidnet_amd.simulate import project, simulate  # noqa: E402

ROUNDS = 5
DEV = torch.device("cuda:0")
SEED = 11


def _timed(forms, calls, before=None):
    for _, fn in forms:
        if before:
            before()
        for _ in range(3):
            fn()
    out = {name: [] for name, _ in forms}
    for _ in range(ROUNDS):
        for name, fn in forms:
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return out


def measure(is3D, dims, calls, precond="ic0"):
    g = datagen.default_gconf(is3D, dims, pcgPrecond=precond)
    plan = datagen.plan_run(g, SEED, 0)
    mconf = datagen.mconf_of(plan)
    batch = datagen.init_state(plan, DEV)
    for _ in range(8):
        simulate(None, mconf, batch, None)
    snap = {k: batch[k].clone() for k in ("pDiv", "UDiv", "density")}
    dev_store, host_store = FrameStore(DEV, is3D, *dims, 2, 2), FrameStore(DEV, is3D, *dims, 2, 0)
    nbytes = 4 * dev_store.record_floats
    flat_src, flat_dst = torch.empty(nbytes // 4, device=DEV), torch.empty(nbytes // 4, device=DEV)
    full = dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"], densityDiv=batch["density"], pTarget=batch["pDiv"],
                UTarget=batch["UDiv"], densityTarget=batch["density"])

    def host_route():
        h = {k: v.cpu().numpy() for k, v in full.items()}
        rec = frame_record(((h["pTarget"], h["UTarget"], h["flags"], h["densityTarget"], is3D),
                            (h["pDiv"], h["UDiv"], h["flags"], h["densityDiv"], is3D)))
        dev_store.put(1, rec)
        dev_store.flush()

    def restore():
        for k, v in snap.items():
            batch[k].copy_(v)

    def generator_step():
        simulate(None, mconf, batch, None, outputDiv=True)
        dev_store.put_device([0], dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"], densityDiv=batch["density"]))
        project(None, mconf, batch)
        dev_store.put_device([0], dict(pTarget=batch["pDiv"], UTarget=batch["UDiv"], densityTarget=batch["density"]))

    def two_call_step():
        simulate(None, mconf, batch, None, outputDiv=True)
        project(None, mconf, batch)

    try:
        frame = _timed([("put_device_hbm", lambda: dev_store.put_device([0], full)),
                        ("put_device_host_mapped", lambda: host_store.put_device([0], full)),
                        ("host_route", host_route),
                        ("memcpy_d2d", lambda: flat_dst.copy_(flat_src, non_blocking=True))], calls)
        # put_device leaves what the host route leaves
        a = {k: torch.empty_like(v) for k, v in full.items()}
        b = {k: torch.empty_like(v) for k, v in full.items()}
        dev_store.gather([0], a)
        dev_store.gather([1], b)
        assert all(torch.equal(a[k], b[k]) for k in a)
        step = _timed([("generator_step", generator_step), ("two_call_step", two_call_step),
                       ("plain_step", lambda: simulate(None, mconf, batch, None))], max(calls // 2, 4), before=restore)
        ends = {}
        for name, fn in (("generator", generator_step), ("plain", lambda: simulate(None, mconf, batch, None))):
            restore()
            for _ in range(4):
                fn()
            ends[name] = {k: batch[k].clone() for k in snap}
        assert all(torch.equal(ends["generator"][k], ends["plain"][k]) for k in snap)
        # one whole run of the paper's recipe, scene set-up included
        store = FrameStore(DEV, is3D, *dims, len(datagen.saved_steps(g)), len(datagen.saved_steps(g)))
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = datagen.run_frames(plan, g, store, 0, DEV)
            max_div = data.max_target_divergence(store, is3D, dims, 0, n)
            torch.cuda.synchronize()
            run_s = time.perf_counter() - t0
        finally:
            store.close()
    finally:
        torch.cuda.synchronize()
        dev_store.close()
        host_store.close()
    med = lambda t: {k: float(np.median(v)) for k, v in t.items()}
    rng = lambda t: {k: [float(min(v)), float(max(v))] for k, v in t.items()}
    return dict(shape="%s %s" % ("3-D" if is3D else "2-D", "x".join(str(d) for d in dims)), record_bytes=nbytes, calls_per_round=calls,
                frame_us=med(frame), frame_us_min_max=rng(frame), step_us=med(step), step_us_min_max=rng(step),
                run_seconds=run_s, run_frames=n, run_max_div=max_div, runs_per_minute=60.0 / run_s,
                plan=dict(obstacles=len(plan["obstacles"]), blobs=len(plan["blobs"]), emitters=len(plan["emitters"]),
                          buoyancyScale=plan["buoyancyScale"], vorticityConfinementAmp=plan["vorticityConfinementAmp"]))


def measure_batched(is3D, dims, calls, precond, batch_runs, steps=256):
    """per R: us of one generator step per run (median of ROUNDS, min .. max), and runs per minute of generate()"""
    g = datagen.default_gconf(is3D, dims, pcgPrecond=precond, divThreshold=None, steps=steps)
    frames = len(datagen.saved_steps(g))
    out = dict(shape="%s %s" % ("3-D" if is3D else "2-D", "x".join(str(d) for d in dims)), pcgPrecond=precond, calls_per_round=calls, R={})
    for R in batch_runs:
        plans = [datagen.plan_run(g, SEED, r) for r in range(max(R, 4) if R == 1 else R)]
        store = FrameStore(DEV, is3D, *dims, max(R, 4), max(R, 4))
        try:
            if R == 1:
                runs = []
                for plan in plans:
                    mconf, batch = datagen.mconf_of(plan), datagen.init_state(plan, DEV)
                    for _ in range(8):
                        simulate(None, mconf, batch, None)
                    runs.append((mconf, batch, {k: batch[k].clone() for k in ("pDiv", "UDiv", "density")}))

                def restore():
                    for _, batch, snap in runs:
                        for k, v in snap.items():
                            batch[k].copy_(v)

                def step():      # one generator step of each of the four runs
                    for mconf, batch, _ in runs:
                        simulate(None, mconf, batch, None, outputDiv=True)
                        store.put_device([0], dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"], densityDiv=batch["density"]))
                        project(None, mconf, batch)
                        store.put_device([0], dict(pTarget=batch["pDiv"], UTarget=batch["UDiv"], densityTarget=batch["density"]))
                per = len(runs)
            else:
                from fluidnet_amd.simulate import project_items, simulate_items
                batch, mconf, forces = datagen.init_wave(plans, DEV)
                for _ in range(8):
                    simulate_items(None, mconf, batch, forces)
                snap = {k: batch[k].clone() for k in ("pDiv", "UDiv", "density")}
                slots = list(range(R))

                def restore():
                    for k, v in snap.items():
                        batch[k].copy_(v)

                def step():
                    simulate_items(None, mconf, batch, forces, outputDiv=True)
                    store.put_device(slots, dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"], densityDiv=batch["density"]))
                    project_items(None, mconf, batch, forces)
                    store.put_device(slots, dict(pTarget=batch["pDiv"], UTarget=batch["UDiv"], densityTarget=batch["density"]))
                per = R
            t = _timed([("step", step)], max(calls // 2, 4), before=restore)["step"]
        finally:
            torch.cuda.synchronize()
            store.close()
        nruns = max(R, 4)
        big = FrameStore(DEV, is3D, *dims, nruns * frames, nruns * frames)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = datagen.generate(g, "tr", nruns, SEED, store=big, device=DEV, **({} if R == 1 else dict(batch_runs=R)))
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            big.close()
        out["R"][str(R)] = dict(step_us_per_run=float(np.median(t)) / per, step_us_per_run_min_max=[min(t) / per, max(t) / per],
                                wave_step_us=float(np.median(t)), runs=nruns, seconds=wall, runs_per_minute=60.0 * nruns / wall,
                                worst_max_div=max(r["max_div"] for r in res["report"]))
    return out


def report(results, path, oracle_lines, precond="ic0"):
    f3 = lambda r, t, k: "%.1f (%.1f .. %.1f)" % (r[t][k], r[t + "_min_max"][k][0], r[t + "_min_max"][k][1])
    lines = ["# The data-set generator (tools/datagen_bench.py)", "",
             "%s, HIP %s. pcgPrecond = '%s'. %d rounds, the forms alternated round by round, device events around a round after a synchronise; medians "
             "of the rounds, min .. max beside them. Every figure below comes from this one run on the device named here."
             % (torch.cuda.get_device_name(0), torch.version.hip, precond, ROUNDS), "",
             "## One saved frame pair into the store", "",
             "| shape | record bytes | put_device, HBM slot us | put_device, host-mapped slot us | host route us | memcpy D2D us | put_device / D2D | host route / put_device |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s | %d | %s | %s | %s | %s | %.2f | %.1f |" % (
            r["shape"], r["record_bytes"], f3(r, "frame_us", "put_device_hbm"), f3(r, "frame_us", "put_device_host_mapped"),
            f3(r, "frame_us", "host_route"), f3(r, "frame_us", "memcpy_d2d"), r["frame_us"]["put_device_hbm"] / r["frame_us"]["memcpy_d2d"],
            r["frame_us"]["host_route"] / r["frame_us"]["put_device_hbm"]))
    lines += ["", "put_device: ONE call with all seven tensors of one item (the generator makes two calls of four and three). host route: "
              "the seven tensors `.cpu()`, `data.frame_record`, `FrameStore.put`, `flush`. memcpy D2D: one `copy_` of the record's bytes. "
              "Where put_device into an HBM slot takes the same time at both shapes although the records differ 20-fold in size, the "
              "supposition is that the call is bound by its host side (seven descriptors, seven pointer queries, one launch) and not "
              "by the device's copy rate; the host side has not been timed on its own.", "",
              "## One step", "",
              "| shape | generator step us | two-call step us | plain simulate(pcg) us | two-call - plain us | generator - two-call us (the puts) |",
              "|---|---|---|---|---|---|"]
    for r in results:
        s = r["step_us"]
        lines.append("| %s | %s | %s | %s | %.1f | %.1f |" % (r["shape"], f3(r, "step_us", "generator_step"), f3(r, "step_us", "two_call_step"),
                                                            f3(r, "step_us", "plain_step"), s["two_call_step"] - s["plain_step"],
                                                            s["generator_step"] - s["two_call_step"]))
    lines += ["", "generator step: `simulate(outputDiv=True)`, the half-put of the divergent frame, `simulate.project`, the half-put of the "
              "target frame. two-call: the same without the puts. plain: one `simulate()`. All three start every round from the same "
              "snapshot and leave equal bits (checked in the run). Almost all of a step is the PCG solve (maxIter 100, the preconditioner named above, a host "
              "read of the residual per solve), which the three forms share; where `two-call - plain` is smaller than the forms' own "
              "min .. max it is not a cost that this run can show. Where it is larger, no measurement here says where it goes. What "
              "the two-call form does more than the plain step, and so the supposed cause: a second host entry per step (`project` "
              "builds the native step's argument structures, asks for the workspace size and validates again). With `simMethod = "
              "'pcg'` the two forms enqueue the same sequence of operators: the solver path folds no setConstVals into a force kernel.", "",
              "## One run of the paper's recipe (256 steps, every 4th saved), wall clock, scene set-up and divergence check included", "",
              "| shape | seconds | frame pairs | max div(U target) | runs per minute | the plan |", "|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s | %.2f | %d | %.3e | %.1f | %s |" % (r["shape"], r["run_seconds"], r["run_frames"], r["run_max_div"],
                                                               r["runs_per_minute"], json.dumps(r["plan"])))
    lines += ["", "## The plans of the tests and the loader's divergence threshold", ""] + oracle_lines
    lines += ["", "Not measured: a set larger than HBM (host-mapped slots under the generator's write pattern at scale), scenes with "
              "voxel models, and anything on more than one GPU."]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def device_figures_of_the_test_plans(precond="ic0"):
    """max div(U target) of the runs tests/test_hip_datagen.py generates, on the device (the CPU figures are in the test's output)"""
    out = []
    for is3D, dims in ((False, (1, 32, 32)), (True, (12, 16, 20))):
        g = datagen.default_gconf(is3D, dims, steps=12, saveEvery=2, pcgPrecond=precond)
        store = FrameStore(DEV, is3D, *dims, 12, 12)
        try:
            res = datagen.generate(g, "tr", 2, SEED, store=store, device=DEV)
        finally:
            store.close()
        out.append((dims, [r["max_div"] for r in res["report"]], all(r["kept"] for r in res["report"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/datagen.md with 'ic0'; required with another preconditioner")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pcgPrecond", default="ic0", choices=("none", "ilu0", "ic0", "mg"))
    ap.add_argument("--batchRuns", default=None, help="R[,R...]: measure generate(batch_runs=R) instead (1 = the serial generator); prints JSON lines")
    ap.add_argument("--steps", type=int, default=256, help="with --batchRuns: steps per run of the wall-clock figure")
    a = ap.parse_args()
    if a.batchRuns is not None:
        if not torch.cuda.is_available():
            raise SystemExit("datagen_bench needs an MI355X: nothing is measured without one")
        for is3D, dims in ((False, (1, 128, 128)), (True, (64, 64, 64))):
            print(json.dumps(measure_batched(is3D, dims, a.calls, a.pcgPrecond, [int(v) for v in a.batchRuns.split(",")], a.steps)), flush=True)
        return
    if a.out is None:
        if a.pcgPrecond != "ic0":
            ap.error("--out is required with --pcgPrecond %s: profiles/datagen.md is the record of the 'ic0' run" % a.pcgPrecond)
        a.out = os.path.join(ROOT, "profiles", "datagen.md")
    if not torch.cuda.is_available():
        raise SystemExit("datagen_bench needs an MI355X: nothing is measured without one")
    results = []
    for is3D, dims in ((False, (1, 128, 128)), (True, (64, 64, 64))):
        r = measure(is3D, dims, a.calls, a.pcgPrecond)
        print(json.dumps(r), flush=True)
        results.append(r)
    oracle_lines = ["`tests/test_hip_datagen.py` generates 2 runs x 6 saved frames (seed %d, 12 steps, every 2nd saved) at 1x32x32 and 12x16x20 and "
                    "requires that no run is dropped by `data.DIV_THRESHOLD` = %g. The signed maximum of div(U target) per run on the device, "
                    "in this run (the CPU figures of the same plans, from the oracle's operators, are printed by "
                    "`pytest tests/test_datagen_cpu.py -s` and are not repeated by this tool):" % (SEED, data.DIV_THRESHOLD), ""]
    for dims, divs, kept in device_figures_of_the_test_plans(a.pcgPrecond):
        oracle_lines.append("* %s: %s, %s" % ("x".join(str(d) for d in dims), ", ".join("%.3e" % d for d in divs), "all kept" if kept else "A RUN WAS DROPPED"))
    report(results, a.out, oracle_lines, a.pcgPrecond)


if __name__ == "__main__":
    main()
