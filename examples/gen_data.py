#!/usr/bin/env python
"""examples/gen_data.py -- generate a training set for examples/train.py on the MI355X (fluidnet_amd.datagen).

Writes <out>/<dataset>/{tr,te}/<run %06d>/<frame %06d>.bin + <frame %06d>_divergent.bin, the layout fluidnet_amd.data.DataBinary
(torch/lib/data_binary.lua) reads: random scenes -- sphere, box and optional binvox obstacles, density blobs and emitters, a
divergence-free noise velocity, random gravity direction, buoyancy and vorticity confinement -- stepped with the PCG projection,
every --save-every-th step one frame pair. The scenes are this project's own; they are NOT the reference's Mantaflow scenes.

  python examples/gen_data.py --out data/datasets --dataset my_set --dim 2 --res 128 --runs-tr 320 --runs-te 320 \\
        [--steps 256] [--save-every 4] [--seed 1] [--models a.binvox b.binvox] [--pcgPrecond mg --batchRuns 16]
  python examples/train.py --dataDir data/datasets --dataset my_set --out /tmp/fit/model
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidnet_amd import datagen, io  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="conf.dataDir: the directory the data set's directory is made in")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--dim", type=int, choices=(2, 3), default=2)
    ap.add_argument("--res", type=int, default=None, help="cells per axis (default 128 in 2-D, 64 in 3-D)")
    ap.add_argument("--runs-tr", type=int, default=320)
    ap.add_argument("--runs-te", type=int, default=320)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--save-every", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--models", nargs="*", default=[], help="binvox files stamped into 3-D scenes as obstacles")
    ap.add_argument("--pcgPrecond", default="ic0", choices=("none", "ilu0", "ic0", "mg"), help="preconditioner of the PCG solves")
    ap.add_argument("--batchRuns", type=int, default=1, help="runs stepped at a time as the items of one batch (1 .. 32; the same set either "
                    "way). It pays where a step is launch-bound: small grids with --pcgPrecond mg | none")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    is3D = a.dim == 3
    res = a.res or (64 if is3D else 128)
    models = [io.loadVoxelData(fn)["data"] for fn in a.models]
    gconf = datagen.default_gconf(is3D, (res if is3D else 1, res, res), steps=a.steps, saveEvery=a.save_every, models=models, pcgPrecond=a.pcgPrecond)
    out = os.path.join(a.out, a.dataset)
    first = 0
    for prefix, nruns in (("tr", a.runs_tr), ("te", a.runs_te)):
        if nruns <= 0:
            continue
        # the test set's runs carry on from the training set's numbers: no scene appears in both
        res_ = datagen.generate(gconf, prefix, nruns, a.seed, out_dir=out, device=a.device, first_run=first, batch_runs=a.batchRuns)
        first += nruns
        again = [r for r in res_["report"] if not r["kept"]]
        print("==> %s: %d runs of %d frame pairs in %s; worst max(div) kept %.3e; %d attempts regenerated"
              % (prefix, len(res_["runs"]), res_["runs"][0][1], os.path.join(out, prefix),
                 max(r["max_div"] for r in res_["report"] if r["kept"]), len(again)))


if __name__ == "__main__":
    main()
