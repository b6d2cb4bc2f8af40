"""Helper of tests/test_hip_scal3_scan_fold.py: own process, because the library (TFL_LIBRARY) and the switches TFL_SCAL3_SPARSE,
TFL_VEL3_KZ and TFL_SCAL3_SEQ0 are chosen once per process. usage: scal3_scan_fold_run.py <out.json> <part> [<part> ...]; every part
steps scenes through tfl_simulate_step and records what tests/scal3_sparse_run.py records (digests of density / UDiv / pDiv, the
trace-error count, tfl_scal3_sparse_stats).
  scenes   the scenes of SCENES below: the brick scan as a by-product of pass A of advectVel
  stale    scal3_sparse_run's: the step's workspace pre-filled with NaN, then with 1e30
  sim      scal3_sparse_run's: twelve steps of the 48^3 plume, step by step
  graph    scal3_sparse_run's: the captured step against the eager one
  kernels  the launches of one profiled step, by timer name: one density channel, then two"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scal3_sparse_run as R  # noqa: E402
from scenes import OBSTACLE  # noqa: E402

# (Z, Y, X). g70 / g130: no extent a multiple of the brick (4, 4, 64) or of 4 -- a partial last brick on every axis, unaligned rows,
# an odd Z (the two-plane pass A ends on a one-plane group); g130s: 5 x 5 x 3 bricks; g72: X % 4 == 0 (the four-cell stand-alone scan)
GRIDS = {"g70": (11, 13, 70), "g130": (12, 12, 130), "g130s": (20, 20, 130), "g72": (10, 9, 72)}
BLOB = (slice(1, 3), slice(1, 3), slice(3, 6))      # smoke in the corner brick: its ring is 2 x 2 x 2 bricks on every grid


def fast_places(dims):
    """(name, component, (k, j, i)) of the one velocity word put at / above the bound"""
    Z, Y, X = dims
    return [("c0", 0, (Z // 2 + 1, Y // 2 + 1, X - 9)), ("c1", 1, (Z // 2 + 1, Y // 2 + 1, X - 9)), ("c2", 2, (Z // 2 + 1, Y // 2 + 1, X - 9)),
            ("border", 0, (0, 3, 5)), ("obstacle", 2, (2, 3, X - 5)),            # (2, 3, X - 5) is an obstacle cell of R.base()
            ("first", 0, (0, 0, 0)), ("last", 2, (Z - 1, Y - 1, X - 1)),          # the first and the last word of the array
            ("partial", 1, (Z - 1, Y - 2, X - 2))]                                # inside the last, partial brick


def word_places(g, dims):
    """(name, (k, j, i)) of the one density word that is not +0"""
    Z, Y, X = dims
    out = []
    if g == "g130":      # the eight corners of the interior brick x 64-127, y 4-7, z 4-7
        out += [("corner%d%d%d" % (a, b, c), ((4, 7)[a], (4, 7)[b], (64, 127)[c])) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    # two opposite corners of the last, partial brick; a border cell; the first and the last word; an obstacle cell of R.base()
    out += [("partial_lo", (Z - 1 - (Z - 1) % 4, Y - 1 - (Y - 1) % 4, X - 1 - (X - 1) % 64)), ("last", (Z - 1, Y - 1, X - 1)),
            ("first", (0, 0, 0)), ("border", (0, 5, 20)), ("obstacle", (2, 3, X - 5))]
    return out


def scenes():
    """name -> (batch of numpy arrays, steps)"""
    out = {}
    at, above = R.fastest_allowed(R.DT)
    for g, dims in GRIDS.items():
        Z, Y, X = dims
        for n, (place, comp, p) in enumerate(fast_places(dims)):
            for kind, v in (("at", at), ("above", above)):
                b = R.base(dims)
                b["density"][(0, 0) + BLOB] = 1.0
                b["UDiv"][(0, comp) + p] = -v if n % 2 else v
                out["fast_%s_%s_%s" % (kind, place, g)] = (b, 1)
        for place, p in word_places(g, dims):
            b = R.base(dims)
            b["density"][(0, 0) + p] = 1.0
            out["word_%s_%s" % (place, g)] = (b, 1)
        for name, word in (("negzero", np.float32(-0.0)), ("denormal", np.float32(1e-41)), ("inf", np.float32(np.inf)), ("nan", np.float32(np.nan))):
            for place, p in (("fluid", (5, 4, X - 3)), ("border", (Z - 1, 2, 7))):
                b = R.base(dims)
                b["density"][(0, 0) + p] = word
                out["bits_%s_%s_%s" % (name, place, g)] = (b, 1)
        b = R.base(dims, B=2)      # a batch of two with one empty item
        b["density"][(1, 0) + BLOB] = 0.9
        out["batch_%s" % g] = (b, 2)
        # a batch of three, smoke in every item over the same cells and the same flow: the items' temporaries must not share words
        b = R.base(dims, B=3)
        for item in range(3):
            b["density"][(item, 0) + BLOB] = 0.5 + 0.2 * item
            b["density"][item, 0, Z - 3:Z - 1, Y - 3:Y - 1, X - 8:X - 4] = 0.3 + 0.1 * item
        b["UDiv"][1:] = b["UDiv"][:1]
        out["batchfull_%s" % g] = (b, 2)
        # two density channels: the first is scanned inside pass A of advectVel, the second by the stand-alone scan
        b = R.base(dims)
        b["density"][(0, 0) + BLOB] = 1.0
        second = np.zeros_like(b["density"])
        second[0, 0, Z - 3:Z - 1, Y - 3:Y - 1, X - 8:X - 4] = 0.7
        b["density"] = [b["density"], second]
        out["twochan_%s" % g] = (b, 2)
    return out


def to_dev(batch):
    import torch
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")
    return {k: [dev(c) for c in v] if isinstance(v, list) else dev(v) for k, v in batch.items()}


def record(batch, extra=None):
    from fluidnet_amd import tfluids
    chans = batch["density"] if isinstance(batch["density"], list) else [batch["density"]]
    r = {"density": R.digest(np.stack([c.cpu().numpy() for c in chans])), "UDiv": R.digest(batch["UDiv"].cpu().numpy()),
         "pDiv": R.digest(batch["pDiv"].cpu().numpy())}
    r["trace_errors"] = int(tfluids.traceErrors(batch["UDiv"]))
    r["stats"] = list(tfluids.scal3SparseStats(batch["UDiv"]))
    r.update(extra or {})
    return r


def run_scenes(model):
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    res = {}
    for name, (b, steps) in scenes().items():
        batch = to_dev(b)
        tfluids.traceErrors(batch["UDiv"])
        tfluids.scal3SparseStats(batch["UDiv"])
        for _ in range(steps):
            simulate_native(None, R.MCONF, batch, model)
        res[name] = record(batch, {"bricks": R.n_bricks(b["UDiv"].shape[2:], b["UDiv"].shape[0])})
    return res


def run_kernels(model):
    """{scene: {timer name: launches}} of the second step of a one-channel and of a two-channel scene"""
    import torch
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    res = {}
    for name in ("batch_g130s", "twochan_g130s"):
        batch = to_dev(scenes()[name][0])
        simulate_native(None, R.MCONF, batch, model)
        torch.cuda.synchronize()
        with tfluids.profile(batch["UDiv"]) as prof:
            simulate_native(None, R.MCONF, batch, model)
            torch.cuda.synchronize()
        res[name] = {k: int(v["calls"]) for k, v in prof.kernels.items()}
    return res


if __name__ == "__main__":
    from fluidnet_amd import FluidNetModel
    model = FluidNetModel.default_3d(seed=1)
    res = {}
    for part in sys.argv[2:]:
        res[part] = {"scenes": lambda: run_scenes(model), "stale": lambda: R.run_stale(model), "sim": lambda: R.run_sim(model),
                     "graph": lambda: R.run_graph(model), "kernels": lambda: run_kernels(model)}[part]()
    json.dump(res, open(sys.argv[1], "w"))
    print("scal3 scan fold ok: " + " ".join(sys.argv[2:]))
