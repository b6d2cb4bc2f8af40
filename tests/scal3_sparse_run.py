"""Helper of tests/test_hip_scal3_sparse.py: own process, because the library (TFL_LIBRARY) and the switch TFL_SCAL3_SPARSE are chosen
once per process. usage: scal3_sparse_run.py <out.json> <part> [<part> ...]; every part steps scenes through tfl_simulate_step and
records sha1 digests of density / UDiv / pDiv, the trace-error count and tfl_scal3_sparse_stats (zeros from the product library).
  scenes   the operator scenes of SCENES (one or two steps each)
  stale    one scene twice, the step's workspace owned by the test and pre-filled with NaN, then with 1e30
  sim      twelve steps of the 48^3 plume + obstacle scene, recorded step by step, and the all-zero-block counters of DESIGN.md 3.12
  policy   a density >= 0.2 everywhere, then cleared: the counters after each phase
  graph    GraphedSimulate(native=True) against the eager step"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from scenes import OBSTACLE, empty_domain, smooth_field  # noqa: E402

DT = 0.1
GRIDS = {"g70": (11, 13, 70), "g130": (12, 12, 130)}      # (Z, Y, X): no extent a multiple of the brick / three bricks in x
BRICK = (4, 4, 64)                                         # (z, y, x)
MCONF = dict(dt=DT, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.0, gravityScale=0,
             vorticityConfinementAmp=1.0, simMethod="convnet")
STALE_GRID = (20, 20, 130)                                 # 5 x 5 x 3 bricks
POLICY_P = 16


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def n_bricks(dims, B=1):
    return B * int(np.prod([-(-n // b) for n, b in zip(dims, BRICK)]))


def fastest_allowed(dt, disp=0.9):
    """the largest float32 u with fl(u * dt) <= 0.9f (the scan lets it pass), and the next float32 (it does not)"""
    F = np.float32
    u = F(F(disp) / F(dt))
    while F(u * F(dt)) > F(disp):
        u = np.nextafter(u, F(0))
    while F(np.nextafter(u, F(np.inf)) * F(dt)) <= F(disp):
        u = np.nextafter(u, F(np.inf))
    return u, np.nextafter(u, F(np.inf))


def base(dims, B=1, seed=3):
    """a slow smooth velocity (|u dt| <= 0.3), a few obstacle cells, density and pressure zero, no boundary pairs"""
    Z, Y, X = dims
    rng = np.random.RandomState(seed)
    flags = empty_domain(B, Z, Y, X, True).astype(np.float32)
    for k, j, i in ((Z // 2, Y // 2, X // 3), (2, 3, X - 5), (Z - 3, 2, 10), (Z // 2, Y // 2, X // 3 + 1)):
        flags[:, 0, k, j, i] = OBSTACLE
    U = smooth_field((B, 3, Z, Y, X), rng)
    U = (U * (0.3 / DT / np.abs(U).max())).astype(np.float32)
    return dict(pDiv=np.zeros((B, 1, Z, Y, X), np.float32), UDiv=U, flags=flags, density=np.zeros((B, 1, Z, Y, X), np.float32))


def with_box(b, box):
    """a sparse idempotent setConstVals pair for the density: 1.0 on the cells of box = (z0, z1, y0, y1, x0, x1), inclusive"""
    z0, z1, y0, y1, x0, x1 = box
    bc, mk = np.zeros_like(b["density"]), np.ones_like(b["density"])
    bc[:, :, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 1.0
    mk[:, :, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 0.0
    b["densityBC"], b["densityBCInvMask"] = bc, mk
    return b


def walk_positions(dims):
    """(name, (k, j, i)): distance 0 (just inside) to 5 outside every face, edge and corner of the interior brick of g130"""
    Z, Y, X = dims
    lo, hi, mid = (4, 4, 64), (7, 7, 127), (5, 5, 96)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) == (0, 0, 0):
                    continue
                d = (dz, dy, dx)
                start = [lo[a] if d[a] < 0 else (hi[a] if d[a] > 0 else mid[a]) for a in range(3)]
                for t in range(6):
                    p = tuple(start[a] + t * d[a] for a in range(3))
                    if all(0 <= p[a] < (Z, Y, X)[a] for a in range(3)):
                        out.append(("walk_%d%d%d_%d" % (dz + 1, dy + 1, dx + 1, t), p))
    return out


def scenes():
    """name -> (batch of numpy arrays, steps)"""
    out = {}
    for g, dims in GRIDS.items():
        Z, Y, X = dims
        # an all-zero density with a non-empty density box: the first step lists the box's bricks
        out["box_" + g] = (with_box(base(dims), (4, 6, 1, 2, X // 2 - 5, X // 2 + 5)), 1)
        out["boxtwo_" + g] = (with_box(base(dims), (4, 6, 1, 2, X // 2 - 5, X // 2 + 5)), 2)
        # words that are not +0.0 in a fluid cell
        for name, word in (("negzero", np.float32(-0.0)), ("denormal", np.float32(1e-41)), ("inf", np.float32(np.inf)), ("nan", np.float32(np.nan))):
            b = base(dims)
            b["density"][0, 0, 5, 8, X - 20] = word
            out["word_%s_%s" % (name, g)] = (b, 1)
        # non-zero density inside obstacle cells next to empty fluid: single cells and a 3^3 block
        b = base(dims)
        b["flags"][0, 0, 4:7, 7:10, 30:33] = OBSTACLE
        b["density"][0, 0, 4:7, 7:10, 30:33] = 0.8
        b["flags"][0, 0, 3, 3, X - 12] = OBSTACLE
        b["density"][0, 0, 3, 3, X - 12] = 0.5
        b["density"][0, 0, Z // 2, Y // 2, X // 3] = 0.7          # one of base()'s obstacle cells
        out["obstacle_" + g] = (b, 2)
        # one velocity face just below / just above |u dt| = 0.9, far from the smoke; and a NaN face
        below, above = fastest_allowed(DT)
        for name, v in (("below", below), ("above", above), ("nan", np.float32(np.nan))):
            b = base(dims)
            b["density"][0, 0, 4:7, 4:7, 8:11] = 1.0
            b["UDiv"][0, 1, 6, 7, X - 9] = -v if name == "below" else v
            out["face_%s_%s" % (name, g)] = (b, 1)
        # a batch of two with one empty item
        b = base(dims, B=2)
        b["density"][1, 0, 3:6, 5:8, 20:30] = 0.9
        out["batch_" + g] = (b, 2)
    for name, p in walk_positions(GRIDS["g130"]):
        b = base(GRIDS["g130"])
        b["density"][(0, 0) + p] = 1.0
        out[name] = (b, 1)
    return out


def to_dev(batch):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in batch.items()}


def record(batch, extra=None):
    from fluidnet_amd import tfluids
    r = {k: digest(batch[k].cpu().numpy()) for k in ("density", "UDiv", "pDiv")}
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
            simulate_native(None, MCONF, batch, model)
        res[name] = record(batch, {"bricks": n_bricks(b["density"].shape[2:], b["density"].shape[0])})
    return res


def run_stale(model):
    """the step called as simulate_native calls it, on a workspace this test owns and fills before every step"""
    import torch
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import _native_args
    res = {}
    for fill in ("nan", "1e30"):
        b = with_box(base(STALE_GRID), (1, 2, 1, 2, 8, 12))      # smoke and box in one corner: most bricks are outside L_A
        b["density"][0, 0, 1:3, 1:3, 3:7] = 1.0
        batch = to_dev(b)
        lib, ctx = tfluids._context(batch["UDiv"])
        for _ in range(2):
            prm, st, keep = _native_args(lib, ctx, MCONF, batch, model)
            nws = int(lib.tfl_simulate_workspace_floats(ctx, ctypes.byref(prm), ctypes.byref(st)))
            ws = torch.full((nws,), float(fill), dtype=torch.float32, device="cuda:0")
            tfluids._call(lib, ctx, lib.tfl_simulate_step(ctx, ctypes.byref(prm), ctypes.byref(st), ctypes.c_void_p(ws.data_ptr()), nws))
            torch.cuda.synchronize()
            del keep, ws
        res[fill] = record(batch, {"bricks": n_bricks(STALE_GRID)})
    return res


def run_sim(model):
    import torch
    import bench
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    batch, mconf = bench.build_scene(48, 48, None, torch.device("cuda:0"))
    tfluids.scal3ZeroBlocks(batch["flags"])
    tfluids.scal3SparseStats(batch["flags"])
    steps = []
    for _ in range(12):
        simulate_native(None, mconf, batch, model)
        steps.append(record(batch))
    return dict(steps=steps, bricks=n_bricks((48, 48, 48)), zero_blocks=list(tfluids.scal3ZeroBlocks(batch["flags"])),
                nonzero_density=int((batch["density"] != 0).sum()))


def run_policy():
    """Jacobi projection, no forces: 1 + 2 P steps on a dense density, the density cleared, P + 1 more steps; a synchronise after
    every step, so that each decision sees what the step before it published"""
    import torch
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    dims = (32, 32, 32)
    b = base(dims)
    rng = np.random.RandomState(9)
    b["density"] = (np.abs(smooth_field(b["density"].shape, rng)) + 0.2).astype(np.float32)
    mconf = dict(MCONF, buoyancyScale=0, vorticityConfinementAmp=0, simMethod="jacobi", maxIter=2)
    batch = to_dev(b)
    tfluids.scal3SparseStats(batch["UDiv"])
    min_density = float(batch["density"].min())

    def steps(n):
        for _ in range(n):
            simulate_native(None, mconf, batch, None)
            torch.cuda.synchronize()
        return list(tfluids.scal3SparseStats(batch["UDiv"]))
    res = dict(bricks=n_bricks(dims), first=steps(1), dense=steps(2 * POLICY_P), min_density=min_density)
    batch["density"].zero_()
    res["cleared_until_probe"] = steps(POLICY_P)
    res["after_probe"] = steps(1)
    return res


def run_graph(model):
    import torch
    import bench
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import GraphedSimulate, simulate_native
    dev = torch.device("cuda:0")
    eager, mconf = bench.build_scene(24, 24, None, dev)
    graphed, _ = bench.build_scene(24, 24, None, dev)
    tfluids.scal3SparseStats(eager["UDiv"])
    g = GraphedSimulate(None, mconf, graphed, model, warmup=1, native=True)
    torch.cuda.synchronize()
    built = list(tfluids.scal3SparseStats(eager["UDiv"]))      # one eager warm-up step, then the captured call
    for _ in range(4):
        g.step()
    torch.cuda.synchronize()
    replayed = list(tfluids.scal3SparseStats(eager["UDiv"]))
    for _ in range(4):
        simulate_native(None, mconf, eager, model)
    return dict(built=built, replayed=replayed, graph={k: digest(graphed[k].cpu().numpy()) for k in ("density", "UDiv", "pDiv")},
                eager={k: digest(eager[k].cpu().numpy()) for k in ("density", "UDiv", "pDiv")})


if __name__ == "__main__":
    from fluidnet_amd import FluidNetModel
    model = FluidNetModel.default_3d(seed=1)
    res = {}
    for part in sys.argv[2:]:
        res[part] = {"scenes": lambda: run_scenes(model), "stale": lambda: run_stale(model), "sim": lambda: run_sim(model),
                     "policy": run_policy, "graph": lambda: run_graph(model)}[part]()
    json.dump(res, open(sys.argv[1], "w"))
    print("scal3 sparse ok: " + " ".join(sys.argv[2:]))
