"""Helper of tests/test_hip_scal3_zero_skip.py: own process, because the library (TFL_LIBRARY: the EXPERIMENTS flavour, which
counts the all-zero blocks) and the switch TFL_SCAL3_ZSKIP are chosen once per process.
`ops <out.json>`: every operator case of tests/scal3_zero_skip.py x method x mode -> sha1 of the result and of the fwd / bounds
temporaries, the counted blocks and the blocks the model finds empty.
`sim <out.json>`: 12 steps of simulate() on the 48^3 plume scene -> sha1 of density, UDiv, pDiv, and the counted blocks.
`slab`: two virtual z-slab ranks on 32 x 16 x 24 (a mostly empty density, a jet through the cut) against the un-cut step."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _record(r):
    import scal3_zero_skip as Z
    return dict(out=Z.digest(r["out"]), fwd=None if r["fwd"] is None else Z.digest(r["fwd"]),
                bounds=None if r["bounds"] is None else Z.digest(r["bounds"]), counted=list(r["counted"]), want=list(r["want"]))


def ops(path):
    import scal3_zero_skip as Z
    res = {}
    named = list(Z.cases().items()) + [("cell_%d_%d_%d" % p, Z.single_cell_case(p)) for p in Z.single_cell_positions()]
    for name, case in named:
        for method in Z.METHODS:
            for mode in Z.MODES:
                res["%s/%s/%s" % (name, method, mode)] = _record(Z.run_case(case, method, mode))
    json.dump(res, open(path, "w"))
    print("ops ok: %d runs" % len(res))


def sim(path):
    import torch
    import bench
    import scal3_zero_skip as Z
    from fluidnet_amd import FluidNetModel, tfluids
    from fluidnet_amd.simulate import simulate
    dev = torch.device("cuda:0")
    batch, mconf = bench.build_scene(48, 48, None, dev)
    model = FluidNetModel.default_3d(seed=1)
    tfluids.scal3ZeroBlocks(batch["flags"])
    for _ in range(12):
        simulate(None, mconf, batch, model)
    counted = tfluids.scal3ZeroBlocks(batch["flags"])
    res = {k: Z.digest(batch[k].cpu().numpy()) for k in ("density", "UDiv", "pDiv")}
    res["counted"] = list(counted)
    res["nonzero_density"] = int((batch["density"] != 0).sum())
    json.dump(res, open(path, "w"))
    print("sim ok", res["counted"])


def slab():
    import ctypes
    import torch
    import test_hip_simulate as T
    import test_hip_slab_methods as M
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate_native
    b = M.scene(24, 16, 32)
    b["density"][...] = 0.0
    b["density"][:, :, 9:13, 5:9, 12:20] = 1.0          # a blob across the cut at plane 12; everything else stays +0.0
    ref = T._to_dev(b, torch.device("cuda:0"))
    conf = M.mconf("maccormackOurs")
    sims = M.sims_for(ref, conf, [0, 12, 24])
    counted = [0, 0]
    for _ in range(3):
        for _ in range(2):
            simulate_native(None, conf, ref, None)
        run_virtual_ranks(sims, 2)
        M.assert_owned(sims, ref)
    for s in sims:
        lib, ctx = s._context()
        out = (ctypes.c_int64 * 2)()
        assert lib.tfl_scal3_zero_blocks(ctx, out) == 0
        counted[0] += out[0]
        counted[1] += out[1]
        s.close()
    assert float(ref["density"].abs().max()) > 0 and float((ref["density"] == 0).float().mean()) > 0.5
    print("slab ok: counted %d %d" % tuple(counted))


if __name__ == "__main__":
    if sys.argv[1] == "ops":
        ops(sys.argv[2])
    elif sys.argv[1] == "sim":
        sim(sys.argv[2])
    else:
        slab()
