"""Helper of tests/test_hip_advect_bound.py: own process, started with TFL_ADVECT_MODE=fast (and, for `shapes`, the switches that
force a block shape: they are read once per process). `shapes <out.npz>`: every scene and case of tests/advect_bound.py through
the tolerance-mode kernels, results stored for the parent to compare. `slab <world>`: `world` virtual z-slab ranks step
maccormackOurs (density present: the fused pair kernels of advect_pair3.hip) in the tolerance mode and must equal the un-cut
tolerance-mode step on their owned planes bit for bit, as tests/test_hip_slab_methods.py asks of the exact mode."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _fast_context():
    import torch
    from fluidnet_amd import tfluids
    t = torch.zeros(1, device="cuda:0")
    lib, ctx = tfluids._context(t)
    assert lib.tfl_get_advect_mode(ctx) == 1, "TFL_ADVECT_MODE=fast did not reach the context"
    return t


def shapes(out):
    import numpy as np
    import advect_bound as A
    from hip_adapter import HipTfluids
    _fast_context()
    hip = HipTfluids()
    res = {}
    for name in A.SCENES:
        sc = A.scene(name)
        for op, method in A.CASES:
            res["%s|%s|%s" % (name, op, method)] = A.run_op(hip, sc, op, method)
    assert hip.traceErrors() == 0
    np.savez(out, **res)
    print("ADVECT_BOUND_SHAPES_OK", len(res))


def slab(world):
    import torch
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import simulate_native
    t = _fast_context()
    conf = M.mconf("maccormackOurs")
    ref = M._dev(M.scene(9 * world + 4))
    # the same two steps in the exact mode: the tolerance mode must have changed bits, or this run compares nothing new
    other = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in M._dev(M.scene(9 * world + 4)).items()}
    assert tfluids.set_advect_mode(t, "exact") == "fast"
    try:
        for _ in range(2):
            simulate_native(None, conf, other, None)
    finally:
        assert tfluids.set_advect_mode(t, "fast") == "exact"
    sims = M.sims_for(ref, conf, J.uneven_cuts(ref["flags"].size(2), world))
    for s in sims:
        assert s.lib.tfl_get_advect_mode(s._own_ctx) == 1
    M.run_and_compare(ref, conf, sims, rounds=1, steps=2)
    assert not torch.equal(ref["UDiv"], other["UDiv"]) and not torch.equal(ref["density"], other["density"])
    print("ADVECT_BOUND_SLAB_OK", world)


if __name__ == "__main__":
    if sys.argv[1] == "shapes":
        shapes(sys.argv[2])
    else:
        slab(int(sys.argv[2]))
