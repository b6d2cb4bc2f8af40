"""Helper of tests/test_hip_vort_pipe_static.py: own process, because the library (TFL_LIBRARY) and the switches TFL_VORT_FUSED,
TFL_VORT_CZ and TFL_VORT_TILE are chosen once per process. usage: vort_pipe_static_run.py <out.npz> <scene> [<scene> ...]; every
scene's results go into the .npz under "<scene>/<name>". The scenes are built from seeds: every process sees the same inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scenes  # noqa: E402

STRENGTH = 0.7
WINDOW = (2, 9, 12, 18)        # two plane runs of the 19-plane scenes: [2, 9) and [12, 18)
OUTSIDE = 7.0                  # what the planes outside the window hold before and after

# operator scenes: (Z, Y, X), seed, B. X = 70 and Y = 20: the 64 x 16 (and 32 x 16) tiles are ragged in x and in y
OP_SCENES = {"ragged19": ((19, 20, 70), 301, 1), "z12": ((12, 20, 70), 302, 1), "z14": ((14, 20, 70), 303, 1), "z40": ((40, 20, 70), 304, 1),
             "batch2": ((19, 20, 70), 305, 2), "awkward": ((19, 20, 70), 306, 1)}
STEP_SCENES = ("fold_step", "fold_slab")
STEP_DIMS = (20, 24, 72)       # fold_step: the plume's setConstVals pair covers rows 0-3 of EVERY plane: its box cuts every chunk boundary
SLAB_DIMS = (36, 24, 64)       # fold_slab: three ranks of 12 planes, each with its halo


def op_inputs(name):
    dims, seed, B = OP_SCENES[name]
    sc = scenes.make_scene(dims, seed=seed, vel_cells=2.0, B=B, empty_cells=True)
    U, fl = sc["U"].copy(), sc["flags"].copy()
    if B == 2:
        assert not np.array_equal(U[0], U[1]) and not np.array_equal(fl[0], fl[1])      # different fields per item
    if name == "awkward":
        # NaN and inf words sit where the operator DEFINES every output bit: a NaN that reaches a fluid cell's arithmetic comes out as
        # a NaN whose sign depends on the order in which the compiler hands two NaN addends to an add (measured with NaN / inf words
        # in fluid cells: 4 of 79 800 words differed between two builds of this kernel, in the NaN's sign bit alone), which is no
        # property of the operator. Here they must (a) be kept out by a SELECT, never by a multiplication with zero, and (b) pass
        # through to the output with sign and payload intact:
        #   * on the low border shell (x = 0, y = 0, z = 0): only the centred velocities of shell cells read those words, and they are 0
        #   * at the heart of an obstacle block (x 56-68, y 9-18, z 4-14: across the tile edges x = 63 | 64 and y = 15 | 16 and the chunk
        #     edges z = 8, 12): the force is NaN up to 3 cells away, face-averaged into the cells up to 3 away, all of them obstacles
        W = U.view(np.uint32)
        fl[0, 0, 4:15, 9:19, 56:69] = scenes.OBSTACLE
        for (z, y, x), w in (((9, 13, 63), 0x7FC00000), ((9, 14, 64), 0x7F800000), ((8, 13, 62), 0xFF800000), ((10, 14, 61), 0xFFC12345),
                             ((6, 8, 0), 0x7FC12345), ((7, 0, 20), 0xFFC00001), ((0, 5, 33), 0x7F800000), ((0, 6, 34), 0xFF800000)):
            W[0, :, z, y, x] = w
        # -0.0 words in fluid cells (signed zeros are defined by the arithmetic)
        U[0, :, 10:12, 4:9, 40:50] = -0.0
        U[0, 1, 15, :9] = -0.0
        # obstacle and empty cells on the tile edges x = 63 | 64 and y = 15 | 16
        fl[0, 0, 2:17, 3:8, 63] = scenes.OBSTACLE
        fl[0, 0, 2:17, 3:8, 64] = scenes.EMPTY
        fl[0, 0, 4:15, 15, 5:50] = scenes.EMPTY
        fl[0, 0, 4:15, 16, 5:50] = scenes.OBSTACLE
        assert np.isnan(U).sum() == 12 and np.isinf(U).sum() == 12
    return U, fl


def run_op(name, out):
    import torch
    from fluidnet_amd import tfluids
    dev = torch.device("cuda:0")
    Un, fn = op_inputs(name)
    U, fl = torch.from_numpy(Un).to(dev), torch.from_numpy(fn).to(dev)
    got = torch.full_like(U, 123.0)
    tfluids.vorticityConfinement(got, fl, STRENGTH, USrc=U)
    assert torch.equal(U.view(torch.int32), torch.from_numpy(Un).to(dev).view(torch.int32))          # the source is left alone
    out[name + "/full"] = got.cpu().numpy()
    if name == "ragged19" and os.environ.get("TFL_VORT_FUSED") == "1":
        # two plane runs in one launch (tfl_set_z_window: na and nb both non-zero). Only the fused route takes this grid under a
        # window (X % 4 != 0: the two launches refuse it), so the expectation is built from the whole-array result
        lib, ctx = tfluids._context(U)
        win = torch.full_like(U, OUTSIDE)
        assert lib.tfl_set_z_window(ctx, *WINDOW) == 0
        try:
            tfluids.vorticityConfinement(win, fl, STRENGTH, USrc=U)
        finally:
            assert lib.tfl_set_z_window(ctx, 0, 0, 0, 0) == 0
        out[name + "/window"] = win.cpu().numpy()


def plume(dims, uscale, obstacles_seed):
    import test_hip_simulate as T
    return T._plume_batch(dims, 0.15, uscale, obstacles_seed=obstacles_seed)


MCONF = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=2.0, gravityScale=0,
             vorticityConfinementAmp=3.0, simMethod="convnet")
SLAB_MCONF = dict(MCONF, buoyancyScale=1.0, gravityScale=0.2, vorticityConfinementAmp=2.0)


def run_fold_step(out):
    """the native step: the confinement writes U and applies the setConstVals pair that follows it (Fold)"""
    import torch
    import test_hip_simulate as T
    from fluidnet_amd import FluidNetModel
    from fluidnet_amd.simulate import simulate_native
    b = plume(STEP_DIMS, 1.0, 5)
    zs = np.nonzero((b["UBCInvMask"][0] != 1.0).any(axis=(0, 2, 3)))[0]
    assert zs.min() == 0 and zs.max() == STEP_DIMS[0] - 1          # the pair's box spans every plane
    tb = T._to_dev(b, torch.device("cuda:0"))
    model = FluidNetModel.default_3d(seed=1)
    for _ in range(3):
        simulate_native(None, MCONF, tb, model)
    for k in ("pDiv", "UDiv", "density"):
        out["fold_step/" + k] = tb[k].cpu().numpy()
    assert float(np.abs(out["fold_step/UDiv"]).max()) > 0


def run_fold_slab(out):
    """the z-slab step of three virtual ranks: each calls the confinement under its z-window (the owned planes and one above),
    with the pair folded; the middle rank's window starts and ends inside its array"""
    import torch
    import test_hip_simulate as T
    from fluidnet_amd.dist import run_virtual_ranks
    from oracle import simulate_np as S
    b = plume(SLAB_DIMS, 0.6, 11)
    ref = T._to_dev(b, torch.device("cuda:0"))
    sims = T._slab_sims(ref, SLAB_MCONF, 3, S.default_3d_layers(seed=2), overlap=True)
    run_virtual_ranks(sims, 3)
    for s in sims:
        for k in ("pDiv", "UDiv", "density"):
            out["fold_slab/%d/%s" % (s.lay.rank, k)] = s.lay.owned(s.batch[k]).cpu().numpy()
        s.close()
    assert float(np.abs(out["fold_slab/1/UDiv"]).max()) > 0


def main():
    path, names = sys.argv[1], sys.argv[2:]
    out = {}
    for n in names:
        if n in OP_SCENES:
            run_op(n, out)
        elif n == "fold_step":
            run_fold_step(out)
        elif n == "fold_slab":
            run_fold_slab(out)
        else:
            raise SystemExit("no such scene: " + n)
    np.savez(path, **out)
    print("vort pipe static ok: " + " ".join(names))


if __name__ == "__main__":
    main()
