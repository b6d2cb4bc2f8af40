"""Per-voxel fp64 error bounds for the tolerance mode of the LDS-tiled advection kernels (tfl_set_advect_mode(TFL_ADVECT_FAST),
TFL_ADVECT_MODE=fast), next to the exact mode on the same inputs. tests/advect_bound.py gives the fp64 value, the bound derived
from the kernels' arithmetic and the mask of decided voxels; tests/test_advect_bound_cpu.py validates that machinery against the
reference alone. Here, per scene, operator and method:

  * the tolerance mode lies within the `fast` bound at every decided voxel; where the bound is 0 (every voxel the kernels hand
    to the generic path in eulerOurs; in maccormackOurs those that read no forward value a lane wrote) that asks for the exact
    mode's bits; non-fluid voxels carry the exact mode's bits;
  * the exact mode equals the oracle bit for bit, before and after the visit to the tolerance mode; traceErrors == 0;
  * in child processes (the block shapes are read once per process) every forced shape gives the SAME bits as the default
    shape in the tolerance mode: one arithmetic, many block shapes;
  * the z-slab step's fused pair kernels: tests/advect_bound_run.py `slab`.

Which test reaches which FAST = true instantiation:
  test_both_modes_within_their_bounds       k_vel3_fwd<1, true> / k_vel3_bwd_fold<true, ..> (advect_vel3_kernels.hpp), launch_a<2, 1, true>,
                                            launch_b<1, 2, true> (advect_scalar3.hip): the default shapes of small grids
  test_forced_shapes_..[kz1-scal-1x1]       launch_a<1, 1, true>, launch_b<1, 1, true>
  test_forced_shapes_..[kz2-scal-1x2]       k_vel3_fwd<2, true> / k_vel3_bwd<2, true> (advect_vel3_kernels.hpp), launch_a<1, 2, true>
  test_forced_shapes_..[kz2-scal-1x4]       launch_a<1, 4, true>, launch_b<1, 4, true> (the 256^3 shapes)
  test_forced_shapes_..[kz1-scal-2x1]       launch_b<2, 1, true>
  test_forced_shapes_..[marched]            zm::launch<true> (advect_scalar3_march.inc, experiments flavour)
  test_slab_pair_kernels_..                 k_adv3_fwd_pair<true> / k_adv3_bwd_pair<true> (advect_pair3.hip)
Run with -s for the witness ratios (largest error / bound per operator, method and mode); profiles/advect_bound.md keeps them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import advect_bound as A
from flavours import child_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RUN = os.path.join(HERE, "advect_bound_run.py")
SWITCHES = ("TFL_VEL3_KZ", "TFL_SCAL3_TZ", "TFL_ADVECT_GATHER", "TFL_SCALAR_GATHER", "TFL_ADVECT_MODE", "TFL_SCAL3M_CZ_A", "TFL_SCAL3M_CZ_B",
            "TFL_SCAL3_MARCH", "TFL_ADV_PAIR")


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    from hip_adapter import HipTfluids
    return HipTfluids()


def _in_mode(mode, fn):
    """fn() with the context of cuda:0 in `mode`, the exact mode restored whatever happens"""
    import torch
    from fluidnet_amd import tfluids
    t = torch.zeros(1, device="cuda:0")
    prev = tfluids.set_advect_mode(t, mode)
    try:
        return fn()
    finally:
        assert tfluids.set_advect_mode(t, prev) == mode


@pytest.fixture(scope="module")
def fast_default(hip):
    """every scene and case in the tolerance mode, default block shapes, in this process"""
    def run():
        out = {}
        for name in A.SCENES:
            sc = A.scene(name)
            for op, method in A.CASES:
                out[(name, op, method)] = A.run_op(hip, sc, op, method)
        return out
    return _in_mode("fast", run)


@pytest.mark.parametrize("name", A.SCENES)
def test_both_modes_within_their_bounds(hip, oracle, fast_default, name):
    sc = A.scene(name)
    for op, method in A.CASES:
        exact = A.run_op(hip, sc, op, method)
        fast = _in_mode("fast", lambda: A.run_op(hip, sc, op, method))
        again = A.run_op(hip, sc, op, method)
        res = A.evaluate(oracle, sc, op, method, "fast")
        rex = A.evaluate(oracle, sc, op, method, "exact")
        what = (name, op, method)
        assert np.array_equal(exact, res["oracle"]), (what, "exact mode vs oracle", int((exact != res["oracle"]).sum()))
        assert np.array_equal(again, exact), (what, "exact mode after the visit to the tolerance mode")
        assert np.array_equal(fast, fast_default[what]), (what, "the tolerance mode is not reproducible")
        assert np.isfinite(fast).all(), what
        bad, wf = A.check(fast, res)
        bade, we = A.check(exact, rex)
        fl = A.fluid_voxels(sc["flags"], fast)
        zero = res["decided"] & (res["bound"] == 0)
        print("%-22s %-12s %-14s err / bound: fast %.3f exact %.3f; voxels that differ between the modes %.1f%%, held to the exact "
              "mode's bits %.1f%%, undecided %.4f%%" % (name, op, method, wf, we, 100.0 * float((fast != exact).mean()),
                                                          100.0 * float(zero.mean()), 100.0 * float((~res["decided"] & fl).sum()) / max(int(fl.sum()), 1)))
        assert not bad.any(), (what, "fast", A.describe(fast, res, bad))
        assert not bade.any(), (what, "exact", A.describe(exact, rex, bade))
        assert np.array_equal(fast[zero], exact[zero]), what              # (what check() asked, said again: the generic path)
        assert np.array_equal(fast[~fl], exact[~fl]), (what, "a non-fluid or border voxel changed with the mode")
        if method == "eulerOurs":
            gen = res["decided"] & ~res["lanes"]
            assert np.array_equal(fast[gen], exact[gen]), (what, "generic path")
    assert hip.traceErrors() == 0


def _child(args, extra, timeout):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e = child_env(e, extra)
    e["TFL_ADVECT_MODE"] = "fast"
    return subprocess.run([sys.executable, RUN] + args, env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("env", [{}, {"TFL_VEL3_KZ": "1", "TFL_SCAL3_TZ": "1"}, {"TFL_VEL3_KZ": "2", "TFL_SCAL3_TZ": "12"},
                                 {"TFL_VEL3_KZ": "2", "TFL_SCAL3_TZ": "14"}, {"TFL_VEL3_KZ": "1", "TFL_SCAL3_TZ": "2"},
                                 {"TFL_SCAL3_MARCH": "1", "TFL_SCAL3M_CZ_A": "3", "TFL_SCAL3M_CZ_B": "2"}],
                         ids=["defaults", "kz1-scal-1x1", "kz2-scal-1x2", "kz2-scal-1x4", "kz1-scal-2x1", "marched"])
def test_forced_shapes_give_the_default_shapes_bits_in_fast_mode(fast_default, tmp_path, env):
    """TFL_ADVECT_MODE=fast in a child process with a forced block shape: bit-equal to this process's tolerance-mode results
    (which test_both_modes_within_their_bounds holds to the bound), on every scene and case."""
    out = str(tmp_path / "fast.npz")
    r = _child(["shapes", out], env, 900)
    assert r.returncode == 0 and "ADVECT_BOUND_SHAPES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert len(z.files) == len(fast_default)
    for (name, op, method), want in fast_default.items():
        got = z["%s|%s|%s" % (name, op, method)]
        assert np.array_equal(got, want), (env, name, op, method, int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("world", [2, 3])
def test_slab_pair_kernels_in_fast_mode_equal_the_uncut_fast_step(world):
    r = _child(["slab", str(world)], {}, 900)
    assert r.returncode == 0 and "ADVECT_BOUND_SLAB_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
