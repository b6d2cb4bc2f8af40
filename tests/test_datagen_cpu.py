"""Host-side checks of the data-set generator (fluidnet_amd/datagen.py), no GPU: the plan is a function of
(gconf, seed, run) and keeps its primitives where they belong, the restated curl field is divergence-free to its roundings, the
layout generate() writes is the one data.scan pairs up, and the plans the GPU tests generate from stay under the loader's
divergence threshold when the restated step runs them on the oracle's operators."""
import os

import numpy as np
import pytest

import datagen_ref as R


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return a == b


def _cube_model(n=8):
    v = np.zeros((n, n, n), np.float32)
    v[2:5, 1:6, 2:4] = 1.0
    return v


@pytest.mark.parametrize("is3D,dims", [(False, (1, 32, 32)), (False, (1, 48, 40)), (True, (12, 16, 20)), (True, (24, 24, 24))])
def test_a_plan_is_a_function_of_gconf_seed_and_run_and_keeps_its_primitives_in_place(is3D, dims):
    from fluidnet_amd import datagen
    g = datagen.default_gconf(is3D, dims, emitterSpeed=0.5, models=[_cube_model()] if is3D else ())
    seen_emitter = seen_obstacle = seen_voxels = False
    for run in range(12):
        a, b = datagen.plan_run(g, 5, run), datagen.plan_run(dict(g), 5, run)
        assert _same(a, b)
        assert not _same(a, datagen.plan_run(g, 6, run)) and not _same(a, datagen.plan_run(g, 5, run + 100))
        assert not _same(a, datagen.plan_run(g, 5, run, attempt=1))
        R.check_plan(a)
        seen_emitter |= bool(a["emitters"])
        seen_obstacle |= bool(a["obstacles"])
        seen_voxels |= a["voxels"] is not None
        assert 1 <= len(a["blobs"]) <= g["maxBlobs"] and len(a["emitters"]) <= g["maxEmitters"]
        assert a["dt"] == 0.1 and a["advectionMethod"] == "maccormack"
        m = datagen.mconf_of(a)
        assert m["simMethod"] == "pcg" and sorted(abs(v) for v in m["gravity"]) == [0.0, 0.0, 1.0]
    assert seen_emitter and seen_obstacle and (seen_voxels or not is3D)


def test_the_hash_is_a_counter_hash_with_exact_values():
    h = R.noise_hash(3, 4, 1, np.arange(1 << 16))
    v = R.noise_value(h)
    assert v.dtype == np.float32 and v.min() >= -1.0 and v.max() < 1.0
    assert np.array_equal(v * np.float32(8388608.0), np.round(v.astype(np.float64) * 8388608.0))      # multiples of 2^-23
    assert abs(float(v.mean())) < 0.01 and abs(float(v.std()) - 3 ** -0.5) < 0.01                       # uniform on [-1, 1)
    assert len(np.unique(h)) > 0.999 * h.size
    # the field does not depend on how it is cut: a cell's value is that of its index alone
    assert np.array_equal(R.noise_hash(3, 4, 1, np.arange(100, 200)), h[100:200])
    for other in (R.noise_hash(2, 4, 1, np.arange(64)), R.noise_hash(3, 5, 1, np.arange(64)), R.noise_hash(3, 4, 2, np.arange(64))):
        assert (other != h[:64]).mean() > 0.9
    # the mixer's known answers (a fixed point at 0; 1 -> the product chain written out)
    assert int(R.noise_mix(0)) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
    assert int(R.noise_mix(1)) == x


@pytest.mark.parametrize("dims", [(1, 9, 33), (5, 7, 19)], ids=["2d", "3d"])
def test_the_restated_curl_field_is_divergence_free_to_its_roundings(dims):
    is3D = dims[0] > 1
    psi = R.noise_field(9, 2, 3 if is3D else 1, dims)
    U = R.curl_mac(psi, 1.0, is3D)
    assert U.dtype == np.float32 and U.shape == (1, 3 if is3D else 2) + dims and float(np.abs(U).max()) > 0.5
    div = R.mac_divergence64(U, is3D)
    assert div.size == (dims[0] - 1 if is3D else 1) * (dims[1] - 1) * (dims[2] - 1)
    bound = R.curl_roundings_bound(is3D) * 2.0 ** -24 * float(np.abs(psi).max())
    print("max|div| = %.3e, bound %.3e" % (float(np.abs(div).max()), bound))
    assert float(np.abs(div).max()) <= bound
    # the clamped neighbour: nothing flows along the grid's last line of each axis
    assert not U[0, 1, :, :, -1].any() if not is3D else True
    # and a scaled field is the scaled field
    assert np.array_equal(R.curl_mac(psi, 0.5, is3D), U * np.float32(0.5))


def test_the_layout_generate_writes_is_what_scan_pairs_up(tmp_path):
    from fluidnet_amd import data, datagen
    g = datagen.default_gconf(False, (1, 16, 16), steps=12, saveEvery=4)
    assert datagen.saved_steps(g) == [0, 4, 8]
    out = str(tmp_path / "sets" / "mine")
    for prefix, runs in (("tr", (0, 1, 2)), ("te", (3,))):
        for run in runs:
            for f in range(len(datagen.saved_steps(g))):
                for fn in datagen.frame_paths(out, prefix, run, f):
                    os.makedirs(os.path.dirname(fn), exist_ok=True)
                    open(fn, "wb").close()
    conf = dict(dataDir=str(tmp_path / "sets"), dataset="mine", ignoreFrames=0)
    sc = data.scan(conf, "tr")
    assert [r["dir"] for r in sc["runs"]] == ["000000", "000001", "000002"] and len(sc["samples"]) == 9
    for r in sc["runs"]:
        assert [os.path.basename(f) for f in r["files"]] == ["%06d.bin" % f for f in range(3)]
        assert [os.path.basename(f) for f in r["divFiles"]] == ["%06d_divergent.bin" % f for f in range(3)]
    assert [r["dir"] for r in data.scan(conf, "te")["runs"]] == ["000003"]


@pytest.mark.parametrize("is3D,dims", R.GEN_CASES, ids=["2d", "3d"])
def test_the_gpu_tests_plans_stay_under_the_divergence_threshold_on_the_oracle(is3D, dims):
    """the condition test_hip_datagen's `no run is dropped` rests on, shown without a GPU: the restated run (the oracle's
    operators, PCG included) keeps the signed maximum of div(U target) under data.DIV_THRESHOLD for the plans of the test's
    seed (profiles/datagen.md records the figures)"""
    from fluidnet_amd import data, datagen
    from oracle import simulate_np
    from oracle.oracle import OracleTfluids, available
    assert available()
    ops = OracleTfluids()
    g = R.gen_gconf(is3D, dims)
    for run in range(R.GEN_RUNS):
        plan = datagen.plan_run(g, R.GEN_SEED, run)
        R.check_plan(plan)
        frames = R.run_frames(ops, simulate_np, plan, g, datagen.mconf_of(plan), datagen.noise_seed(plan), datagen.emitter_pairs(plan))
        assert len(frames) == 6
        worst = -np.inf
        for divergent, target in frames:
            div = np.zeros_like(target["p"])
            ops.velocityDivergenceForward(np.ascontiguousarray(target["U"]), target["flags"], div)
            worst = max(worst, float(div.max()))
            assert np.isfinite(target["U"]).all() and np.isfinite(divergent["U"]).all()
        print("dims %s run %d: max div(U target) = %.3e, peak |U| dt = %.3f" % (dims, run, worst, float(np.abs(frames[-1][1]["U"]).max()) * plan["dt"]))
        assert worst <= data.DIV_THRESHOLD


def _count_stamped(gconf, seed, runs):
    from fluidnet_amd import datagen
    n = 0
    for run in range(runs):
        plan = datagen.plan_run(gconf, seed, run)
        R.check_plan(plan)
        if plan["voxels"] is not None:
            n += 1
            assert plan["voxels"].shape == gconf["dims"] and plan["voxels"].any()
    return n


def test_a_voxel_model_with_a_large_bounding_box_stays_inside_the_border():
    """a 48^3 array holding a 44^3 object on a 64^3 grid: its bounding box spans over 0.6 of the grid, so most of the +-0.2 offsets
    would push it out of the grid; every plan must come through (check_plan: the model's cells off the border) and the model must
    be stamped whole wherever a plan holds one"""
    from fluidnet_amd import datagen
    model = np.zeros((48, 48, 48), np.float32)
    model[2:46, 2:46, 2:46] = 1.0
    g = datagen.default_gconf(True, (64, 64, 64), models=[model], maxEmitters=0)
    stamped = 0
    for run in range(40):
        plan = datagen.plan_run(g, 1, run)
        if plan["voxels"] is not None:
            stamped += 1
            v = plan["voxels"]
            assert int(v.sum()) == 44 ** 3
            assert not (v[[0, -1]].any() or v[:, [0, -1]].any() or v[:, :, [0, -1]].any())
    # maxModels = 1: the number of models is drawn from {0, 1}; without emitters no try can fail, so about half the plans hold it
    assert 10 <= stamped <= 30, stamped


def test_a_voxel_model_whose_array_equals_the_grid_is_stamped():
    """a binvox file at the grid's own resolution: a 64^3 array with a 20^3 object on a 64^3 grid (the array itself is larger than
    the grid less its border; the object is not), and a non-cubic array, which no flip applies to"""
    from fluidnet_amd import datagen
    model = np.zeros((64, 64, 64), np.float32)
    model[10:30, 20:40, 5:25] = 1.0
    g = datagen.default_gconf(True, (64, 64, 64), models=[model], maxEmitters=0)
    assert 10 <= _count_stamped(g, 1, 40) <= 30
    flat = np.zeros((24, 30, 40), np.float32)
    flat[3:9, 4:20, 6:30] = 1.0
    g = datagen.default_gconf(True, (24, 32, 48), models=[flat], maxEmitters=0)
    assert 10 <= _count_stamped(g, 2, 40) <= 30
    # with emitters a try can fail on the clearance, never with an exception
    g = datagen.default_gconf(True, (64, 64, 64), models=[model])
    assert _count_stamped(g, 3, 40) >= 5


def test_a_voxel_model_that_can_never_fit_is_refused_by_name():
    from fluidnet_amd import TfluidsError, datagen
    model = np.zeros((48, 48, 48), np.float32)
    model[2:46, 2:46, 2:46] = 1.0
    with pytest.raises(TfluidsError, match="voxel model 1 can never fit"):
        datagen.plan_run(datagen.default_gconf(True, (32, 32, 32), models=[np.ones((4, 4, 4), np.float32), model]), 1, 0)
    with pytest.raises(TfluidsError, match="voxel model 0 is not a 3-D array with a set voxel"):
        datagen.plan_run(datagen.default_gconf(True, (32, 32, 32), models=[np.zeros((4, 4, 4), np.float32)]), 1, 0)
    # a slab that fits only when flipped: refused in no orientation that fits, stamped in those that do
    slab = np.zeros((40, 40, 40), np.float32)
    slab[1:39, 1:39, 18:22] = 1.0      # 38 x 38 x 4 (z, y, x)
    g = datagen.default_gconf(True, (40, 40, 8), models=[slab], maxEmitters=0)      # grid z = 40, y = 40, x = 8
    assert _count_stamped(g, 4, 40) >= 5
