"""The brick scan of advectScalar as a by-product of pass A of advectVel (k_vel3_fwd_scan, fluidnet_amd/csrc/advect_scalar3_sparse.hip,
DESIGN.md 3.17): where tfl_simulate_step advects the first density channel over the brick lists it runs pass A of advectVel first,
which leaves the tags k_scal3_scan used to write; the results are the bits they were. Every scene of tests/scal3_scan_fold_run.py goes
through tfl_simulate_step in child processes: the EXPERIMENTS flavour with TFL_SCAL3_SPARSE = 0 (today's two full launches, today's
order) and = 2 (always the lists), and the product library (the host policy). density, UDiv and pDiv must be bit-equal and the
trace-error counts equal; the EXPERIMENTS flavour's counters show that the lists were used and what they held.

The two-plane pass A (KZ = 2, the kernel of grids above 6 M cells) runs the same scenes under TFL_VEL3_KZ=2, which both flavours read
and which the scan request goes along with: the small grids with an odd Z end on a one-plane group, which a 96 x 256 x 256 scene
would not. The scan's number is stepped across its wrap with TFL_SCAL3_SEQ0=-3 (EXPERIMENTS flavour)."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import scal3_scan_fold_run as F
from flavours import EXP_LIB

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(os.path.dirname(HERE), "fluidnet_amd", "libtfluids_hip.so")
pytestmark = pytest.mark.gpu
FIELDS = ("density", "UDiv", "pDiv")
SWITCHES = ("TFL_SCAL3_SPARSE", "TFL_VEL3_KZ", "TFL_SCAL3_SEQ0")


def _child(path, parts, mode, **switches):
    """mode: 0 / 1 / 2 = the EXPERIMENTS flavour under TFL_SCAL3_SPARSE, None = the product library"""
    if mode is not None and not os.path.exists(EXP_LIB):
        pytest.fail("fluidnet_amd/libtfluids_hip_exp.so is not built")
    env = dict(os.environ, TFL_LIBRARY=PRODUCT_LIB if mode is None else EXP_LIB)
    for name in SWITCHES:
        env.pop(name, None)
    if mode is not None:
        env["TFL_SCAL3_SPARSE"] = str(mode)
    env.update(switches)
    r = subprocess.run([sys.executable, os.path.join(HERE, "scal3_scan_fold_run.py"), path] + parts, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "scal3 scan fold ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return json.load(open(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{0, 2, None} -> one child process each; "kz2": the same under TFL_VEL3_KZ=2; "wrap": always the lists, the scan's number
    starting three scans before its wrap"""
    d = tmp_path_factory.mktemp("scal3_scan_fold")
    jobs = {0: (["scenes", "stale", "sim", "kernels"], 0, {}), "wrap": (["scenes", "sim"], 2, {"TFL_SCAL3_SEQ0": "-3"})}
    for mode in (2, None):
        jobs[mode] = (["scenes", "stale", "sim", "kernels"], mode, {})
        jobs[("kz2", mode)] = (["scenes", "sim", "kernels"], mode, {"TFL_VEL3_KZ": "2"})
    with ThreadPoolExecutor(len(jobs)) as ex:      # six small processes side by side: the suite waits for the slowest, not for the sum
        futures = {key: ex.submit(_child, str(d / ("run_%d.json" % n)), parts, mode, **sw) for n, (key, (parts, mode, sw)) in enumerate(jobs.items())}
        return {key: f.result() for key, f in futures.items()}


@pytest.fixture(scope="module")
def policy_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("scal3_scan_fold_policy")
    return _child(str(d / "run_1.json"), ["graph"], 1)


DEPTHS = ["kz1", "kz2"]


def trio(runs, depth):
    """(never, always the lists, the product library) at one depth of pass A; `never` runs no scanning form at either depth"""
    return (runs[0], runs[2], runs[None]) if depth == "kz1" else (runs[0], runs[("kz2", 2)], runs[("kz2", None)])


def same(runs, depth, part, name):
    off, on, prod = (r[part][name] for r in trio(runs, depth))
    for k in FIELDS:
        assert off[k] == on[k], (name, k, "TFL_SCAL3_SPARSE = 0 / 2")
        assert off[k] == prod[k], (name, k, "TFL_SCAL3_SPARSE = 0 / the product library")
    assert off["trace_errors"] == on["trace_errors"] == prod["trace_errors"], (name, off["trace_errors"], on["trace_errors"], prod["trace_errors"])
    assert off["stats"][:2] == [0, 0] and prod["stats"] == [0, 0, 0, 0, 0], name
    assert on["stats"][0] == on["stats"][1] > 0 and on["stats"][2] == 0, (name, on["stats"])      # every advection scanned and ran over the lists
    return on


def names(runs, prefix):
    found = sorted(n for n in runs[0]["scenes"] if n.startswith(prefix))
    assert found, prefix
    return found


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_velocity_word_at_and_above_the_bound(runs, depth):
    """one word of U at the largest value the scan lets pass and at the next float32, in each component, a border cell, an obstacle
    cell, the first and the last word of the array and the last, partial brick: at the bound the lists are the smoke's ring, above
    it every brick is listed"""
    at, above = names(runs, "fast_at_"), names(runs, "fast_above_")
    assert len(at) == len(above) == 8 * len(F.GRIDS)
    for name in at:
        on = same(runs, depth, "scenes", name)
        # L_B: the 2 x 2 x 2 ring of the smoke's corner brick; L_A: its ring, 3 x 3 x 3 bricks, or 3 x 3 x 2 where x has only two
        assert on["stats"][3:] == [27 if "g130" in name else 18, 8], (name, on["stats"])
    for name in above:
        on = same(runs, depth, "scenes", name)
        assert on["stats"][3] == on["stats"][4] == on["bricks"], (name, on["stats"])


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_density_word_at_brick_corners_borders_and_in_an_obstacle(runs, depth):
    found = names(runs, "word_")
    assert len(found) == 5 * len(F.GRIDS) + 8
    for name in found:
        on = same(runs, depth, "scenes", name)
        assert 0 < on["stats"][4] <= on["stats"][3] <= on["bricks"], (name, on["stats"])
    # a word in a corner brick of the grid lists that brick's 2 x 2 x 2 ring; one in the interior brick of the 3 x 3 x 3 grid all 27
    for name in names(runs, "word_first_") + names(runs, "word_last_") + names(runs, "word_partial_lo_"):
        assert runs[2]["scenes"][name]["stats"][4] == 8, name
    for name in names(runs, "word_corner"):
        assert runs[2]["scenes"][name]["stats"][4] == 27, name


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("word", ["negzero", "denormal", "inf", "nan"])
def test_words_that_are_not_plus_zero(runs, depth, word):
    for name in names(runs, "bits_%s_" % word):
        on = same(runs, depth, "scenes", name)
        assert on["stats"][4] > 0, (name, "the word's brick is listed")


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_batch_of_two_with_one_empty_item(runs, depth):
    for name in names(runs, "batch_"):
        on = same(runs, depth, "scenes", name)
        assert 0 < on["stats"][4] <= on["bricks"] // 2, (name, on["stats"])      # nothing of the empty item is listed


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_batch_of_three_with_smoke_in_every_item(runs, depth):
    """the scalar temporaries of the items beside pass A's live temporary: bounds are laid out three planes per item, so a forward
    field packed behind the second plane of the LAST item's would share words with the bounds of the items before it"""
    for name in names(runs, "batchfull_"):
        on = same(runs, depth, "scenes", name)
        assert 0 < on["stats"][4] <= on["bricks"], (name, on["stats"])


@pytest.mark.parametrize("depth", DEPTHS)
def test_two_density_channels(runs, depth):
    """the second channel is scanned by the stand-alone k_scal3_scan, with pass A's temporary live beside its passes"""
    for name in names(runs, "twochan_"):
        on = same(runs, depth, "scenes", name)
        assert on["stats"][:3] == [4, 4, 0] and 0 < on["stats"][4] <= on["bricks"], (name, on["stats"])      # two steps of two channels


@pytest.mark.parametrize("fill", ["nan", "1e30"])
def test_stale_temporaries_are_never_read(runs, fill):
    """two steps on a workspace the test owns, every word NaN / 1e30 before each step: the scalar temporaries now live on the planes
    pass B of advectVel writes later, beside the live temporary of its pass A"""
    on = same(runs, "kz1", "stale", fill)
    assert 0 < on["stats"][4] < on["stats"][3] < on["bricks"] == 75


@pytest.mark.parametrize("depth", DEPTHS)
def test_twelve_steps_of_the_plume_step_by_step(runs, depth):
    off, on, prod = trio(runs, depth)
    bricks = on["sim"]["bricks"]
    assert bricks == 144 and off["sim"]["nonzero_density"] > 0
    for i in range(12):
        a, b, c = (r["sim"]["steps"][i] for r in (off, on, prod))
        for k in FIELDS:
            assert a[k] == b[k] == c[k], (i, k)
        assert a["trace_errors"] == b["trace_errors"] == c["trace_errors"] == 0, i
        assert b["stats"][:3] == [1, 1, 0] and 0 < b["stats"][4] < bricks, (i, b["stats"])


def test_the_scan_number_across_its_wrap(runs):
    """every field's state starts three scans before the number's wrap (the plume crosses it at its fourth step, the two-step scenes
    sooner or later, as the allocator hands the states' fields back): the bits, and the lists' LENGTHS -- a stale tag that compared
    equal would list a brick more"""
    ref, wrapped = runs[2], runs["wrap"]
    for i in range(12):
        a, b = ref["sim"]["steps"][i], wrapped["sim"]["steps"][i]
        assert {k: a[k] for k in FIELDS} == {k: b[k] for k in FIELDS}, i
        assert a["stats"] == b["stats"] and a["trace_errors"] == b["trace_errors"], (i, a["stats"], b["stats"])
    for name, a in ref["scenes"].items():
        b = wrapped["scenes"][name]
        assert {k: a[k] for k in FIELDS} == {k: b[k] for k in FIELDS}, name
        assert a["stats"] == b["stats"] and a["trace_errors"] == b["trace_errors"], (name, a["stats"], b["stats"])


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_stand_alone_scan_is_gone_from_a_step_on_the_lists(runs, depth):
    """launches of one profiled step by timer name: with one channel no k_scal3_scan; with two, one (the second channel's)"""
    off, on, prod = trio(runs, depth)
    for r in (on, prod):
        one, two = r["kernels"]["batch_g130s"], r["kernels"]["twochan_g130s"]
        assert "k_scal3_scan" not in one and one["k_vel_fwd"] == one["k_vel_bwd"] == one["k_scal3_lists"] == one["k_scalar_fwd"] == one["k_scalar_bwd"] == 1, one
        assert two["k_scal3_scan"] == 1 and two["k_vel_fwd"] == two["k_vel_bwd"] == 1 and two["k_scal3_lists"] == two["k_scalar_fwd"] == two["k_scalar_bwd"] == 2, two
    for k in off["kernels"].values():      # never: no scan, no lists, in either form
        assert "k_scal3_scan" not in k and "k_scal3_lists" not in k and k["k_vel_fwd"] == 1, k


def test_a_captured_step_records_no_scan_and_replays_the_eager_bits(policy_run):
    g = policy_run["graph"]
    assert g["built"][:3] == [1, 1, 1]      # the eager warm-up step scanned (inside pass A) and ran over the lists; the captured call did neither
    assert g["replayed"][:3] == [0, 0, 0]
    assert g["graph"] == g["eager"]
