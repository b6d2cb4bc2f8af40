"""advectScalar of tfl_simulate_step over a device-built list of the non-empty bricks (fluidnet_amd/csrc/advect_scalar3_sparse.hip,
DESIGN.md 3.17): the results are the bits they were. Every scene of tests/scal3_sparse_run.py goes through tfl_simulate_step in child
processes: against the EXPERIMENTS flavour with TFL_SCAL3_SPARSE = 0 (never: today's two launches) and = 2 (always: scan, lists and
the passes over the lists), and against the product library (the host policy). density, UDiv and pDiv must be bit-equal and the
trace-error counts equal. The EXPERIMENTS flavour's counters (tfl_scal3_sparse_stats) show that the lists were really used, that a
velocity face above |u dt| = 0.9 lists every brick, and what the policy does on a dense field."""
import json
import os
import subprocess
import sys

import pytest

import scal3_sparse_run as R
from flavours import EXP_LIB

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(os.path.dirname(HERE), "fluidnet_amd", "libtfluids_hip.so")
pytestmark = pytest.mark.gpu
FIELDS = ("density", "UDiv", "pDiv")


def _child(path, parts, mode):
    """mode: 0 / 1 / 2 = the EXPERIMENTS flavour under TFL_SCAL3_SPARSE, None = the product library"""
    if mode is not None and not os.path.exists(EXP_LIB):
        pytest.fail("fluidnet_amd/libtfluids_hip_exp.so is not built")
    env = dict(os.environ, TFL_LIBRARY=PRODUCT_LIB if mode is None else EXP_LIB)
    env.pop("TFL_SCAL3_SPARSE", None)
    if mode is not None:
        env["TFL_SCAL3_SPARSE"] = str(mode)
    r = subprocess.run([sys.executable, os.path.join(HERE, "scal3_sparse_run.py"), path] + parts, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "scal3 sparse ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return json.load(open(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{0, 2, None} -> scenes, stale and sim of one child process each"""
    d = tmp_path_factory.mktemp("scal3_sparse")
    return {mode: _child(str(d / ("run_%s.json" % mode)), ["scenes", "stale", "sim"], mode) for mode in (0, 2, None)}


@pytest.fixture(scope="module")
def policy_run(tmp_path_factory):
    """the EXPERIMENTS flavour under the policy (TFL_SCAL3_SPARSE = 1)"""
    d = tmp_path_factory.mktemp("scal3_sparse_policy")
    return _child(str(d / "run_1.json"), ["sim", "policy", "graph"], 1)


def same(runs, part, name):
    """the three runs of one scene agree bit for bit and in their trace-error counts; returns the always-lists run's record"""
    off, on, prod = (runs[m][part][name] for m in (0, 2, None))
    for k in FIELDS:
        assert off[k] == on[k], (name, k, "TFL_SCAL3_SPARSE = 0 / 2")
        assert off[k] == prod[k], (name, k, "TFL_SCAL3_SPARSE = 0 / the product library")
    assert off["trace_errors"] == on["trace_errors"] == prod["trace_errors"], (name, off["trace_errors"], on["trace_errors"], prod["trace_errors"])
    assert off["stats"][:2] == [0, 0] and prod["stats"] == [0, 0, 0, 0, 0], name      # never / the product library counts nothing
    assert on["stats"][0] == on["stats"][1] > 0 and on["stats"][2] == 0, (name, on["stats"])      # every step scanned and ran over the lists
    return on


def names(runs, prefix):
    found = sorted(n for n in runs[0]["scenes"] if n.startswith(prefix))
    assert found, prefix
    return found


def test_all_zero_density_with_a_boundary_box_lists_the_boxes_bricks(runs):
    # the boxes span 11 cells of x around the middle of rows 1-2, planes 4-6: one brick of the 70-wide grid (its ring: 3 x 2 x 2),
    # two of the 130-wide one (their ring: 3 x 2 x 3)
    assert same(runs, "scenes", "box_g70")["stats"][3:] == [12, 1]
    assert same(runs, "scenes", "box_g130")["stats"][3:] == [18, 2]
    for name in names(runs, "boxtwo_"):      # the second step finds what the first step's pair wrote
        on = same(runs, "scenes", name)
        assert 0 < on["stats"][4] < on["stats"][3] <= on["bricks"], (name, on["stats"])


def test_one_cell_walked_around_an_interior_brick(runs):
    """one non-zero cell at distance 0 ... 5 outside every face, edge and corner of the brick x 64-127, y 4-7, z 4-7 of the
    130 x 12 x 12 grid, and just inside it"""
    walked = names(runs, "walk_")
    assert len(walked) >= 26 * 4
    listed = set()
    for name in walked:
        on = same(runs, "scenes", name)
        assert 0 < on["stats"][4] <= on["stats"][3] <= on["bricks"] == 27
        listed.add(on["stats"][4])
    assert min(listed) == 8 and max(listed) == 27      # a cell in a corner brick lists 8 bricks, one in the centre brick all 27


@pytest.mark.parametrize("word", ["negzero", "denormal", "inf", "nan"])
def test_words_that_are_not_plus_zero(runs, word):
    for name in names(runs, "word_%s_" % word):
        on = same(runs, "scenes", name)
        assert on["stats"][4] > 0, (name, "the word's brick is listed")


def test_density_hidden_inside_obstacles(runs):
    for name in names(runs, "obstacle_"):
        on = same(runs, "scenes", name)
        assert 0 < on["stats"][4] <= on["bricks"]


def test_a_velocity_face_at_the_bound(runs):
    """|u dt| just below 0.9 on one face far from the smoke: lists as usual; just above, and a NaN face: every brick is listed"""
    for g in R.GRIDS:
        below, above, nan = (same(runs, "scenes", "face_%s_%s" % (n, g)) for n in ("below", "above", "nan"))
        assert 0 < below["stats"][4] < below["bricks"], below["stats"]
        assert above["stats"][3] == above["stats"][4] == above["bricks"], above["stats"]
        assert nan["stats"][3] == nan["stats"][4] == nan["bricks"], nan["stats"]


def test_a_batch_of_two_with_one_empty_item(runs):
    for name in names(runs, "batch_"):
        on = same(runs, "scenes", name)
        assert 0 < on["stats"][4] <= on["bricks"] // 2, (name, on["stats"])      # nothing of the empty item is listed


@pytest.mark.parametrize("fill", ["nan", "1e30"])
def test_stale_temporaries_are_never_read(runs, fill):
    """two steps on a workspace the test owns, every word NaN / 1e30 before each step"""
    on = same(runs, "stale", fill)
    assert 0 < on["stats"][4] < on["stats"][3] < on["bricks"] == 75      # bricks outside L_A keep the fill


def test_twelve_steps_of_the_plume_step_by_step(runs, policy_run):
    bricks = runs[2]["sim"]["bricks"]
    assert bricks == 144 and runs[0]["sim"]["nonzero_density"] > 0
    for i in range(12):
        off, on, prod, pol = (r["sim"]["steps"][i] for r in (runs[0], runs[2], runs[None], policy_run))
        for k in FIELDS:
            assert off[k] == on[k] == prod[k] == pol[k], (i, k)
        assert off["trace_errors"] == on["trace_errors"] == prod["trace_errors"] == pol["trace_errors"] == 0, i
        assert on["stats"][:3] == [1, 1, 0] and 0 < on["stats"][4] < bricks, (i, on["stats"])
        assert pol["stats"][:3] == [1, 1, 0] and pol["stats"][4] == on["stats"][4], (i, pol["stats"])      # the policy keeps to the lists
    for r in (runs[0], runs[2], policy_run):
        assert min(r["sim"]["zero_blocks"]) > 0      # the short path of DESIGN.md 3.12 is still taken


def test_the_policy_on_a_dense_field_and_back(policy_run):
    p, P = policy_run["policy"], R.POLICY_P
    assert p["min_density"] >= 0.2
    assert p["first"] == [1, 1, 0, p["bricks"], p["bricks"]]            # nothing known: scan and lists; every brick is listed
    assert p["dense"][:3] == [2, 0, 2 * P]                              # then the two full launches, and exactly one probe per P calls
    assert p["dense"][3:] == [p["bricks"], p["bricks"]]
    assert p["cleared_until_probe"] == [1, 0, P, 0, 0]                  # the cleared field is seen by the next probe ...
    assert p["after_probe"][:3] == [1, 1, 0]                            # ... and the step after it is back on the lists


def test_a_captured_step_records_no_scan_and_replays_the_eager_bits(policy_run):
    g = policy_run["graph"]
    assert g["built"][:3] == [1, 1, 1]      # the eager warm-up step scanned and ran over the lists; the captured call did neither
    assert g["replayed"][:3] == [0, 0, 0]
    assert g["graph"] == g["eager"]
