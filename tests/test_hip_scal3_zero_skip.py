"""advectScalar's short path for blocks whose staged tile is all +0.0 (fluidnet_amd/csrc/advect_scalar3.hip):
the results are the bits they were. Every case of tests/scal3_zero_skip.py runs with maccormackOurs and eulerOurs, in the
exact and the tolerance mode, three times: in this process against the product library, and in two child processes against the
EXPERIMENTS flavour with the short path on and off (TFL_SCAL3_ZSKIP=0; tests/scal3_zero_skip_run.py). Exact mode: equal to
the C oracle as tests/test_hip_parity.py compares this operator, and the same bits from all three runs. Tolerance mode: the same
bits as the same library with the switch off. The fwd / bounds temporaries: the same bits on and off. The EXPERIMENTS
flavour's counter: exactly the blocks whose staged box holds no non-zero fluid word with the switch on (so a block whose box
holds the cell is never counted, and the short path is really taken), 0 with it off."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scal3_zero_skip as Z
from flavours import EXP_LIB, is_experiments_process

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


def _child(args, zskip, timeout=900):
    if not os.path.exists(EXP_LIB):
        pytest.fail("fluidnet_amd/libtfluids_hip_exp.so is not built")
    env = dict(os.environ, TFL_LIBRARY=EXP_LIB)
    env.pop("TFL_SCAL3_ZSKIP", None)
    if not zskip:
        env["TFL_SCAL3_ZSKIP"] = "0"
    r = subprocess.run([sys.executable, os.path.join(HERE, "scal3_zero_skip_run.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def exp_ops(tmp_path_factory):
    """{True: short path on, False: off} -> the records of scal3_zero_skip_run.py ops (EXPERIMENTS flavour)"""
    d = tmp_path_factory.mktemp("zskip")
    out = {}
    for on in (True, False):
        path = str(d / ("ops_%d.json" % on))
        assert "ops ok" in _child(["ops", path], on)
        out[on] = json.load(open(path))
    return out


@pytest.fixture(scope="module")
def cases():
    return Z.cases()


_product = {}


def product(name, case, method, mode):
    """the product library's run of one case (this process), computed once"""
    key = (name, method, mode)
    if key not in _product:
        _product[key] = Z.run_case(case, method, mode)
    return _product[key]


def oracle_out(oracle, case, method, strict=True):
    s = case["s"].copy()
    prev = oracle.strict
    oracle.strict = strict
    try:
        oracle.advectScalar(Z.DT, s, case["U"], case["flags"], method)
    finally:
        oracle.strict = prev
    return s


def check_case(name, case, oracle, exp_ops, strict=True):
    """one case, both methods and modes, through every comparison of the module's docstring; returns the counted blocks"""
    counted = {}
    for method in Z.METHODS:
        want = oracle_out(oracle, case, method, strict)
        for mode in Z.MODES:
            key = "%s/%s/%s" % (name, method, mode)
            got, on, off = product(name, case, method, mode), exp_ops[True][key], exp_ops[False][key]
            if mode == "exact":
                assert Z.same_as_oracle(got["out"], want), (key, int((got["out"] != want).sum()))
            for part in ("out", "fwd", "bounds"):
                assert on[part] == off[part], (key, part, "short path on / off")
            assert Z.digest(got["out"]) == off["out"], (key, "product library / switch off")
            if got["fwd"] is not None:
                assert Z.digest(got["fwd"]) == off["fwd"] and Z.digest(got["bounds"]) == off["bounds"], key
            assert on["counted"] == on["want"], (key, on["counted"], on["want"])
            assert off["counted"] == [0, 0], key
            if not is_experiments_process():
                assert list(got["counted"]) == [0, 0], key       # the product library counts nothing
            counted[(method, mode)] = on["counted"]
    return counted


def test_all_zero_density_every_block_takes_the_short_path(oracle, exp_ops, cases):
    for name in ("all_zero", "golden_shape_all_zero"):
        case = cases[name]
        n = Z.n_blocks(case["s"].shape)
        counted = check_case(name, case, oracle, exp_ops)
        for (method, mode), c in counted.items():
            assert c == [n, n if method == "maccormackOurs" else 0], (name, method, mode, c, n)
    assert Z.n_blocks(cases["all_zero"]["s"].shape) == 96


def test_one_cell_walked_around_a_block(oracle, exp_ops):
    """one non-zero cell at distance 1 and 2 outside every face, edge and corner of an interior block and just inside it: the
    same bits everywhere, and the counters are exactly the blocks whose staged box does not hold the cell (pass A: halo 2 with
    the bounds search, halo 1 without; pass B: the boxes of the forward field, halo 1)"""
    fewest = 96
    for p in Z.single_cell_positions():
        counted = check_case("cell_%d_%d_%d" % p, Z.single_cell_case(p), oracle, exp_ops)
        fewest = min(fewest, counted[("maccormackOurs", "exact")][0])
        assert 0 < counted[("maccormackOurs", "exact")][0] < 96
    assert fewest <= 96 - 2 * 8          # a cell near a corner of the block sits in the halo boxes of 8 blocks per batch item


@pytest.mark.parametrize("word", ["neg_zero", "denormal", "inf", "nan"])
def test_words_that_are_not_plus_zero(oracle, exp_ops, cases, word):
    """-0.0, a denormal, +inf and a NaN in a fluid cell of the halo of an otherwise empty block: that block traces"""
    counted = check_case("word_" + word, cases["word_" + word], oracle, exp_ops)
    assert counted[("maccormackOurs", "exact")][0] == 78 and counted[("eulerOurs", "exact")][0] == 88


def test_density_hidden_inside_obstacles(oracle, exp_ops, cases):
    """non-zero density in obstacle cells (a 3^3 block, and single cells next to the border shell): the tile hides it, every
    block still counts as empty, and the obstacle's neighbours match the oracle"""
    counted = check_case("obstacle_with_density", cases["obstacle_with_density"], oracle, exp_ops)
    assert counted[("maccormackOurs", "exact")] == [96, 96]


@pytest.mark.parametrize("name", ["u_zero", "u_threshold", "u_long", "u_nan_inf"])
def test_velocities_on_an_all_zero_density(oracle, exp_ops, cases, name):
    """u = 0; one lane per wave with a component just below / above T / dt; |u dt| > 0.99 (the generic trace); a NaN and
    two infinite velocity faces (the oracle counts reference error paths there and carries on as the kernels do)"""
    counted = check_case(name, cases[name], oracle, exp_ops, strict=name != "u_nan_inf")
    assert counted[("maccormackOurs", "exact")] == [96, 96]
    if name == "u_threshold":
        lo, hi = Z.threshold_velocities(0.45)
        assert abs(np.float32(lo) * np.float32(Z.DT)) <= np.float32(0.45) < abs(np.float32(hi) * np.float32(Z.DT))


def test_batch_item_empty_next_to_a_dense_one(oracle, exp_ops, cases):
    counted = check_case("item1_dense", cases["item1_dense"], oracle, exp_ops)
    assert counted[("maccormackOurs", "exact")][0] == 48


def test_simulate_is_bit_equal_with_the_switch_on_and_off(tmp_path):
    """12 steps of simulate() (ConvNet projection) on the 48^3 plume scene"""
    res = {}
    for on in (True, False):
        path = str(tmp_path / ("sim_%d.json" % on))
        assert "sim ok" in _child(["sim", path], on)
        res[on] = json.load(open(path))
    for k in ("density", "UDiv", "pDiv"):
        assert res[True][k] == res[False][k], k
    assert res[True]["nonzero_density"] > 0
    assert min(res[True]["counted"]) > 0 and res[False]["counted"] == [0, 0]


def test_two_z_slab_ranks_equal_the_uncut_step():
    out = _child(["slab"], True)
    assert "slab ok" in out
    a, b = (int(v) for v in out.strip().splitlines()[-1].split("counted")[1].split())
    assert a > 0 and b > 0
