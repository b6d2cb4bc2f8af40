"""The numpy restatement of the optimiser step (tests/optim_ref.py) before tests/test_hip_optim.py relies on it: its fp32 form,
rounded where tfl_optim_step rounds, stays inside the bound on every test input, and each broken variant leaves it -- so the
bound has room for fp32 arithmetic and for nothing else."""
import numpy as np
import pytest

import optim_ref as O


@pytest.mark.parametrize("kind,method,clip", O.CASES)
def test_fp32_restatement_is_inside_the_bound(kind, method, clip):
    cfg = O.config(method, clip)
    want = O.trajectory(kind, cfg, np.float64)
    got = O.trajectory(kind, cfg, np.float32)
    wx, ws = O.check(got, want, O.parameters(kind), method == O.ADAM)
    print("%s %s clip=%s: fp32 worst error/bound %.3f, worst state rel-L2 %.2e" % (kind, method, clip, wx, ws))
    assert wx <= 1.0 and ws <= O.BAR
    if clip:      # the case is what it claims: the clip acted (the gradients came back smaller)
        assert O.l2(np.concatenate([a.ravel() for a in want[0][1]])) < 0.5 * O.l2(np.concatenate([a.ravel() for a in O.gradients(kind, 0)]))


# every (case, variant) pair in which the variant changes something the configuration computes
BROKEN = [(k, m, c, v) for k, m, c in O.CASES for v in O.VARIANTS if O.applies(v, O.config(m, c))]


def test_every_variant_is_exercised():
    assert {v for _, _, _, v in BROKEN} == set(O.VARIANTS) and len(BROKEN) >= 24


@pytest.mark.parametrize("kind,method,clip,variant", BROKEN)
def test_broken_variants_leave_the_bound(kind, method, clip, variant):
    cfg = O.config(method, clip)
    want = O.trajectory(kind, cfg, np.float64)
    got = O.trajectory(kind, cfg, np.float64, variant)
    wx, ws = O.check(got, want, O.parameters(kind), method == O.ADAM)
    assert wx > 1.0 or ws > O.BAR, (variant, wx, ws)


def test_state_and_counter():
    """RMSprop's mean square starts at initialMean; t counts steps; clr reads t before the increment (step 1 runs at lr)"""
    cfg = O.config(O.RMSPROP, False)
    st = O.new_state(O.parameters("yang"), cfg)
    assert all((m == cfg["initialMean"]).all() for m in st["m"])
    cfg = dict(O.config(O.ADAM, False), weightDecay=0.0, epsilon=0.0)
    x = [np.zeros(3)]
    st = O.new_state(x, cfg)
    x1, _ = O.step(x, [np.array([1.0, -2.0, 0.5])], st, cfg)
    assert st["t"] == 1 and np.allclose(x1[0], -cfg["learningRate"] * np.array([1.0, -1.0, 1.0]), rtol=1e-12)
