"""fluidnet_amd.run_epoch.plan_batch (the random decisions of torch/lib/run_epoch.lua:133-158, 243-258) against a scripted rng
that records every draw, and the manta refusal of simulate.dataAugmentation (simulate.lua:378-380). No GPU."""
import copy
import itertools

import pytest

from fluidnet_amd import TfluidsError, dataAugmentation
from fluidnet_amd.run_epoch import RandomStateRng, plan_batch


class Scripted:
    """uniform() / randint() / randn() hand out the scripted values in turn and log (kind, args, value)"""

    def __init__(self, uniform=(), randint=(), randn=()):
        self._u, self._i, self._n = list(uniform), list(randint), list(randn)
        self.log = []

    def uniform(self):
        v = self._u.pop(0)
        self.log.append(("uniform", (), v))
        return v

    def randint(self, lo, hi):
        v = self._i.pop(0)
        assert lo <= v <= hi
        self.log.append(("randint", (lo, hi), v))
        return v

    def randn(self):
        v = self._n.pop(0)
        self.log.append(("randn", (), v))
        return v


def _mconf(**over):
    m = dict(dt=0.1, buoyancyScale=0, gravityScale=0, vorticityConfinementAmp=0, gravity=[0.0, 1.0, 0.0],
             trainBuoyancyProb=0.5, trainBuoyancyScale=2.0, trainGravityProb=0.5, trainGravityScale=3.0,
             trainVorticityConfinementProb=0.5, trainVorticityConfinementAmp=0.8,
             longTermDivLambda=1, longTermDivNumSteps=[4, 16], longTermDivProbability=0.9, timeScaleSigma=1,
             optimState=dict(learningRate=0.0025, nested=[1, 2, 3]))
    m.update(over)
    return m


def _kinds(rng):
    return [(k, a) for k, a, _ in rng.log]


@pytest.mark.parametrize("on", list(itertools.product([False, True], repeat=3)), ids=lambda on: "".join("BGV"[i] if v else "-" for i, v in enumerate(on)))
def test_draw_order_and_count_for_every_combination(on):
    """draws below 0.5 switch a force on: three uniforms first, the gravity axis and sign only when buoyancy or gravity ended
    up on, then randn and the fourth uniform of the long-term pass"""
    buoy, grav, vort = on
    mconf = _mconf()
    before = copy.deepcopy(mconf)
    rng = Scripted(uniform=[0.1 if buoy else 0.9, 0.1 if grav else 0.9, 0.1 if vort else 0.9, 0.5], randint=[3, 0], randn=[-0.25])
    plan = plan_batch(mconf, rng, True)
    want = [("uniform", ())] * 3
    if buoy or grav:
        want += [("randint", (1, 3)), ("randint", (0, 1))]
    want += [("randn", ()), ("uniform", ())]
    assert _kinds(rng) == want
    assert plan["buoyancyScale"] == (2.0 if buoy else 0)
    assert plan["gravityScale"] == (3.0 if grav else 0)
    assert plan["vorticityConfinementAmp"] == (0.8 if vort else 0)
    assert plan["gravity"] == ([0.0, 0.0, -1.0] if (buoy or grav) else [0.0, 1.0, 0.0])
    assert plan["numFutureSteps"] == 4
    assert mconf == before
    assert set(plan) == {"buoyancyScale", "gravityScale", "vorticityConfinementAmp", "gravity", "dt", "numFutureSteps"}


def test_a_scale_already_on_in_mconf_draws_the_gravity_too():
    """run_epoch.lua:152 reads the scales as they END UP: a standing gravityScale > 0 draws a direction with all three
    probability draws failing; the sign 1 gives +1"""
    rng = Scripted(uniform=[0.9, 0.9, 0.9, 0.5], randint=[1, 1], randn=[0.0])
    plan = plan_batch(_mconf(gravityScale=0.5), rng)
    assert _kinds(rng)[3:5] == [("randint", (1, 3)), ("randint", (0, 1))]
    assert plan["gravity"] == [1.0, 0.0, 0.0] and plan["gravityScale"] == 0.5


def test_no_gravity_draw_when_both_scales_stay_zero():
    rng = Scripted(uniform=[0.9, 0.9, 0.1, 0.5], randn=[0.3])
    plan = plan_batch(_mconf(), rng)
    assert not any(k == "randint" for k, _ in _kinds(rng))
    assert plan["gravity"] == [0.0, 1.0, 0.0] and plan["vorticityConfinementAmp"] == 0.8


@pytest.mark.parametrize("x,sigma", [(-0.25, 1), (1.7320508, 0.3), (-3.1e-3, 2.5), (0.0, 1)])
def test_the_timescale_to_the_last_bit(x, sigma):
    rng = Scripted(uniform=[0.9, 0.9, 0.9, 0.5], randn=[x])
    plan = plan_batch(_mconf(timeScaleSigma=sigma, dt=0.1), rng)
    assert plan["dt"] == 0.1 * (0.2028 + abs(x * sigma))


def test_no_timescale_draw_without_a_sigma():
    rng = Scripted(uniform=[0.9, 0.9, 0.9, 0.5])
    plan = plan_batch(_mconf(timeScaleSigma=0), rng)
    assert _kinds(rng) == [("uniform", ())] * 4 and plan["dt"] == 0.1


@pytest.mark.parametrize("draw,steps", [(0.89, 4), (0.9, 4), (0.91, 16)])
def test_both_branches_of_the_long_term_probability(draw, steps):
    """run_epoch.lua:254-258: the second count only when the draw is ABOVE longTermDivProbability"""
    rng = Scripted(uniform=[0.9, 0.9, 0.9, draw], randn=[0.1])
    assert plan_batch(_mconf(), rng)["numFutureSteps"] == steps


@pytest.mark.parametrize("over", [dict(longTermDivLambda=0), dict(longTermDivNumSteps=None)], ids=["lambda0", "no-table"])
def test_no_long_term_draws_when_the_pass_is_off(over):
    mconf = _mconf(**over)
    before = copy.deepcopy(mconf)
    rng = Scripted(uniform=[0.1, 0.9, 0.9], randint=[2, 0])
    plan = plan_batch(mconf, rng, False)
    assert _kinds(rng) == [("uniform", ())] * 3 + [("randint", (1, 3)), ("randint", (0, 1))]
    assert plan["numFutureSteps"] == 0 and plan["dt"] == 0.1 and plan["gravity"] == [0.0, -1.0, 0.0]
    assert mconf == before


def test_the_default_rng_is_seeded_and_in_range():
    a, b = RandomStateRng(7), RandomStateRng(7)
    m = _mconf(trainBuoyancyProb=1.0)
    plans = [plan_batch(m, a) for _ in range(50)]
    assert plans == [plan_batch(m, b) for _ in range(50)]
    axes = {tuple(p["gravity"]) for p in plans}
    assert all(sorted(abs(v) for v in g) == [0.0, 0.0, 1.0] for g in axes) and len(axes) == 6      # both ends of both ranges
    assert {p["numFutureSteps"] for p in plans} <= {4, 16} and all(p["dt"] >= 0.1 * 0.2028 for p in plans)


def test_data_augmentation_refuses_manta_targets():
    with pytest.raises(TfluidsError, match="target source is manta, this method should not be called!"):
        dataAugmentation(None, dict(trainTargetSource="manta"), {})
