"""What the tests of the generator's batched form share (tests/test_datagen_batched_cpu.py, tests/test_hip_datagen_batched.py;
DESIGN.md 3.25): the plans every GPU test draws its batch items from -- seed 11, runs 0 .. 7 of the two GEN_CASES shapes -- and
the mix of forces and emitters those plans are held to on the CPU, so that the GPU tests cannot silently lose it."""
SEED = 11
RUNS = 8
CASES = [(False, (1, 32, 32)), (True, (12, 16, 20))]
STEP_PLANS = (0, 3, 4, 6)      # the batch items of the step tests


def gconf(is3D, dims, **over):
    from fluidnet_amd import datagen
    kw = dict(steps=12, saveEvery=2)
    kw.update(over)
    return datagen.default_gconf(is3D, dims, **kw)


def plans(is3D, dims, runs=range(RUNS), **over):
    from fluidnet_amd import datagen
    g = gconf(is3D, dims, **over)
    return [datagen.plan_run(g, SEED, r) for r in runs]


def mix(plan_list):
    """(gravity axes, runs with buoyancy, runs with confinement, emitters per run) of a list of plans"""
    axes = [tuple(p["gravity"]) for p in plan_list]
    buoy = [i for i, p in enumerate(plan_list) if p["buoyancyScale"] > 0]
    vort = [i for i, p in enumerate(plan_list) if p["vorticityConfinementAmp"] > 0]
    emit = [len(p["emitters"]) for p in plan_list]
    return axes, buoy, vort, emit
