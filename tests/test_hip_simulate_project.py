"""GPU checks of tfl_simulate_project / simulate.project (csrc/simulate.cpp): the projection phase of the step as its own entry.
An outputDiv step followed by project() leaves the bits of ONE full step -- for pcg, jacobi and convnet (seeded default nets), in
2-D and 3-D, with a plume BC pair and without, over two consecutive steps; against the native step and the Python orchestration
alike; and the state between the two calls is the outputDiv state."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(1, 16, 24), (8, 12, 16)]
METHODS = ["pcg", "jacobi", "convnet"]


def _batch(dims, plume, seed):
    """a closed box with a sphere obstacle, a smooth-ish random velocity and density; plume: createPlumeBCs' U and density pairs"""
    from fluidnet_amd import tfluids
    from fluidnet_amd.simulate import createPlumeBCs
    Z, Y, X = dims
    is3D = Z > 1
    C = 3 if is3D else 2
    rng = np.random.RandomState(seed)
    flags = torch.empty(1, 1, Z, Y, X, device=DEV)
    tfluids.emptyDomain(flags, is3D)
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    blob = (i - 0.6 * X) ** 2 + (j - 0.6 * Y) ** 2 + ((k - 0.5 * Z) ** 2 if is3D else 0) <= (0.15 * min(Y, X)) ** 2
    flags[0, 0][torch.from_numpy(blob).to(DEV) & (flags[0, 0] == 1)] = 2.0
    fluid = (flags == 1).float()
    U = torch.from_numpy((rng.randn(1, C, Z, Y, X) * 0.8).astype(np.float32)).to(DEV)
    tfluids.setWallBcsForward(U, flags)
    density = torch.from_numpy(rng.uniform(0, 1, (1, 1, Z, Y, X)).astype(np.float32)).to(DEV) * fluid
    p = torch.from_numpy((rng.randn(1, 1, Z, Y, X) * 0.1).astype(np.float32)).to(DEV) * fluid
    b = dict(pDiv=p.contiguous(), UDiv=U, flags=flags, density=density.contiguous())
    if plume:
        createPlumeBCs(b, [1.0], 1.5, 0.2)
    return b


def _clone(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _model(method, is3D):
    if method != "convnet":
        return None
    from fluidnet_amd import FluidNetModel
    return FluidNetModel.default_3d(seed=1) if is3D else FluidNetModel.from_mconf(dict(modelType="default"), False, seed=1)


@pytest.mark.parametrize("plume", [True, False], ids=["plume", "no-bc"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dims", GRIDS, ids=["2d", "3d"])
def test_outputdiv_step_plus_project_is_the_full_step(dims, method, plume):
    from fluidnet_amd.simulate import project, simulate, simulate_native
    is3D = dims[0] > 1
    model = _model(method, is3D)
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, buoyancyScale=1.0, gravityScale=0,
                 vorticityConfinementAmp=0.5, simMethod=method, maxIter=20)
    base = _batch(dims, plume, seed=dims[1])
    full, split, split_py, eager = _clone(base), _clone(base), _clone(base), _clone(base)
    for step in range(2):
        simulate_native(None, mconf, full, model)
        simulate(None, mconf, eager, model)
        # the state between the two calls is the outputDiv state of the full step's input
        before = _clone(split)
        simulate_native(None, mconf, split, model, outputDiv=True)
        simulate_native(None, mconf, before, model, outputDiv=True)
        for k in ("pDiv", "UDiv", "density"):
            assert torch.equal(split[k], before[k]), (step, k)
        project(None, mconf, split, model)
        simulate(None, mconf, split_py, model, outputDiv=True)
        project(None, mconf, split_py, model)
        for k in ("pDiv", "UDiv", "density"):
            assert torch.isfinite(full[k]).all(), (step, k)
            assert torch.equal(split[k], full[k]), (step, k, "native outputDiv + project vs native step")
            assert torch.equal(split_py[k], full[k]), (step, k, "python outputDiv + project vs native step")
            assert torch.equal(eager[k], full[k]), (step, k, "python step vs native step")
    assert float(full["UDiv"].abs().max()) > 0.05 and float((full["UDiv"] - base["UDiv"]).abs().max()) > 1e-3


def test_project_refuses_what_the_step_refuses():
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.simulate import project
    b = _batch((1, 16, 24), False, seed=1)
    keep = _clone(b)
    with pytest.raises(TfluidsError, match="not a valid option"):
        project(None, dict(dt=0.1, simMethod="multigrid"), b)
    with pytest.raises(TfluidsError, match="needs a model"):
        project(None, dict(dt=0.1, simMethod="convnet"), b)
    torch.cuda.synchronize()
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(b[k], keep[k]), k


def test_refusals_inherited_from_the_steps_validation_carry_the_entrys_name():
    """a banked model's grid factor (3 mres banks: 4) against a grid it does not divide: refused before anything is written,
    under `simulate_project` from project() and under `simulate_step` from the step"""
    from fluidnet_amd import FluidNetModel, TfluidsError
    from fluidnet_amd.simulate import project, simulate_native
    model = FluidNetModel.from_mconf(dict(banksNum=3, banksType="mres", banksAggregateMethod="concat", banksSplitStage=2, banksJoinStage=4),
                                     True, seed=1)
    b = _batch((16, 24, 30), False, seed=2)
    keep = _clone(b)
    mconf = dict(dt=0.1, advectionMethod="maccormackOurs", maccormackStrength=0.6, simMethod="convnet")
    with pytest.raises(TfluidsError, match="simulate_project: the grid is not divisible by the model's downsampling factor 4"):
        project(None, mconf, b, model)
    with pytest.raises(TfluidsError, match="simulate_step: the grid is not divisible by the model's downsampling factor 4"):
        simulate_native(None, mconf, b, model)
    torch.cuda.synchronize()
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(b[k], keep[k]), k
