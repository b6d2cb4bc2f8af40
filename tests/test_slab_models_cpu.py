"""CPU checks of the z-slab cone of the projection nets (fluidnet_amd.dist.model_cone, the Python statement of the walk behind
tfl_slab_halo_model) against an EMPIRICAL cone of the PyTorch-CPU restatement of the net
(tests/model_graph_ref.graph_stack): perturbing the net input one plane beyond the cone leaves pPred on the owned planes and
the plane below them (what the velocity update reads) unchanged, and perturbing it on the last plane the cone claims -- before
the rounding to the downsampling factor -- changes them. For the default, yang, tog and a k5 / pressure-skip table."""
import numpy as np
import pytest

from fluidnet_amd import FluidNetModel, TfluidsError
from fluidnet_amd.dist import model_cone
from oracle import simulate_np as S


def _k5_skip():
    rng = np.random.RandomState(4)
    shapes = [(8, 3, 5), (8, 8, 3), (1, 9, 1)]
    layers = [((rng.randn(co, ci, k, k, k) * 0.3).astype(np.float32), (rng.randn(co) * 0.01).astype(np.float32))
              for co, ci, k in shapes]
    return FluidNetModel(layers, True, opts=dict(addPressureSkip=True))


MODELS = {
    "default": lambda: FluidNetModel(S.default_3d_layers(seed=3), True),
    "yang": lambda: FluidNetModel.from_mconf(dict(modelType="yang"), True, seed=3),
    "tog": lambda: FluidNetModel.tog(True, seed=3),
    "k5-skip": _k5_skip,
}


def test_cone_numbers():
    """the worked numbers of DESIGN.md 6d"""
    c = model_cone(MODELS["default"]())
    assert (c["input"], c["depth"], c["F"], c["halo"]) == ((4, 3), 4, 1, 4)
    c = model_cone(MODELS["yang"]())
    assert (c["input"], c["depth"], c["F"], c["halo"]) == ((2, 1), 2, 1, 2)
    c = model_cone(MODELS["tog"]())
    assert (c["input"], c["depth"], c["F"], c["halo"]) == ((15, 15), 15, 4, 16)
    assert [L["d"] for L in c["layers"]] == [1, 2, 4, 4, 4, 4, 2]
    assert [L["conv"] for L in c["layers"]] == [(14, 14), (6, 6), (2, 2), (1, 1), (1, 1), (1, 1), (1, 0)]
    c = model_cone(MODELS["k5-skip"]())
    assert (c["input"], c["depth"], c["F"], c["halo"]) == ((4, 3), 4, 1, 4)


def test_graph_and_2d_models_have_no_cone():
    with pytest.raises(TfluidsError, match="un-sharded"):
        model_cone(FluidNetModel.from_mconf(dict(banksNum=2, banksType="dilate"), True))
    with pytest.raises(TfluidsError, match="2-D"):
        model_cone(FluidNetModel.tog(False))


def _pred(model, x):
    import model_graph_ref as R
    skip = x[:, :1] if model.opts["addPressureSkip"] else None     # the joined channel is pDiv / scale: x's channel 0
    return R.graph_stack(x, model, "float64", skip)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_cone_matches_the_empirical_cone(name):
    model = MODELS[name]()
    c = model_cone(model)
    lo, hi = c["input"]
    F = c["F"]
    o0, o1 = 8 * F, 16 * F                         # owned planes, on the downsampling factor
    Z = o1 + 8 * F
    rng = np.random.RandomState(7)
    in_c = model.layers[0][0].shape[1]
    x = rng.randn(1, in_c, Z, 8, 8).astype(np.float64)
    base = _pred(model, x)
    need = slice(o0 - 1, o1)                        # pPred on the owned planes widened by (1, 0)

    def moved(z):
        y = x.copy()
        y[:, :, z] += 3.0 * rng.randn(*y[:, :, z].shape)
        return float(np.abs(_pred(model, y)[:, :, need] - base[:, :, need]).max())

    assert moved(o0 - lo - 1) == 0.0 and moved(o1 + hi) == 0.0, "the cone misses planes the owned pressure reads"
    assert moved(o0 - lo) > 0.0 and moved(o1 + hi - 1) > 0.0, "the cone claims planes the owned pressure does not read"
