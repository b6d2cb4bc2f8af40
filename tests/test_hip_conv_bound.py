"""Every projection ConvNet path of tfl_model_forward against the per-voxel fp64 error bound of tests/conv_bound.py: at every
voxel of every batch sample |p - p64| <= bound_p and |U - U64| <= bound_U; where velocityUpdate leaves U alone, U equals the
restatement bit for bit; nothing clamps at the fp16 range; and the aggregate fp64 witness stays within 4x PyTorch-CPU
fp32's error. Shapes sit around each path's tile edges (mfma16 32x8 columns / 32x4x4 tiles, conv_mfma 32x8x4, Winograd
64 x 2 VY x 4 with x-pairs, conv2d_mfma 32x4); inputs are smooth and rough scenes, adversarial weights and magnitudes at
the ends of the input-scale branch and of fp16's range. Each case prints max(err / bound), the slack left."""
import time

import numpy as np
import pytest

import conv_bound as CB
import model_graph_ref as R
import scenes
from flavours import experiments_flavour
from oracle import simulate_np as S

pytestmark = pytest.mark.gpu
BUDGET_S = 120          # per case: the fp64 CPU reference dominates


def _layers2d():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "myModel2D_weights.npz"))
    return [(z["w%d" % i], z["b%d" % i]) for i in range(5)]


def _mconf(n, bt, agg, bn, **kw):
    m = dict(banksNum=n, banksType=bt, banksAggregateMethod=agg, banksSplitStage=2, banksJoinStage=4)
    m.update(kw)
    if bn != "off":
        m.update(addBatchNorm=True, batchNormAffine=bn == "affine")
    return m


def _scene(kind, dims, B, seed):
    if kind == "smooth":
        return scenes.make_scene(dims, seed=seed, vel_cells=0.4, B=B)
    return scenes.rough_scene(dims, seed=seed, B=B)


def _scale_to(sc, targets, oracle):
    """U (and p with it) of each sample scaled so that its input scale (the std of U_bc) lands at targets[b]"""
    U = sc["U"].copy()
    ops = oracle
    Ub = U.copy()
    ops.setWallBcsForward(Ub, sc["flags"])
    s = S.input_scale(Ub).astype(np.float64)
    for b, t in enumerate(targets):
        sc["U"][b] = (U[b] * (t / s[b])).astype(np.float32)
        sc["p"][b] = (sc["p"][b] * (t / s[b])).astype(np.float32)
    Ub = sc["U"].copy()
    ops.setWallBcsForward(Ub, sc["flags"])
    return S.input_scale(Ub)


def check(oracle, model, sc, env_path=None, name="", tile=(32, 8, 4), expect_no_clamp=True):
    """forward on the GPU (the model created under the current environment) and every assertion of the module"""
    import torch
    t0 = time.time()
    dev = torch.device("cuda:0")
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    p, U = model.forward([tp, tU, tf])
    clamps = model.range_errors(tp)
    p, U = p.cpu().numpy(), U.cpu().numpy()
    path = CB.conv_path(model, env_path)
    p64, U64, bp, bU, info = CB.forward_bound(oracle, model, sc["p"], sc["U"], sc["flags"], path=path)
    if model.graph is None:
        p_ref, U_ref = S.model_forward(oracle, model.layers, sc["p"], sc["U"], sc["flags"], pool=model.pool, up=model.up,
                                       opts=model.opts)
    else:
        p_ref, U_ref = R.model_forward(oracle, model, sc["p"], sc["U"], sc["flags"])
    rp, _ = CB.worst(p, p64, bp)
    rU, _ = CB.worst(U, U64, bU)
    ew, et = scenes.rel_l2(p, p64), scenes.rel_l2(p_ref, p64)
    print("%-44s %-8s max err/bound p %.3g U %.3g | witness %.2e vs fp32 %.2e | scale %s | %.1fs"
          % (name, path, rp, rU, ew, et, " ".join("%.4g" % v for v in info["scale"]), time.time() - t0))
    assert np.isfinite(p).all() and np.isfinite(U).all(), name
    for b in range(p.shape[0]):
        assert CB.worst(p[b:b + 1], p64[b:b + 1], bp[b:b + 1])[0] <= 1.0, CB.report(name + " p", p[b:b + 1], p64[b:b + 1], bp[b:b + 1], tile)
        assert CB.worst(U[b:b + 1], U64[b:b + 1], bU[b:b + 1])[0] <= 1.0, CB.report(name + " U", U[b:b + 1], U64[b:b + 1], bU[b:b + 1], tile)
    m = info["untouched"]
    assert np.array_equal(U[m], U_ref[m]), (name, int((U[m] != U_ref[m]).sum()))
    if expect_no_clamp:
        assert clamps == 0, (name, clamps)
    # the default-topology kernels within 4x of PyTorch-CPU fp32's error; the shape-generic ones (conv.hip: one fmaf chain
    # over up to 1600 terms, where PyTorch sums in short blocks) with the 1e-7 floor test_hip_simulate.py's tog test and
    # test_hip_model_graph.py already give them -- their per-voxel bound above is the sharp check
    assert ew <= 4.0 * et + (1e-8 if path != "fp32" or env_path == "direct" else 1e-7), (name, ew, et)
    assert time.time() - t0 <= BUDGET_S, (name, time.time() - t0)
    return rp, rU


# ---- the 3-D default topology on its four paths, around the tile edges --------------------------------------------------
SHAPES3 = [((5, 9, 33), 3, "rough"), ((3, 7, 65), 1, "smooth"), ((2, 3, 17), 1, "rough"), ((9, 17, 63), 1, "smooth"),
           ((3, 9, 130), 3, "smooth"), ((5, 3, 31), 3, "rough")]


@pytest.mark.parametrize("env", [None, "mfma", "winograd", "direct"])
def test_default_3d_every_path(oracle, monkeypatch, env):
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    model = FluidNetModel.default_3d(seed=3)
    for i, (dims, B, kind) in enumerate(SHAPES3):
        check(oracle, model, _scene(kind, dims, B, 100 + i), env, "default3d %s %s B=%d" % (kind, dims, B))


def test_default_3d_many_blocks(oracle, monkeypatch):
    from fluidnet_amd import FluidNetModel
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    check(oracle, FluidNetModel.default_3d(seed=3), _scene("rough", (40, 128, 128), 1, 120), None, "default3d rough 40x128x128")


@pytest.mark.parametrize("env", [None, "direct"])
def test_default_2d_every_path(oracle, monkeypatch, env):
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    model = FluidNetModel(_layers2d(), False)
    for i, (dims, B, kind) in enumerate([((1, 17, 130), 3, "rough"), ((1, 9, 31), 1, "smooth"), ((1, 3, 33), 1, "rough"),
                                         ((1, 7, 65), 3, "smooth")]):
        check(oracle, model, _scene(kind, dims, B, 130 + i), env, "default2d %s %s B=%d" % (kind, dims, B), tile=(32, 4, 1))


# ---- the other topologies (generic and graph kernels) -------------------------------------------------------------------
OTHER = {
    "tog3d": (lambda F: F.tog(True, seed=9), (4, 8, 32)),
    "tog2d": (lambda F: F.tog(False, seed=9), (1, 16, 66)),
    "yang3d": (lambda F: F.from_mconf(dict(modelType="yang"), True, seed=4), (5, 9, 33)),
    "yang2d": (lambda F: F.from_mconf(dict(modelType="yang"), False, seed=4), (1, 17, 65)),
    "relu6": (lambda F: F.from_mconf(dict(nonlinType="relu6"), True, seed=2), (5, 9, 33)),
    "sigmoid": (lambda F: F.from_mconf(dict(nonlinType="sigmoid"), True, seed=2), (5, 9, 33)),
    "skip": (lambda F: F.from_mconf(dict(addPressureSkip=True), True, seed=2), (3, 7, 17)),
    "norm": (lambda F: F.from_mconf(dict(normalizeInputFunc="norm"), True, seed=2), (3, 7, 17)),
    "udiv_input": (lambda F: F.from_mconf(dict(inputChannels=dict(UDiv=True)), True, seed=2), (3, 7, 17)),
    "mres_concat_affine": (lambda F: F.from_mconf(_mconf(2, "mres", "concat", "affine"), True, seed=2), (4, 8, 32)),
    "dilate_add_plain": (lambda F: F.from_mconf(_mconf(2, "dilate", "add", "plain"), True, seed=3), (5, 9, 33)),
    "tog_banks_max": (lambda F: F.from_mconf(dict(modelType="tog", banksNum=2, banksSplitStage=2, banksJoinStage=5,
                                                  poolType="max", addBatchNorm=True), True, seed=9), (8, 16, 32)),
}


@pytest.mark.parametrize("name", sorted(OTHER))
def test_other_topologies(oracle, monkeypatch, name):
    from fluidnet_amd import FluidNetModel
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    build, dims = OTHER[name]
    model = build(FluidNetModel)
    for kind, B, seed in (("smooth", 1, 140), ("rough", 3, 141)):
        check(oracle, model, _scene(kind, dims, B, seed), None, "%s %s %s B=%d" % (name, kind, dims, B))


# ---- adversarial weights and magnitudes on the 3-D default paths --------------------------------------------------------
EDGES = {"max=8": 8.0, "max=16": 16.0, "max=2^-10": 2.0 ** -10}


def _adversarial_weights(which):
    layers = [(w.copy(), b.copy()) for w, b in S.default_3d_layers(seed=3)]
    rng = np.random.RandomState(11)
    if which == "loguniform":                  # one layer's magnitudes spread over 1e-4 .. 1
        w = layers[1][0]
        layers[1] = ((np.sign(rng.randn(*w.shape)) * 10.0 ** rng.uniform(-4, 0, w.shape)).astype(np.float32), layers[1][1])
    elif which in EDGES:                       # max |w| exactly on a power of two (frexpf's edges) in layer 1 and the
        mx = EDGES[which]                      # tail's 8 -> 8, the layer after each scaled back (ReLU is homogeneous)
        for li in (1, 3):
            (w, b), (wn, bn) = layers[li], layers[li + 1]
            k = mx / float(np.abs(w).max())
            w = (w * k).astype(np.float32)
            w.flat[int(np.argmax(np.abs(w)))] = np.float32(mx)
            layers[li] = (w, (b * k).astype(np.float32))
            layers[li + 1] = ((wn / k).astype(np.float32), bn)
    elif which == "zero_channel":              # one output channel of all-zero weights
        w, b = layers[1]
        w = w.copy()
        w[3] = 0.0
        layers[1] = (w, b)
    elif which == "bias_only":                 # all zeros but the bias: the mx == 0 branch of the weight packing
        w, b = layers[2]
        layers[2] = (np.zeros_like(w), (np.abs(b) + 0.05).astype(np.float32))
    return layers


@pytest.mark.parametrize("env", [None, "winograd", "mfma"])
@pytest.mark.parametrize("which", ["loguniform", "max=8", "max=16", "max=2^-10", "zero_channel", "bias_only"])
def test_adversarial_weights(oracle, monkeypatch, env, which):
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    model = FluidNetModel(_adversarial_weights(which), True)
    for kind, dims, B, seed in (("rough", (5, 9, 33), 2, 150), ("smooth", (3, 7, 65), 1, 151)):
        check(oracle, model, _scene(kind, dims, B, seed), env, "weights %s %s %s B=%d" % (which, kind, dims, B))


SCALES = {"2^-13": [2.0 ** -13], "under 2^-12": [2.0 ** -12 * (1 - 1e-3)], "over 2^-12": [2.0 ** -12 * (1 + 1e-3)],
          "under 2^21": [2.0 ** 21 * (1 - 1e-3)], "over 2^21": [2.0 ** 21 * (1 + 1e-3)], "2^22": [2.0 ** 22],
          "in and out": [0.5, 2.0 ** 22]}


@pytest.mark.parametrize("env", [None, "winograd", "mfma", "direct"])
def test_input_scale_branches(oracle, monkeypatch, env):
    """the per-sample input scale on both sides of the [2^-12, 2^21] branch of the first layer, B = 2 with one sample in
    range and one out"""
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    model = FluidNetModel.default_3d(seed=3)
    for i, (name, targets) in enumerate(SCALES.items()):
        sc = _scene("rough", (5, 9, 33), len(targets), 160 + i)
        s = _scale_to(sc, targets, oracle)
        for b, t in enumerate(targets):
            assert (2.0 ** -12 <= s[b] <= 2.0 ** 21) == (2.0 ** -12 <= t <= 2.0 ** 21), (name, s, targets)
        check(oracle, model, sc, env, "scale %s" % name)


@pytest.mark.parametrize("env", [None, "winograd"])
def test_fp16_range_edges(oracle, monkeypatch, env):
    """mfma16's operands near both ends of fp16: a net input of about 3e4, hidden activations of 1e4 .. 5e4 (the largest
    clear of 65504 after rounding), and a region whose activations sit in fp16's subnormal range"""
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    base = S.default_3d_layers(seed=3)
    # pDiv large: |pDiv / scale| up to 3e4
    sc = _scene("smooth", (5, 9, 33), 1, 170)
    Ub = sc["U"].copy()
    oracle.setWallBcsForward(Ub, sc["flags"])
    s = float(S.input_scale(Ub)[0])
    sc["p"] = (sc["p"] / np.abs(sc["p"]).max() * 3e4 * s).astype(np.float32)
    model = FluidNetModel([(w.copy(), b.copy()) for w, b in base], True)
    *_, info = CB.forward_bound(oracle, model, sc["p"], sc["U"], sc["flags"], path="fp32")
    assert max(info["acts"]) < 6e4, info["acts"]
    check(oracle, model, sc, env, "net input 3e4")
    # hidden activations up to about 4e4: the first layer scaled (ReLU is positively homogeneous)
    sc = _scene("rough", (5, 9, 33), 2, 171)
    *_, info = CB.forward_bound(oracle, FluidNetModel(base, True), sc["p"], sc["U"], sc["flags"], path="fp32")
    f = np.float32(4e4 / max(info["acts"][:3]))
    layers = [((base[0][0] * f).astype(np.float32), (base[0][1] * f).astype(np.float32))] + [(w.copy(), b.copy()) for w, b in base[1:]]
    model = FluidNetModel(layers, True)
    *_, info = CB.forward_bound(oracle, model, sc["p"], sc["U"], sc["flags"], path="fp32")
    assert 1e4 <= max(info["acts"]) <= 5.5e4, info["acts"]
    check(oracle, model, sc, env, "activations %.3g" % max(info["acts"]))
    # a subnormal region: p and U 1e-6 of the rest in a box, so that the first layer's p / div operands there (< 2^-14) split
    # into halves in fp16's subnormal range
    sc = _scene("rough", (9, 17, 33), 1, 172)
    sc["p"][..., 2:7, 3:12, 5:25] *= 1e-6
    sc["U"][..., 2:7, 3:12, 5:25] *= 1e-6
    check(oracle, FluidNetModel(base, True), sc, env, "subnormal region")


# ---- the kernel forms of the EXPERIMENTS flavour (child process, libtfluids_hip_exp.so) ----------------------------------
EXP_FORMS = [dict(TFL_M16_TILED="3"), dict(TFL_M16_FUSE12="1", TFL_M16_CZ_F2="1"), dict(TFL_M16_FUSE12="1", TFL_M16_CZ_F2="3"),
             dict(TFL_M16_PIPE="0"), dict(TFL_M16_TAIL_MFMA="0"), dict(TFL_M16_CZ="1", TFL_M16_CZ_IN="1"), dict(TFL_M16_CZ="3", TFL_M16_CZ_IN="3")]


@experiments_flavour
def test_experiments_flavour_forms(oracle, monkeypatch):
    from fluidnet_amd import FluidNetModel
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    for form in EXP_FORMS:
        for k, v in form.items():
            monkeypatch.setenv(k, v)
        model = FluidNetModel.default_3d(seed=3)
        for i, (dims, B, kind) in enumerate([((5, 9, 33), 3, "rough"), ((9, 17, 63), 1, "smooth"), ((7, 7, 17), 1, "rough")]):
            check(oracle, model, _scene(kind, dims, B, 180 + i), None, "%s %s %s B=%d" % (form, kind, dims, B))
        for k in form:
            monkeypatch.delenv(k)
