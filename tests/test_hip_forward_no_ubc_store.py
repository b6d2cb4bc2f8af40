"""The one-call forward without the store of SetWallBcs(UDiv) (fluidnet_amd/csrc/model.hip header).

tfl_model_forward of a net without a UDiv input channel leaves U_bc in registers: k_bcs_div_stats does not write it, and the
projection reads the caller's un-masked velocity -- its last step zeroes the very components the wall BCs zero. The two-call
form (tfl_model_begin + tfl_model_finish) still stores U_bc into UOut and reads it back, so it is the yardstick here:
  * (p, U) of the one-call forward are the two-call form's, bit for bit, on every conv path of the product library, with and
    without the flags' wall plan, in place (UDiv == UOut) and with a separate UOut that starts out as NaN, on grids that take
    the four-cells-per-thread kernels and on one with odd X that takes the scalar ones;
  * NaN and +-inf in input components that the wall decision zeroes change nothing: finite outputs, the bits of the run with
    those components set to 0;
  * U_bc is still where its readers look for it: tfl_model_begin leaves it in UOut, a net with a UDiv input channel reads it
    there (one-call forward, separate NaN-filled UOut), and the z-slab step of such a net equals the un-cut step."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

# (Z, Y, X): rows of 5 / 2 four-cell vectors, several blocks in y and z; X = 9 takes the scalar forms of both kernels (no plan)
GRIDS = [(16, 12, 20), (8, 8, 8), (6, 7, 9)]
PATHS = [None, "mfma", "winograd", "direct"]


def scene(dims, seed=5, B=1):
    """stick obstacles inside the walls, the +y face an outflow face, white-noise U and p, a plume pair on U"""
    Z, Y, X = dims
    rng = np.random.RandomState(seed)
    flags = scenes.empty_domain(B, Z, Y, X, True)
    flags[:, :, Z // 2:Z // 2 + 2, Y // 3:Y // 3 + 3, X // 4:X // 4 + 3] = scenes.OBSTACLE | scenes.STICK
    flags[:, :, 1:3, Y // 2:Y // 2 + 2, X - 4:X - 2] = scenes.OBSTACLE | scenes.STICK
    flags[:, :, 1:-1, Y - 1, 1:-1] = scenes.EMPTY | scenes.OUTFLOW
    U = rng.randn(B, 3, Z, Y, X).astype(np.float32)
    p = (0.1 * rng.randn(B, 1, Z, Y, X)).astype(np.float32)
    bc = np.zeros_like(U)
    inv = np.ones_like(U)
    inv[:, :, :, 1:3, :] = 0.0
    zz, xx = np.meshgrid(np.arange(Z), np.arange(X), indexing="ij")
    disk = ((zz - Z // 2) ** 2 + (xx - X // 2) ** 2 <= (X // 4) ** 2).astype(np.float32)
    bc[:, 1, :, 1:3, :] = disk[None, :, None, :]
    return dict(flags=flags, U=U, p=p, UBC=bc, UBCInvMask=inv)


def wall_zeroed(oracle, flags):
    """True where setWallBcs zeroes the component (it writes 0 there and leaves every other word alone)"""
    ones = np.ones((flags.shape[0], 3) + flags.shape[2:], np.float32)
    oracle.setWallBcsForward(ones, flags)
    return ones == 0.0


class Run:
    """one model on one device scene: the one-call forward and the two-call form on the SAME flags tensor (its wall plan)"""

    def __init__(self, model, sc, plan, monkeypatch):
        import torch
        from fluidnet_amd import simulate, tfluids
        self.torch, self.model = torch, model
        dev = torch.device("cuda:0")
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
        monkeypatch.setattr(simulate, "_WALL_PLANS", bool(plan))
        lib, ctx = tfluids._context(self.t["flags"])
        got = [simulate.wall_plan(lib, ctx, self.t["flags"]) for _ in range(2)][-1]      # (created at the second sighting)
        assert (got is not None) == bool(plan)

    def pair(self):
        return dict(UBC=self.t["UBC"], UBCInvMask=self.t["UBCInvMask"], clamp=(-1e6, 1e6))

    def forward(self, U, inplace):
        torch, t = self.torch, self.t
        Uin = torch.from_numpy(U).to(t["p"].device)
        Uout = Uin if inplace else torch.full_like(Uin, float("nan"))
        pout = torch.full_like(t["p"], float("nan"))
        self.model.forward([t["p"], Uin, t["flags"]], out=[pout, Uout], **self.pair())
        if not inplace:
            assert np.array_equal(Uin.cpu().numpy().view(np.uint32), U.view(np.uint32))        # the input is only read
        return pout.cpu().numpy(), Uout.cpu().numpy()

    def begin(self, U):
        torch, t = self.torch, self.t
        Ub = torch.from_numpy(U).to(t["p"].device)
        stats = torch.zeros(U.shape[0], 2, dtype=torch.float64, device=Ub.device)
        self.model.begin(Ub, t["flags"], 0, U.shape[2], stats)
        return Ub, stats

    def two_calls(self, U):
        t = self.t
        Ub, stats = self.begin(U)
        pb = t["p"].clone()
        self.model.finish(pb, Ub, t["flags"], stats, float(np.prod(U.shape[1:])), **self.pair())
        return pb.cpu().numpy(), Ub.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("plan", [True, False], ids=["wall_plan", "flag_words"])
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("env", PATHS, ids=lambda e: e or "mfma16")
def test_forward_equals_begin_plus_finish(oracle, monkeypatch, env, dims, plan):
    from fluidnet_amd import FluidNetModel
    if env:
        monkeypatch.setenv("TFL_CONV_PATH", env)
    else:
        monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    sc = scene(dims)
    run = Run(FluidNetModel.default_3d(seed=3), sc, plan, monkeypatch)
    p_ref, U_ref = run.two_calls(sc["U"])
    assert np.isfinite(p_ref).all() and np.isfinite(U_ref).all()
    zeroed = wall_zeroed(oracle, sc["flags"])
    assert zeroed.any() and (U_ref[zeroed & (sc["UBCInvMask"] == 1.0)] == 0.0).all()
    for inplace in (True, False):
        p, U = run.forward(sc["U"], inplace)
        assert same_bits(p, p_ref), (env, dims, plan, inplace, int((p != p_ref).sum()))
        assert same_bits(U, U_ref), (env, dims, plan, inplace, int((U != U_ref).sum()))
    # NaN / +inf / -inf in every component the wall decision zeroes, against the run with 0 there
    U0, Un = sc["U"].copy(), sc["U"].copy()
    U0[zeroed] = 0.0
    Un[zeroed] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(zeroed.sum()))
    p0, V0 = run.forward(U0, True)
    assert same_bits(p0, p_ref) and same_bits(V0, U_ref)           # (SetWallBcs makes the two inputs the same field)
    for inplace in (True, False):
        p, U = run.forward(Un, inplace)
        assert np.isfinite(p).all() and np.isfinite(U).all(), (env, dims, plan, inplace)
        assert same_bits(p, p0) and same_bits(U, V0), (env, dims, plan, inplace)


@pytest.mark.parametrize("plan", [True, False], ids=["wall_plan", "flag_words"])
def test_begin_still_leaves_u_bc_in_uout(oracle, monkeypatch, plan):
    from fluidnet_amd import FluidNetModel
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    sc = scene(GRIDS[0])
    run = Run(FluidNetModel.default_3d(seed=3), sc, plan, monkeypatch)
    Ub, _ = run.begin(sc["U"])
    want = sc["U"].copy()
    oracle.setWallBcsForward(want, sc["flags"])
    assert (want != sc["U"]).any() and same_bits(Ub.cpu().numpy(), want)


@pytest.mark.parametrize("plan", [True, False], ids=["wall_plan", "flag_words"])
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_a_net_with_a_udiv_input_still_reads_u_bc(monkeypatch, dims, plan):
    """its one-call forward keeps the store: with a separate UOut that starts out as NaN the net would read NaN otherwise"""
    from fluidnet_amd import FluidNetModel
    monkeypatch.delenv("TFL_CONV_PATH", raising=False)
    sc = scene(dims)
    run = Run(FluidNetModel.from_mconf(dict(inputChannels=dict(UDiv=True)), True, seed=2), sc, plan, monkeypatch)
    p_ref, U_ref = run.two_calls(sc["U"])
    assert np.isfinite(p_ref).all() and np.isfinite(U_ref).all()
    for inplace in (True, False):
        p, U = run.forward(sc["U"], inplace)
        assert same_bits(p, p_ref) and same_bits(U, U_ref), (dims, plan, inplace)


def test_z_slab_step_of_a_udiv_input_net_equals_uncut():
    """two ranks: the UDiv channels of the net input come from what tfl_model_begin left in UOut's owned planes"""
    import test_hip_slab_models as SM
    SM.test_model_opts_slabs_equal_uncut("UDiv-input", 2)


def test_step_whose_velocity_sits_in_the_workspace_keeps_the_store(oracle):
    """tfl_simulate_step without a confinement force hands the projection the advection's scratch velocity, which lies in the
    workspace the conv stack overwrites: that call has to store U_bc (the projection would read conv activations otherwise).
    Three steps of the 24^3 plume scene against the numpy / C restatement of the step."""
    import torch
    import bench
    from fluidnet_amd import FluidNetModel
    from fluidnet_amd.simulate import simulate_native
    from oracle import simulate_np as S
    batch, mconf = bench.build_scene(24, 24, None, torch.device("cuda:0"))
    mconf = dict(mconf, vorticityConfinementAmp=0)
    model = FluidNetModel.default_3d(seed=1)
    nb = {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in batch.items()}
    for _ in range(3):
        simulate_native(None, mconf, batch, model)
        S.simulate(oracle, mconf, nb, model.layers)
    for k in ("pDiv", "UDiv", "density"):
        got = batch[k].cpu().numpy()
        assert np.isfinite(got).all() and scenes.rel_l2(got, nb[k]) <= 1e-5, (k, scenes.rel_l2(got, nb[k]))
