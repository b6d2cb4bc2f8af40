"""nn.FluidCriterion on the device: tfluids.criterionWeight / tfluids.fluidCriterion (tfl_criterion_weight, tfl_fluidCriterion,
criterion.hip), criterion.FluidCriterion (autograd) and simulate.calcPUTargets.

The weight and both gradients are held bit-equal (up to the sign of a zero) to the numpy restatement of
tests/criterion_ref.py; the four loss doubles to 1e-10 relative of its exactly summed value (derived there)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import criterion_ref as R
import flavours

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _dev(a, how="aligned"):
    """device tensor of a numpy array; "misaligned": a contiguous view that starts 4 bytes past a 16-byte boundary"""
    import torch
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.array(a, np.float32))          # (a copy: the cases are shared and read-only)
    if how == "misaligned":
        buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    out = t.to(dev)
    assert out.data_ptr() % 16 == 0
    return out


def _like(t, how, fill=None):
    out = _dev(np.zeros(tuple(t.shape), np.float32), how)
    if fill is not None:
        out.fill_(fill)
    return out


def _inputs(name):
    how = R.case(name)[3]
    return [_dev(a, how) for a in R.make_case(name)], how


def _run(ts, how, w, lambdas, sizeAverage=True, grads=True):
    import torch
    from fluidnet_amd import tfluids
    pP, UP, pT, UT, flags = ts
    loss = torch.full((4,), -1.0, dtype=torch.float64, device=pP.device)
    gP = _like(pP, how, 7.0) if grads else None
    gU = _like(UP, how, 7.0) if grads else None
    tfluids.fluidCriterion(pP, UP, pT, UT, flags, w, lambdas[0], lambdas[1], lambdas[2], sizeAverage, loss, gP, gU)
    return loss, gP, gU


def _same(got, want):
    """bit-equal up to the sign of a zero (no NaNs on either side)"""
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    return g.shape == want.shape and not np.isnan(g).any() and bool((g == want).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.NAMES)
def test_weight_is_bit_equal_to_the_restatement(oracle, name):
    import torch
    from fluidnet_amd import tfluids
    (pP, UP, pT, UT, flags), how = _inputs(name)
    want = R.expected(oracle, name, True)["weight"]
    out = _like(flags, how, -3.0)
    got = tfluids.criterionWeight(flags, R.BORDER[1], R.BORDER[0], out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(tfluids.criterionWeight(flags, R.BORDER[1], R.BORDER[0]), got)
    # the starting point is what signedDistanceField writes
    sdf = torch.empty_like(flags)
    tfluids.signedDistanceField(flags, R.BORDER[1], flags.size(2) > 1, sdf)
    assert torch.equal(got == R.BORDER[0], sdf <= 1)


@pytest.mark.gpu
@pytest.mark.parametrize("lam", list(R.LAMBDAS))
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", R.NAMES)
def test_losses_and_gradients_against_the_restatement(oracle, name, weighted, lam):
    import torch
    ts, how = _inputs(name)
    before = [t.clone() for t in ts]
    exp = R.expected(oracle, name, weighted, lam)
    w = _dev(exp["weight"], how) if weighted else None
    lambdas = R.LAMBDAS[lam]
    loss, gP, gU = _run(ts, how, w, lambdas)
    got = loss.cpu().numpy()
    for t in range(4):
        rel = abs(got[t] - exp["loss"][t]) / exp["loss"][t] if exp["loss"][t] else abs(got[t])
        print("criterion %-26s %-8s %-7s loss[%d] = %.17g want %.17g rel %.2e" % (name, "weighted" if weighted else "plain", lam, t, got[t], exp["loss"][t], rel))
    nP = int((gP.cpu().numpy() != exp["gradP"]).sum())
    nU = int((gU.cpu().numpy() != exp["gradU"]).sum())
    print("criterion %-26s %-8s %-7s gradP words off %d / %d, gradU words off %d / %d" % (name, "weighted" if weighted else "plain", lam, nP, gP.numel(), nU, gU.numel()))
    for t in range(4):
        if exp["loss"][t] == 0.0:
            assert got[t] == 0.0, (t, got[t])            # a lambda of 0 leaves its loss at 0
        else:
            assert abs(got[t] - exp["loss"][t]) <= R.LOSS_REL * exp["loss"][t], (t, got[t], exp["loss"][t])
    assert _same(gP, exp["gradP"]) and _same(gU, exp["gradU"]), (nP, nU)
    # the same bits every call; the losses do not depend on whether gradients were asked for; no input was written
    loss2, gP2, gU2 = _run(ts, how, w, lambdas)
    assert torch.equal(loss, loss2) and torch.equal(gP, gP2) and torch.equal(gU, gU2)
    loss3, _, _ = _run(ts, how, w, lambdas, grads=False)
    assert torch.equal(loss, loss3)
    assert all(torch.equal(a, b) for a, b in zip(ts, before))


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", [c[0] for c in R.CASES if c[2] == 2 and c[3] == "aligned"])
def test_a_sample_does_not_depend_on_the_batch(oracle, name, weighted):
    """sizeAverage = 0 (no n in the arithmetic): the gradients of sample b of the B = 2 call are the bits of the B = 1 call on
    that sample, and the B = 1 losses meet the restatement's on that sample (the plane sums are formed per (b, z) alike)."""
    import torch
    ts, how = _inputs(name)
    lambdas = R.LAMBDAS["all"]
    w = _dev(R.expected(oracle, name, True)["weight"]) if weighted else None
    _, gP, gU = _run(ts, how, w, lambdas, sizeAverage=False)
    exp = R.expected(oracle, name, weighted, "all", False)
    assert _same(gP, exp["gradP"]) and _same(gU, exp["gradU"])
    for b in range(2):
        one = [t[b:b + 1].contiguous() for t in ts]
        wb = w[b:b + 1].contiguous() if weighted else None
        loss1, gP1, gU1 = _run(one, how, wb, lambdas, sizeAverage=False)
        assert torch.equal(gP1[0], gP[b]) and torch.equal(gU1[0], gU[b]), (name, b)
        arrs = [a[b:b + 1] for a in R.make_case(name)]
        ref1 = R.criterion(oracle, *arrs, exp["weight"][b:b + 1] if weighted else None, lambdas, False)
        got = loss1.cpu().numpy()
        for t in range(4):
            assert abs(got[t] - ref1["loss"][t]) <= R.LOSS_REL * ref1["loss"][t], (name, b, t)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", [c[0] for c in R.CASES if c[2] == 2 and c[3] == "aligned"])
def test_plane_sums_do_not_depend_on_the_batch(oracle, name, weighted):
    """A batch item's plane sums do not depend on B, held bit for bit through the public entry: with sizeAverage = 0 (no n in
    the arithmetic) and the OTHER sample made to contribute exact zeros (prediction == target, U = 0, so every z and every
    divergence is +-0 and its plane sums are 0.0), the four losses of the B = 2 call are the bits of the B = 1 call on the
    sample that counts -- whichever of the two places in the batch it sits at."""
    import torch
    ts, how = _inputs(name)
    lambdas = R.LAMBDAS["all"]
    w = _dev(R.expected(oracle, name, True)["weight"]) if weighted else None
    for b in range(2):
        pP, UP, pT, UT, flags = [t.clone() for t in ts]
        o = 1 - b
        UP[o].zero_()
        UT[o].zero_()
        pT[o].copy_(pP[o])
        both, _, _ = _run([pP, UP, pT, UT, flags], how, w, lambdas, sizeAverage=False)
        one, _, _ = _run([t[b:b + 1].contiguous() for t in (pP, UP, pT, UT, flags)], how,
                         w[b:b + 1].contiguous() if weighted else None, lambdas, sizeAverage=False)
        print("criterion batch %-26s %-8s sample %d: B=2 %r  B=1 %r" % (name, "weighted" if weighted else "plain", b, both.tolist(), one.tolist()))
        assert float(one[3]) > 1e-3 and torch.equal(both, one), (name, b, both.tolist(), one.tolist())


@pytest.mark.gpu
def test_weight_cache_is_per_tensor_and_a_returned_weight_never_changes(oracle):
    """a NEW flags tensor is a miss even where the caching allocator hands it the freed tensor's address at version 0; so is a
    non-contiguous flags whose contiguous temporary lives at a reused address; a weight returned earlier is never rewritten"""
    import torch
    from fluidnet_amd import FluidCriterion, tfluids
    ts, how = _inputs("3d-short-row-8x12x16-b2")
    flags = ts[4]
    crit = FluidCriterion(1, 1, 1, borderWeight=R.BORDER[0], borderWidth=R.BORDER[1])
    other = flags.clone()
    other[:, :, 3:5, 4:8, 5:11] = 2.0
    want_a = tfluids.criterionWeight(flags, R.BORDER[1], R.BORDER[0])
    want_b = tfluids.criterionWeight(other, R.BORDER[1], R.BORDER[0])
    assert not torch.equal(want_a, want_b)
    a = flags.clone()
    ptr = a.data_ptr()
    wa = crit.weight(a)
    assert crit.weight(a) is wa and torch.equal(wa, want_a)
    del a
    b = other.clone()                                                  # usually lands on the address `a` had, at _version 0
    print("weight cache: the new flags tensor %s the freed one's address" % ("reuses" if b.data_ptr() == ptr else "does not reuse"))
    wb = crit.weight(b)
    assert torch.equal(wb, want_b) and torch.equal(wa, want_a) and wb is not wa
    nc = flags.transpose(3, 4).contiguous().transpose(3, 4)            # same values, not contiguous
    assert not nc.is_contiguous() and torch.equal(nc, flags)
    assert torch.equal(crit.weight(nc), want_a) and torch.equal(wb, want_b)
    assert crit.weight(nc) is crit.weight(nc)
    total = crit((ts[0], ts[1]), (ts[2], ts[3], nc))
    ref, _, _ = _run(ts, how, want_a, (1, 1, 1), grads=False)
    assert torch.equal(total, ref[3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3d-16x24x32", "2d-ragged-33x47-b2"])
def test_module_backward_fills_grad_with_the_entrys_gradients(oracle, name):
    import torch
    from fluidnet_amd import FluidCriterion
    ts, how = _inputs(name)
    pP, UP, pT, UT, flags = ts
    crit = FluidCriterion(*R.LAMBDAS["all"], borderWeight=R.BORDER[0], borderWidth=R.BORDER[1])
    w = crit.weight(flags)
    assert crit.weight(flags) is w                                     # cached per flags tensor and version
    assert np.array_equal(w.cpu().numpy(), R.expected(oracle, name, True)["weight"])
    loss, gP, gU = _run(ts, how, w, R.LAMBDAS["all"])
    p = pP.clone().requires_grad_(True)
    U = UP.clone().requires_grad_(True)
    total = crit((p, U), (pT, UT, flags))
    assert total.dim() == 0 and total.dtype == torch.float64 and total.is_cuda
    assert torch.equal(torch.stack([crit.pLoss, crit.uLoss, crit.divLoss, total.detach()]), loss)
    total.backward()
    assert torch.equal(p.grad, gP) and torch.equal(U.grad, gU)
    # lambdas are plain attributes; grad_output scales the gradients
    crit.divLambda = 0.0
    p.grad = U.grad = None
    (3.0 * crit((p, U), (pT, UT, flags))).backward()
    _, gP0, gU0 = _run(ts, how, w, R.LAMBDAS["div-off"])
    assert float(crit.divLoss) == 0.0 and torch.equal(p.grad, gP0 * 3.0) and torch.equal(U.grad, gU0 * 3.0)
    # no input requires grad: losses only, the same bits
    crit.divLambda = R.LAMBDAS["all"][2]
    assert torch.equal(crit((pP, UP), (pT, UT, flags)), loss[3])
    # the weight follows an in-place change of flags
    f2 = flags.clone()
    w2 = crit.weight(f2).clone()
    f2[0, 0, f2.size(2) // 2, f2.size(3) // 2, 2:6] = 2.0
    assert not torch.equal(crit.weight(f2), w2)


@pytest.mark.gpu
def test_autograd_composes_with_the_tfluids_modules(oracle):
    """the criterion on the output of VelocityUpdate(p, U, flags): p.grad is velocityUpdateBackward of the criterion's gradU; and
    with a VelocityDivergence term of the caller's own next to it the two gradients add"""
    import torch
    from fluidnet_amd import FluidCriterion, modules, tfluids
    ts, how = _inputs("3d-16x24x32")
    pP, UP, pT, UT, flags = ts
    crit = FluidCriterion(*R.LAMBDAS["all"], borderWeight=R.BORDER[0], borderWidth=R.BORDER[1])
    p = pP.clone().requires_grad_(True)
    Uout = modules.VelocityUpdate()((p, UP, flags))
    crit((pT, Uout), (pT, UT, flags)).backward()
    _, _, gU = _run([pT, Uout.detach(), pT, UT, flags], how, crit.weight(flags), R.LAMBDAS["all"])
    want = torch.empty_like(pP)
    tfluids.velocityUpdateBackward(UP, flags, pP, gU, want)
    assert torch.equal(p.grad, want) and float(p.grad.abs().max()) > 0
    U = UP.clone().requires_grad_(True)
    div = modules.VelocityDivergence()((U, flags))
    (crit((pT, U), (pT, UT, flags)) + div.double().sum()).backward()
    _, _, gU2 = _run([pT, UP, pT, UT, flags], how, crit.weight(flags), R.LAMBDAS["all"])
    gD = torch.empty_like(UP)
    tfluids.velocityDivergenceBackward(UP, flags, torch.ones_like(flags), gD)
    assert torch.equal(U.grad, gU2 + gD)                               # (a two-term sum: the order autograd adds in does not matter)


@pytest.mark.gpu
def test_captured_call_replays_to_the_same_bits(oracle):
    import torch
    name = "3d-ragged-13x17x23-b2"
    ts, how = _inputs(name)
    w = _dev(R.expected(oracle, name, True)["weight"])
    first = _run(ts, how, w, R.LAMBDAS["all"])                         # warm-up: the scratch exists before the capture
    from fluidnet_amd import tfluids
    loss = torch.zeros(4, dtype=torch.float64, device=w.device)
    gP, gU = torch.zeros_like(ts[0]), torch.zeros_like(ts[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tfluids.fluidCriterion(*ts, w, *R.LAMBDAS["all"], True, loss, gP, gU)
    for t in (loss, gP, gU):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, first[0]) and torch.equal(gP, first[1]) and torch.equal(gU, first[2])
    ts[1].mul_(1.5)                                                    # new data in place
    want = _run(ts, how, w, R.LAMBDAS["all"])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, want[0]) and torch.equal(gU, want[2]) and not torch.equal(loss, first[0])


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    import torch
    from fluidnet_amd import TfluidsError, tfluids
    ts, how = _inputs("3d-short-row-8x12x16-b2")
    pP, UP, pT, UT, flags = ts
    before = [t.clone() for t in ts]
    loss = torch.full((4,), -1.0, dtype=torch.float64, device=pP.device)
    gP, gU = torch.full_like(pP, 7.0), torch.full_like(UP, 7.0)

    def refused(*args):
        with pytest.raises(TfluidsError):
            tfluids.fluidCriterion(*args)
        torch.cuda.synchronize()
        assert bool((loss == -1.0).all()) and bool((gP == 7.0).all()) and bool((gU == 7.0).all())
        assert all(torch.equal(a, b) for a, b in zip(ts, before))
    refused(pP, UP, pT, UT, flags, None, 1, 1, 1, True, loss, gP, UP)           # gradU aliases UPred
    refused(pP, UP, pT, UT, flags, None, 1, 1, 1, True, loss, gP, UT)           # ... UTarget
    refused(pP, UP, pT, UT, flags, None, 1, 1, 1, True, loss, pP, gU)           # gradP aliases an input
    refused(pP, UP, pT, UT, flags, None, 1, 1, 1, True, loss, flags, gU)
    refused(pP, UP, pT, UT, flags, None, 1, 1, 1, True, loss, gP, None)         # both or neither
    refused(pP, UP, pT[:1].contiguous(), UT, flags, None, 1, 1, 1, True, loss, gP, gU)            # batch size
    refused(pP, UP[:, :2].contiguous(), pT, UT[:, :2].contiguous(), flags, None, 1, 1, 1, True, loss, gP, gU)      # 2 channels, depth > 1
    refused(pP, UP, pT, UT[..., :-1].contiguous(), flags, None, 1, 1, 1, True, loss, gP, gU)      # xdim
    refused(pP, UP, pT, UT, flags, flags[..., :-1].contiguous(), 1, 1, 1, True, loss, gP, gU)     # weight
    refused(pP, UP, pT, UT, flags.cpu(), None, 1, 1, 1, True, loss, gP, gU)                          # a CPU pointer among device tensors
    refused(pP, UP, pT.cpu(), UT, flags, None, 1, 1, 1, True, loss, gP, gU)
    from fluidnet_amd import FluidCriterion
    with pytest.raises(TfluidsError):
        FluidCriterion(1, 1, 1)((pP, UP), (pT, UT, flags.cpu()))
    # the C entry's own "both or neither" (the Python layer refuses before it): straight through the C ABI
    import ctypes
    lib, ctx = tfluids._context(UP)
    n = int(lib.tfl_fluid_criterion_workspace_floats(*[int(v) for v in (flags.size(0), flags.size(2), flags.size(3), flags.size(4))]))
    ws, = tfluids.getTempStorage(UP, [(n,)])
    for gp, gu in ((tfluids._tt(gP), None), (None, tfluids._tt(gU))):
        rc = lib.tfl_fluidCriterion(ctx, tfluids._tt(pP), tfluids._tt(UP), tfluids._tt(pT), tfluids._tt(UT), tfluids._tt(flags), None, 1.0, 1.0,
                                    1.0, 1, 1, ctypes.c_void_p(loss.data_ptr()), gp, gu, ctypes.c_void_p(ws.data_ptr()), n)
        assert rc != 0 and b"both or neither" in lib.tfl_last_error(ctx)
    torch.cuda.synchronize()
    assert bool((loss == -1.0).all()) and bool((gP == 7.0).all()) and bool((gU == 7.0).all())
    out = torch.full_like(flags, -3.0)
    for bw, bwt in ((1, 2.0), (2.5, 2.0), (3, 1.0), (3, 0.5), (1025, 2.0)):
        with pytest.raises(TfluidsError):
            tfluids.criterionWeight(flags, bw, bwt, out=out)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


@pytest.mark.gpu
def test_calc_pu_targets(oracle):
    import torch
    import scenes
    from fluidnet_amd import TfluidsError, calcPUTargets
    sc = scenes.make_scene((12, 16, 20), seed=71, vel_cells=0.4)
    f, U0 = sc["flags"], sc["U"]

    def host(solve):
        U = U0.copy()
        oracle.setWallBcsForward(U, f)
        div = np.zeros_like(f)
        oracle.velocityDivergenceForward(U, f, div)
        p = np.zeros_like(f)
        solve(p, div)
        Ut = U.copy()
        oracle.velocityUpdateForward(Ut, f, p)
        oracle.setWallBcsForward(Ut, f)
        return p, Ut, U, div

    def device(mconf):
        batch = dict(UDiv=_dev(U0), flags=_dev(f), pTarget=_dev(np.zeros_like(f)), UTarget=_dev(np.zeros_like(U0)))
        calcPUTargets(None, mconf, batch)
        div = batch["div"]
        calcPUTargets(None, mconf, batch)                                      # batch["div"] is kept between calls
        assert batch["div"] is div
        return batch
    p, Ut, Ubc, div = host(lambda p, div: oracle.solveLinearSystemJacobi(p, f, div, True, 0.0, 8))
    b = device(dict(trainTargetSource="jacobi", maxIter=8))
    assert _same(b["pTarget"], p) and _same(b["UTarget"], Ut) and _same(b["UDiv"], Ubc) and _same(b["div"], div)
    assert np.abs(p).max() > 0
    p, Ut, _, _ = host(lambda p, div: oracle.solveLinearSystemPCG(p, f, div, True, 1e-4, 100, "ic0"))
    b = device(dict(trainTargetSource="pcg"))
    err, scale = np.abs(b["pTarget"].cpu().numpy() - p).max(), np.abs(p).max()
    print("calcPUTargets pcg: max |p - p_oracle| = %.3e, max |p| = %.3e, relative %.3e" % (err, scale, err / scale))
    assert err <= 5e-5 * scale, (err, scale)
    with pytest.raises(TfluidsError, match="manta"):
        calcPUTargets(None, dict(trainTargetSource="manta"), {})
    with pytest.raises(TfluidsError):
        calcPUTargets(None, dict(trainTargetSource="other"), dict(b))


@pytest.mark.gpu
def test_two_launches_both_from_criterion_hip(oracle):
    from fluidnet_amd import _kernels, tfluids
    ts, how = _inputs("3d-16x24x32")
    w = tfluids.criterionWeight(ts[4], R.BORDER[1], R.BORDER[0])
    _run(ts, how, w, R.LAMBDAS["all"])
    with tfluids.profile(ts[0]) as prof:
        _run(ts, how, w, R.LAMBDAS["all"])
    assert sorted(k for k in prof.kernels if k.startswith("k_")) == ["k_criterion_finish", "k_criterion_planes"], prof.kernels
    assert all(_kernels.source_of(k) == "criterion.hip" for k in prof.kernels if k.startswith("k_"))


@pytest.mark.gpu
def test_experiments_flavour_runs_this_file_green():
    """the second library flavour (libtfluids_hip_exp.so) carries the same kernels: this file in a child process against it"""
    if flavours.is_experiments_process():
        return
    assert os.path.exists(flavours.EXP_LIB), "fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                         env=dict(os.environ, TFL_LIBRARY=flavours.EXP_LIB), capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
