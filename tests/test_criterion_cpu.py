"""CPU-side checks of the fused criterion (tfl_criterion_weight, tfl_fluidCriterion, criterion.FluidCriterion,
simulate.calcPUTargets): the three layers agree on the new entries, CPU tensors are refused, the numpy restatement the GPU
tests compare against (tests/criterion_ref.py) is sound and non-trivial on every case, and criterion.hip compiles for gfx950
without scratch memory or spills."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import criterion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidnet_amd", "csrc")
NEW = ("tfl_criterion_weight", "tfl_fluid_criterion_workspace_floats", "tfl_fluidCriterion")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _args(s):
    return [a for a in s.split(",") if a.strip()]


def test_header_python_and_lua_declare_the_same_entries():
    from fluidnet_amd import _kernels, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfluids_hip.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "fluidnet_amd", "lua", "tfluids_hip.lua")).read()
    lua_body = re.sub(r"--[^\n]*", "", lua[lua.index("]]", lua.index("ffi.cdef[[")):])
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/tfluids_hip.h"
        n = len(_args(m.group(1)))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
        c = re.search(r"lib\.%s\(" % name, lua_body)
        assert c, "tfluids_hip.lua does not call " + name
        depth, j = 1, c.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(lua_body[j], 0)
            j += 1
        call, depth, cnt = lua_body[c.end():j - 1], 0, 1
        for ch in call:
            depth += {"(": 1, ")": -1}.get(ch, 0)
            cnt += ch == "," and depth == 0
        assert cnt == n, (name, cnt, n)
    assert "function M.criterionWeight(" in lua and "function M.FluidCriterion(" in lua
    assert re.search(r"#define\s+TFL_ABI_VERSION\s+4\b", open(os.path.join(ROOT, "include", "tfluids_hip.h")).read())
    for k in ("k_criterion_weight", "k_criterion_planes", "k_criterion_finish"):
        assert _kernels.KERNEL_SOURCE[k] == "criterion.hip"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bcriterion\.hip\b", mk, re.M)       # one list feeds both flavours


def test_package_exports():
    import fluidnet_amd
    from fluidnet_amd import criterion, simulate
    assert fluidnet_amd.FluidCriterion is criterion.FluidCriterion and fluidnet_amd.calcPUTargets is simulate.calcPUTargets
    c = fluidnet_amd.FluidCriterion(1, 1, 1)
    assert c.sizeAverage is True and c.borderWeight == 1 and c.weight(None) is None
    with pytest.raises(fluidnet_amd.TfluidsError):
        fluidnet_amd.FluidCriterion(1, 1, 1, borderWeight=2)                      # no width
    with pytest.raises(fluidnet_amd.TfluidsError):
        fluidnet_amd.FluidCriterion(1, 1, 1, borderWeight=2, borderWidth=1)
    with pytest.raises(fluidnet_amd.TfluidsError):
        fluidnet_amd.FluidCriterion(1, 1, 1, borderWeight=2, borderWidth=2.5)


def test_cpu_tensors_are_refused():
    import torch
    from fluidnet_amd import FluidCriterion, TfluidsError, calcPUTargets, tfluids
    p, U, flags = torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 2, 1, 8, 8), torch.ones(1, 1, 1, 8, 8)
    with pytest.raises(TfluidsError):
        tfluids.criterionWeight(flags, 3, 2.0)
    with pytest.raises(TfluidsError):
        tfluids.fluidCriterion(p, U, p.clone(), U.clone(), flags, None, 1, 1, 1, True, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TfluidsError):
        FluidCriterion(1, 1, 1)((p, U), (p.clone(), U.clone(), flags))
    with pytest.raises(TfluidsError):
        FluidCriterion(1, 1, 1, 2.0, 3)((p, U), (p.clone(), U.clone(), flags))
    batch = dict(UDiv=U, flags=flags, pTarget=p.clone(), UTarget=U.clone())
    with pytest.raises(TfluidsError):
        calcPUTargets(None, dict(trainTargetSource="jacobi", maxIter=2), batch)
    with pytest.raises(TfluidsError, match="manta"):
        calcPUTargets(None, dict(trainTargetSource="manta"), batch)


def _autograd(name, w, lambdas):
    """torch-CPU fp64 autograd of the plain formula: lambda mean((w x - w t)^2) per term; the divergence as differences"""
    import torch
    pP, UP, pT, UT, flags = (torch.from_numpy(np.array(a, np.float64)) for a in R.make_case(name))
    pP.requires_grad_(True)
    UP.requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)) if w is not None else torch.ones_like(flags)
    is3d = UP.shape[1] == 3
    fluid = (flags.long() & 1) != 0
    inner = torch.zeros_like(fluid)
    if is3d:
        inner[:, :, 1:-1, 1:-1, 1:-1] = True
    else:
        inner[:, :, :, 1:-1, 1:-1] = True
    div = torch.zeros_like(flags)
    div[..., :-1] += UP[:, 0:1, :, :, :-1] - UP[:, 0:1, :, :, 1:]
    div[..., :-1, :] += UP[:, 1:2, :, :-1, :] - UP[:, 1:2, :, 1:, :]
    if is3d:
        div[:, :, :-1] += UP[:, 2:3, :-1] - UP[:, 2:3, 1:]
    div = div * (fluid & inner)
    pl, ul, dl = lambdas
    lp = pl * ((wt * pP - wt * pT) ** 2).mean() if pl > 0 else torch.zeros((), dtype=torch.float64)
    lu = ul * ((wt * UP - wt * UT) ** 2).mean() if ul > 0 else torch.zeros((), dtype=torch.float64)
    ld = dl * ((wt * div) ** 2).mean() if dl > 0 else torch.zeros((), dtype=torch.float64)
    total = lp + lu + ld
    total.backward()
    gP = pP.grad.numpy() if pP.grad is not None else np.zeros(pP.shape)
    return [float(v.detach()) for v in (lp, lu, ld, total)], gP, UP.grad.numpy()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_is_sound_and_not_trivial(oracle, name, weighted):
    import scenes
    pP, UP, pT, UT, flags = R.make_case(name)
    for lam, lambdas in R.LAMBDAS.items():
        exp = R.expected(oracle, name, weighted, lam)
        loss, gP, gU = _autograd(name, exp["weight"], lambdas)
        for t in range(4):
            print("criterion ref %-26s %-8s %-7s loss[%d] = %.12e  autograd %.12e" % (name, "weighted" if weighted else "plain", lam, t, exp["loss"][t], loss[t]))
            assert abs(exp["loss"][t] - loss[t]) <= 1e-5 * abs(loss[t]), (name, lam, t, exp["loss"][t], loss[t])
            if t < 3:
                assert (exp["loss"][t] > 1e-6) if lambdas[t] > 0 else (exp["loss"][t] == 0.0), (name, lam, t, exp["loss"][t])
        if lambdas[0] > 0:
            assert scenes.rel_l2(exp["gradP"], gP) <= 1e-5, (name, lam, scenes.rel_l2(exp["gradP"], gP))
        else:
            assert not exp["gradP"].any()
        assert scenes.rel_l2(exp["gradU"], gU) <= 1e-5, (name, lam, scenes.rel_l2(exp["gradU"], gU))
        is3d = flags.shape[2] > 1
        inner = np.zeros(flags.shape, bool)
        inner[(slice(None), slice(None), slice(1, -1) if is3d else slice(None), slice(1, -1), slice(1, -1))] = True
        fluid = inner & ((flags.astype(np.int64) & 1) != 0)
        nz = (exp["gradU"] != 0).any(axis=1, keepdims=True)
        assert nz[fluid].mean() > 0.5, (name, lam, nz[fluid].mean())
    if weighted:
        w = R.expected(oracle, name, True)["weight"]
        assert len(np.unique(w)) >= 3 and w.min() >= 1.0 and w.max() == R.BORDER[0], np.unique(w)
    assert (flags[..., 1:-1, 1:-1] == 2).any(), "no obstacle inside the walls"
    if flags.shape[0] == 2:
        assert not np.array_equal(pP[0], pP[1])


def test_checker_pieces_equal_the_compiled_reference(oracle, ref):
    """the three tfluids pieces the restatement takes from the C checker, against the reference's own sources compiled here"""
    for name in ("3d-16x24x32", "2d-ragged-33x47-b2"):
        a = R.expected(oracle, name, True)
        pP, UP, pT, UT, flags = R.make_case(name)
        b = R.criterion(ref, pP, UP, pT, UT, flags, R.weight(ref, flags, *R.BORDER), R.LAMBDAS["all"])
        assert np.array_equal(R.weight(ref, flags, *R.BORDER), a["weight"])
        assert a["loss"] == b["loss"] and np.array_equal(a["gradP"], b["gradP"]) and np.array_equal(a["gradU"], b["gradU"])


@needs_hipcc
def test_criterion_hip_compiles_without_scratch_or_spills(tmp_path):
    """every kernel of criterion.hip: no private segment, no SGPR or VGPR spills (the code object's metadata)"""
    asm = str(tmp_path / "criterion.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-I" + os.path.join(ROOT, "include"), "--offload-device-only", "-S", "-o", asm,
                           os.path.join(CSRC, "criterion.hip")], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    kernels = re.findall(r"\.name:\s+(\S*k_criterion\S*)\n(.*?)\.wavefront_size", text, re.S)
    names = {k for k, _ in kernels if not k.endswith(".kd")}
    # stage 1: two forms x (2-D, 3-D) x (losses only, with gradients) x (plain, weighted); the weight; stage 2
    assert len(names) == 18, names
    for k, meta in kernels:
        for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
            m = re.search(r"\.%s:\s+(\d+)" % key, meta)
            assert m and int(m.group(1)) == 0, (k, key, m and m.group(1))
