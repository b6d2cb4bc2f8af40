"""CPU-side checks of the divergence-norm rollout (tfl_velocityDivergenceNorm, tfl_slab_divergence_norm, stats.calcStats):
the three layers agree on the new entries, the expected value of the GPU tests (tests/divnorm_ref.py) is sound and non-trivial on
every case the GPU tests use, CPU tensors are refused, and divnorm.hip compiles for gfx950 the way a streaming kernel must.
(The 128^3 case of tests/test_hip_divnorm.py starts from three GPU steps; its `exact > 1e-3` is asserted there.)"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import divnorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidnet_amd", "csrc")
NEW = ("tfl_divergence_norm_workspace_floats", "tfl_velocityDivergenceNorm", "tfl_slab_divergence_norm")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _args(s):
    return [a for a in s.split(",") if a.strip()]


def test_header_python_and_lua_declare_the_same_entries():
    from fluidnet_amd import _lib
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
    assert "function M.velocityDivergenceNorm(U, flags)" in lua and "function Slab:divergenceNorm()" in lua
    assert "BIT FOR BIT" in open(os.path.join(ROOT, "include", "tfluids_hip.h")).read()
    from fluidnet_amd import _kernels
    assert _kernels.KERNEL_SOURCE["k_divnorm_planes"] == _kernels.KERNEL_SOURCE["k_divnorm_finish"] == "divnorm.hip"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdivnorm\.hip\b", mk, re.M)       # one list feeds both flavours


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_exact_norm_is_sound_and_not_trivial(oracle, name):
    U, flags = R.make_case(name)
    exact = R.exact_norm(oracle, U, flags)
    div = np.zeros_like(flags)
    oracle.velocityDivergenceForward(U, flags, div)
    for b in range(flags.shape[0]):
        ref = np.linalg.norm(div[b].astype(np.float64).ravel())
        assert abs(exact[b] - ref) <= 1e-12 * ref, (name, b, exact[b], ref)
        assert exact[b] > R.MIN_EXACT, (name, b, exact[b])
    if flags.shape[0] == 2:
        assert exact[0] != exact[1]
    assert (flags[..., 1:-1, 1:-1] == 2).any(), "no obstacle inside the walls"


def test_cpu_tensors_are_refused():
    import torch
    from fluidnet_amd import TfluidsError, stats, tfluids
    U, flags = torch.zeros(1, 2, 1, 8, 8), torch.ones(1, 1, 1, 8, 8)
    with pytest.raises(TfluidsError):
        tfluids.velocityDivergenceNorm(U, flags)
    batch = dict(pDiv=torch.zeros(1, 1, 1, 8, 8), UDiv=U, flags=flags, density=torch.zeros(1, 1, 1, 8, 8))
    with pytest.raises(TfluidsError):
        stats.calcStats(dict(dt=0.1, simMethod="jacobi", maxIter=2), batch, None, 3)


@needs_hipcc
def test_divnorm_compiles_without_scratch_and_loads_in_one_batch(tmp_path):
    """no scratch memory, no spills in any kernel of divnorm.hip; the fast stage-1 kernel never drains its load queue while loads
    of its own are still to come (counted by tools/isa_loads.py as tests/test_isa_cpu.py does)"""
    asm = str(tmp_path / "divnorm.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-I" + os.path.join(ROOT, "include"), "--offload-device-only", "-S", "-o", asm,
                           os.path.join(CSRC, "divnorm.hip")], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    kernels = re.findall(r"\.name:\s+(\S*k_divnorm\S*)\n(.*?)\.wavefront_size", text, re.S)
    names = {k for k, _ in kernels if not k.endswith(".kd")}
    assert len(names) == 5, names          # two forms x (2-D, 3-D) of stage 1, and stage 2
    for k, meta in kernels:
        for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
            m = re.search(r"\.%s:\s+(\d+)" % key, meta)
            assert m and int(m.group(1)) == 0, (k, key, m and m.group(1))
    assert "scratch_" not in re.sub(r";.*", "", text).replace(".amdhsa_enable_private_segment", "")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_loads.py"), r"^k_divnorm_planes_v4<", os.path.join(CSRC, "divnorm.hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    found = re.findall(r"^(\S.*?)\s+(\d+) loads,\s+(\d+) full drains", out.stdout, re.M)
    assert sorted(f[0] for f in found) == ["k_divnorm_planes_v4<false>", "k_divnorm_planes_v4<true>"], out.stdout
    for k, loads, drains in found:
        assert int(loads) >= 10 and int(drains) == 0, (k, loads, drains, out.stdout)
