"""CPU-only guard on a code-generation property the streaming kernels depend on: a guarded load
(`if (ok) v = *p`) compiles to a branch whose join waits for vmcnt(0), so guarded loads written back to back run one memory
round trip after the other (k_confine_v4 had 20 such drains between its 30 loads, k_project_v4 16, k_pcg_apply 14). The
kernels below were rewritten to load unconditionally and select the value; this test cross-compiles them for gfx950 (hipcc,
no GPU) and counts, in the ISA, the full drains that are followed by further loads (tools/isa_loads.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidnet_amd", "csrc")

# kernel (demangled prefix) -> (source file, most full drains allowed before its last load; the value before round 4's rewrite)
CASES = {
    "k_project_v4<true, false>": ("model.hip", 0, 18),
    "k_project_v4<true, true>": ("model.hip", 0, 18),             # (round 6: on the flags' wall codes, tfl_wall_plan)
    "k_bcs_div_stats_code<true>": ("model.hip", 0, 17),
    "k_bcs_div_stats_v4<true, false>": ("model.hip", 0, 17),     # (<.., true> = the opt-in ticket tail, model.hip)
    "k_curl_v4<true>": ("vorticity.hip", 0, 11),
    "k_pcg_apply<true>": ("pcg.hip", 0, 14),
    "k_jacobi<true, false>": ("jacobi.hip", 0, 1),
    "k_jacobi<false, false>": ("jacobi.hip", 0, 1),
    "k_conv2_mfma<16, false, false>": ("conv2d_mfma.hip", 0, 8),
    "k_minmax3_v4<false>": ("advect.hip", 0, 24),
    "k_velocity_update<true>": ("stencil.hip", 0, 5),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_streaming_kernels_issue_their_loads_in_one_batch():
    by_file = {}
    for k, (f, _, _) in CASES.items():
        by_file.setdefault(f, []).append(k)
    found = {}
    for f, kernels in by_file.items():
        pat = "|".join("^" + re.escape(k) + "$" for k in kernels)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_loads.py"), pat, os.path.join(CSRC, f)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for line in out.stdout.splitlines():
            m = re.match(r"^(\S.*?)\s+(\d+) loads,\s+(\d+) full drains", line)
            if m:
                found[m.group(1).strip()] = (int(m.group(2)), int(m.group(3)))
    for k, (f, allowed, before) in CASES.items():
        assert k in found, (k, sorted(found))
        loads, drains = found[k]
        assert loads >= 4 and drains <= allowed, "%s (%s): %d full drains between its %d loads (%d before the rewrite)" % (k, f, drains, loads, before)


# advectVel's 3-D tile kernels (advect_vel3_kernels.hpp): the registers and SGPR spills of each, as built from commit a0b1164 --
# the last one that kept the one-plane kernels as a verbatim copy beside the templated two-plane ones, which is what the copy
# was protecting (a one-trip plane loop at depth 1 costs pass A 13 VGPRs: 67 instead of 54, and an occupancy step).
# kernel (demangled, namespaces stripped) -> (VGPRs, SGPR spills) at a0b1164; k_vel3_bwd_fold<FAST, BUOY> was kz1::k_vel3_bwd<FAST, BUOY>
VEL3_AT_A0B1164 = {
    "k_vel3_fwd<1, true>": (54, 0), "k_vel3_fwd<1, false>": (54, 0),
    "k_vel3_bwd_fold<true, 2>": (78, 66), "k_vel3_bwd_fold<false, 2>": (73, 66),
    "k_vel3_bwd_fold<true, 7>": (73, 68), "k_vel3_bwd_fold<false, 7>": (73, 72),
    "k_vel3_bwd_fold<true, 0>": (72, 60), "k_vel3_bwd_fold<false, 0>": (70, 60),
    "k_vel3_fwd<2, true>": (64, 34), "k_vel3_fwd<2, false>": (63, 34),
    "k_vel3_bwd<2, true>": (95, 72), "k_vel3_bwd<2, false>": (94, 73),
}


def _makefile_flags(obj):
    """the hipcc flags the Makefile compiles build/<obj> with: FLAGS plus what the target adds"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)).split()
    for m in re.finditer(r"^(\$\(HERE\)build/.*): FLAGS \+= (.*)$", mk, re.M):
        if "$(HERE)build/" + obj in m.group(1).split():
            flags += m.group(2).split()
    return flags


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_advect_vel3_kernels_keep_their_registers():
    flags = _makefile_flags("advect_vel3.o")
    assert "-fno-slp-vectorize" in flags and "--offload-arch=gfx950" in flags, flags
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "advect_vel3.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    found, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name":
            name = subprocess.run(["c++filt", val.strip()], capture_output=True, text=True).stdout.strip()
            cur = found.setdefault(re.sub(r"\(.*", "", re.sub(r"^void |\(anonymous namespace\)::|\w+::", "", name)), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    assert sorted(found) == sorted(VEL3_AT_A0B1164), sorted(found)
    for k, (vgprs, sspill) in VEL3_AT_A0B1164.items():
        print("%-28s VGPRs %s (a0b1164: %d)  SGPR spills %s (%d)" % (k, found[k]["VGPRs"], vgprs, found[k]["SGPRs Spill"], sspill))
    for k, (vgprs, sspill) in VEL3_AT_A0B1164.items():
        assert int(found[k]["VGPRs"]) <= vgprs and int(found[k]["SGPRs Spill"]) <= sspill, (k, found[k])
