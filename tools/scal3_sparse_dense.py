"""The dense worst case of the brick lists (profiles/scal3_sparse.md): the bench scene with a density >= 0.2
everywhere and no buoyancy, stepped through tfl_simulate_step. After its first scan the policy stays on the two full launches and
pays one probe (scan + lists) per 16 steps. Prints ms per step of three repeats; alternate the libraries with TFL_LIBRARY.
usage: python tools/scal3_sparse_dense.py <res> [steps per repeat]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fluidnet_amd import FluidNetModel, tfluids  # noqa: E402
from fluidnet_amd.simulate import simulate_native  # noqa: E402

res = int(sys.argv[1])
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
dev = torch.device("cuda:0")
batch, mconf = bench.build_scene(res, res, None, dev)
mconf = dict(mconf, buoyancyScale=0)
z = torch.linspace(0, 6.28, res, device=dev)
batch["density"][...] = 0.2 + 0.1 * (1 + torch.sin(z).view(1, 1, res, 1, 1) * torch.cos(z).view(1, 1, 1, res, 1))
model = FluidNetModel.default_3d(seed=1)
for _ in range(20):
    simulate_native(None, mconf, batch, model)
out = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        simulate_native(None, mconf, batch, model)
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / steps * 1e3)
with tfluids.profile(batch["UDiv"]) as prof:
    for _ in range(32):
        simulate_native(None, mconf, batch, model)
k = {n: r["ms"] / 32 * 1e3 for n, r in prof.kernels.items() if n.startswith("k_scal")}
print("dense %d^3 %s: ms per step per repeat: %s | us per step: %s" % (
    res, os.path.basename(os.environ.get("TFL_LIBRARY", "libtfluids_hip.so")), " / ".join("%.4f" % v for v in out),
    ", ".join("%s %.2f" % kv for kv in sorted(k.items()))))
