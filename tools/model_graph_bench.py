"""Per-kernel device times (tfl_profile) of the projection net's forward pass on the shape-generic path for a 3-D 128^3
`default`-shaped model, plain and with the model-graph knobs (tfl_model_create_graph): 3 mres banks (concat), 3 dilated
banks (concat), batch norm. Prints one JSON line per configuration; profiles/model_graph.md keeps a record.
usage: python tools/model_graph_bench.py [--size 128] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "plain": {},
    "bn": dict(addBatchNorm=True),
    "mres3_concat": dict(banksNum=3, banksType="mres", banksSplitStage=2, banksJoinStage=4),
    "dilate3_concat": dict(banksNum=3, banksType="dilate", banksSplitStage=2, banksJoinStage=4),
    "dilate3_concat_bn": dict(banksNum=3, banksType="dilate", banksSplitStage=2, banksJoinStage=4, addBatchNorm=True),
}


def _ex_ms(model, tp, tU, tf, reps):
    """device ms per forward of the model's k_conv_direct_ex launches, and the whole profile"""
    import torch
    from fluidnet_amd import tfluids
    for _ in range(3):
        model.forward([tp, tU, tf])
    torch.cuda.synchronize()
    with tfluids.profile(tU) as prof:
        for _ in range(reps):
            model.forward([tp, tU, tf])
    torch.cuda.synchronize()
    k = {kn: dict(calls=v["calls"] / reps, ms=v["ms"] / reps, us_per_call=1e3 * v["ms"] / max(v["calls"], 1))
         for kn, v in sorted(prof.kernels.items())}
    return k.get("k_conv_direct_ex", {}).get("ms", 0.0), k


def _chain(k3, seed=1):
    """the 3-D default shapes with k3 launches of the 8 -> 8 k3 layer, on the graph kernels without BN (poolType 'max'
    with no pooling layer selects the graph path and changes nothing else)"""
    import numpy as np
    from fluidnet_amd import FluidNetModel
    rng = np.random.RandomState(seed)
    shapes = [(8, 3, 3)] + [(8, 8, 3)] * k3 + [(8, 8, 1), (1, 8, 1)]
    layers = [((rng.randn(co, ci, k, k, k) * 0.1).astype(np.float32), (rng.randn(co) * 0.01).astype(np.float32))
              for co, ci, k in shapes]
    return FluidNetModel(layers, True, graph=dict(poolType="max"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    os.environ["TFL_CONV_PATH"] = "direct"      # the plain model on the shape-generic kernels too (read at model creation)
    import torch
    import scenes
    from fluidnet_amd import FluidNetModel
    dev = torch.device("cuda:0")
    n = a.size
    sc = scenes.make_scene((n, n, n), seed=5, vel_cells=0.4, B=1)
    tp, tU, tf = (torch.from_numpy(sc[k]).to(dev) for k in ("p", "U", "flags"))
    for name, mc in CONFIGS.items():
        model = FluidNetModel.from_mconf(mc, True, seed=1)
        _, k = _ex_ms(model, tp, tU, tf, a.reps)
        out = dict(config=name, size=n, per_forward=k, total_ms=sum(v["ms"] for v in k.values()))
        if name.startswith("mres") or name.startswith("dilate"):
            # a float copy of the join's output (3 banks x 8 channels at full resolution), timed by events
            x = torch.empty(3 * 8 * n ** 3, device=dev)
            y = torch.empty_like(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            y.copy_(x)
            e0.record()
            for _ in range(a.reps):
                y.copy_(x)
            e1.record()
            torch.cuda.synchronize()
            out["copy_of_join_output_us"] = 1e3 * e0.elapsed_time(e1) / a.reps
        print(json.dumps(out))
    # isolated launches, as differences of k_conv_direct_ex totals between models whose launches differ in ONE thing:
    #   C_k = the default shapes with k launches of the 8 -> 8 k3 layer (no BN, no dilation)
    #   D_2 / D_3 = split before stage 2, join (add) before stage 3, 2 / 3 dilated banks: C_2's launches + a dilation-2
    #   (+ a dilation-4) 8 -> 8 k3 launch
    #   the 3-D default model with and without BN: the same launches with and without the BN epilogue
    c2, _ = _ex_ms(_chain(2), tp, tU, tf, a.reps)
    c3, _ = _ex_ms(_chain(3), tp, tU, tf, a.reps)
    dil = dict(banksType="dilate", banksAggregateMethod="add", banksSplitStage=2, banksJoinStage=3)
    d2, _ = _ex_ms(FluidNetModel.from_mconf(dict(dil, banksNum=2), True, seed=1), tp, tU, tf, a.reps)
    d3, _ = _ex_ms(FluidNetModel.from_mconf(dict(dil, banksNum=3), True, seed=1), tp, tU, tf, a.reps)
    base = FluidNetModel.from_mconf({}, True, seed=1)
    nobn, _ = _ex_ms(FluidNetModel(base.layers, True, graph=dict(poolType="max")), tp, tU, tf, a.reps)
    withbn, _ = _ex_ms(FluidNetModel.from_mconf(dict(addBatchNorm=True), True, seed=1), tp, tU, tf, a.reps)
    one = c3 - c2
    print(json.dumps(dict(isolated=True, size=n, conv_8to8_k3_dil1_ms=one, conv_8to8_k3_dil2_ms=d2 - c2,
                          conv_8to8_k3_dil4_ms=d3 - d2, dil2_ratio=(d2 - c2) / one, dil4_ratio=(d3 - d2) / one,
                          default_5_launches_no_bn_ms=nobn, default_5_launches_bn_ms=withbn, bn_ratio=withbn / nobn)))


if __name__ == "__main__":
    main()
