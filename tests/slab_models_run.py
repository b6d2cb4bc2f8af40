"""Helper of tests/test_hip_slab_models.py: own process (the conv path is chosen when a model is created, and the library binds
ONE RCCL per process, here tests/stub_rccl.cpp named by TFL_RCCL_LIBRARY).
`direct`: the default topology under TFL_CONV_PATH=direct on uneven slabs equals the un-cut step (exact at world 1).
`native`: tog and yang slabs through the library's native transport equal the un-cut step.
`graph`:  a tog rank-step recorded into a HIP graph (tfl_slab_graph_create, stub in STUB_RCCL_NULL mode) replays to the bits of
          the eager step -- middle and end rank of a 4-rank layout -- and, on a slab without neighbours, to the un-cut step's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def direct():
    import test_hip_slab_models as T
    assert os.environ.get("TFL_CONV_PATH") == "direct"
    for world in (1, 3):
        Zt = 9 * world + 4
        ref = T.scene(Zt, Y=20, X=24)
        c = T.conf()
        make = (lambda: T.net("default"))
        T.compare(ref, c, T.sims(ref, c, T.cuts_for(Zt, world, 1), make, overlap=world > 1), make, 0.0 if world == 1 else 1e-7)
    print("slab models direct ok")


def native():
    import torch
    import test_hip_slab_methods as M
    import test_hip_slab_models as T
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import RcclComm, SlabSimulation
    for name, Zt, F in (("tog", 72, 4), ("yang", 31, 1)):
        ref = T.scene(Zt, Y=20, X=24)
        lib, ctx = tfluids._context(ref["flags"])
        assert lib.tfl_rccl_comm_origin(ctx).decode() == os.environ["TFL_RCCL_LIBRARY"]
        c = T.conf()
        cuts = T.cuts_for(Zt, 3, F)
        uid = RcclComm.unique_id(ctx)
        sims = []
        for r in range(3):
            model = T.net(name)
            lay = T.layout(cuts, r, model)
            loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
            sims.append(SlabSimulation(loc, c, model, lay, (lambda cx, r=r: RcclComm(cx, uid, r, 3)), own_context=True))
        M.run_and_compare(ref, c, sims, model=T.net(name), tol=1e-7)
    print("slab models native ok")


def graph():
    import torch
    import test_hip_slab_models as T
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import RcclComm, SlabLayout, SlabSimulation
    from fluidnet_amd.simulate import simulate_native
    world, Zt = 4, 64
    ref = T.scene(Zt, Y=20, X=24)
    c = T.conf()
    for _ in range(2):
        simulate_native(None, c, ref, T.net("tog"))         # a developed state to cut the slabs from
    lib, ctx = tfluids._context(ref["flags"])
    for rank in (1, 0):
        out = {}
        for g in (False, True):
            model = T.net("tog")
            lay = SlabLayout(Zt, world, rank, model=model)
            assert lay.halo == 16
            loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
            comm = RcclComm(ctx, RcclComm.unique_id(ctx), rank, world)
            sim = SlabSimulation(loc, c, model, lay, comm, graph=g)
            for n in range(5):
                sim.step(eager=g and n == 3)
            sim.drain()
            torch.cuda.synchronize()
            assert (sim.graph is not None) == g, sim.graph_error
            out[g] = {k: loc[k].clone() for k in T.STATE}
            sim.close()
        for k in out[False]:
            assert torch.equal(out[False][k], out[True][k]), (rank, k)
    model = T.net("tog")
    lay = SlabLayout(Zt, 1, 0, model=model)
    loc = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref.items()}
    sim = SlabSimulation(loc, c, model, lay, None, graph=True)
    ref_model = T.net("tog")
    for _ in range(4):
        sim.step()
        simulate_native(None, c, ref, ref_model)
    torch.cuda.synchronize()
    assert sim.graph is not None, sim.graph_error
    for k in T.STATE:
        assert torch.equal(loc[k], ref[k]), k
    sim.close()
    print("slab models graph ok")


if __name__ == "__main__":
    {"direct": direct, "native": native, "graph": graph}[sys.argv[1]]()
