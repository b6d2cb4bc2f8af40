"""Helper of tests/test_hip_slab_methods.py: own process (the library binds ONE RCCL per process, here tests/stub_rccl.cpp named
by TFL_RCCL_LIBRARY). `native <world> <method>`: `world` virtual z-slab ranks step the Jacobi projection with that advection
method through the library's native transport and must equal the un-cut step bit for bit. `graph 0 <method>`: the rank-step
recorded into a HIP graph (tfl_slab_graph_create, stub in STUB_RCCL_NULL mode) replays to the bits of the eager step -- middle
and end rank of a 4-rank layout -- and, on a slab without neighbours, to the un-cut step's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def native(world, method):
    import torch
    import test_hip_simulate as T
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate_native
    dev = torch.device("cuda:0")
    ref = T._to_dev(M.scene(10 * world + 2), dev)
    lib, ctx = tfluids._context(ref["flags"])
    assert lib.tfl_rccl_comm_origin(ctx).decode() == os.environ["TFL_RCCL_LIBRARY"]
    mconf = M.mconf(method)
    sims = J.slab_sims(ref, mconf, J.uneven_cuts(ref["flags"].size(2), world), transport="native")
    for _ in range(3):
        for _ in range(2):
            simulate_native(None, mconf, ref, None)
        run_virtual_ranks(sims, 2)
        M.assert_owned(sims, ref)
    for s in sims:
        s.close()
    print("methods native transport ok: world %d, %s" % (world, method))


def graph(method):
    import torch
    import test_hip_simulate as T
    import test_hip_slab_methods as M
    from fluidnet_amd import tfluids
    from fluidnet_amd.dist import RcclComm, SlabLayout, SlabSimulation
    from fluidnet_amd.simulate import simulate_native
    dev = torch.device("cuda:0")
    world, Zt = 4, 48
    ref = T._to_dev(M.scene(Zt), dev)
    mconf = M.mconf(method)
    for _ in range(2):
        simulate_native(None, mconf, ref, None)          # a developed state to cut the slabs from
    lib, ctx = tfluids._context(ref["flags"])
    for rank in (1, 0):
        out = {}
        for g in (False, True):
            lay = SlabLayout(Zt, world, rank)
            loc = {k: (lay.extract(v) if torch.is_tensor(v) else v) for k, v in ref.items()}
            comm = RcclComm(ctx, RcclComm.unique_id(ctx), rank, world)
            sim = SlabSimulation(loc, mconf, None, lay, comm, graph=g)
            for n in range(5):
                sim.step(eager=g and n == 3)
            sim.drain()
            torch.cuda.synchronize()
            assert (sim.graph is not None) == g, sim.graph_error
            out[g] = {k: loc[k].clone() for k in ("pDiv", "UDiv", "density")}
            sim.close()
        for k in out[False]:
            assert torch.equal(out[False][k], out[True][k]), (rank, k)
    lay = SlabLayout(Zt, 1, 0)
    loc = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref.items()}
    sim = SlabSimulation(loc, mconf, None, lay, None, graph=True)
    for _ in range(4):
        sim.step()
        simulate_native(None, mconf, ref, None)
    torch.cuda.synchronize()
    assert sim.graph is not None, sim.graph_error
    for k in ("pDiv", "UDiv", "density"):
        assert torch.equal(loc[k], ref[k]), k
    sim.close()
    print("methods slab graph ok: %s" % method)


if __name__ == "__main__":
    if sys.argv[1] == "native":
        native(int(sys.argv[2]), sys.argv[3])
    else:
        graph(sys.argv[3])
