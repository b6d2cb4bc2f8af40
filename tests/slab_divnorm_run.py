"""Helper of tests/test_hip_divnorm.py: own process (the library binds ONE RCCL per process, here tests/stub_rccl.cpp named by
TFL_RCCL_LIBRARY). `native`: SlabSimulation.divergence_norm through the library's native transport on 2, 3 and 4 slabs equals
tfluids.velocityDivergenceNorm of the un-cut run bit for bit, and the next step still equals the un-cut step."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def native():
    import torch
    import test_hip_divnorm as T
    from fluidnet_amd import tfluids
    lib, ctx = tfluids._context(torch.zeros(1, device="cuda:0"))
    assert lib.tfl_rccl_comm_origin(ctx).decode() == os.environ["TFL_RCCL_LIBRARY"]
    for world in (2, 3, 4):
        T.slab_norms_equal_uncut(world, transport="native")
    print("slab divnorm native ok")


if __name__ == "__main__":
    {"native": native}[sys.argv[1]]()
