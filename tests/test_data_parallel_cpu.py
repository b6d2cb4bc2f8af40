"""CPU checks behind the data-parallel step (tfl_optim_step_reduced, fluidnet_amd.run_epoch.Closure(comm=...)): the new entry
points are declared alike in the header, the Python signatures and the Lua binding; and the premises of
tests/test_hip_data_parallel.py hold in the restatement of tests/data_parallel_ref.py -- in fp64 the mean of the ranks' gradients
IS the whole-batch gradient, PyTorch's own fp32 stays within the bar the GPU test uses on the same inputs, and each of the four
mistakes the GPU test makes in its hand sequence changes the result.
(The reduce buffer's layout is the optimiser's flat parameter index itself -- slot i = flat element i of tfl_refresh.hpp's
offset table, which tests/refresh_layout_host.cpp walks -- so there is no separate layout header and no program for one.)"""
import os
import re

import numpy as np
import pytest
import torch

import data_parallel_ref as D
import model_grad_ref as R
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tfl_optim_reduce_doubles", "tfl_optim_step_reduced", "tfl_optim_reduced_guard", "tfl_optim_sync_parameters")


def _args(s):
    return [a for a in s.split(",") if a.strip()]


def test_header_python_and_lua_declare_the_new_entries():
    from fluidnet_amd import _kernels, _lib
    text = open(os.path.join(ROOT, "include", "tfluids_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lua = open(os.path.join(ROOT, "fluidnet_amd", "lua", "tfluids_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]", lua.index("ffi.cdef[["))]
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/tfluids_hip.h"
        n = len(_args(m.group(1)))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
        assert re.search(r"\b%s\s*\(" % name, cdef), name + " is not in the Lua cdef"
    assert "function M.optimStepReduced(" in lua and "lib.tfl_optim_step_reduced(" in lua
    assert re.search(r"#define\s+TFL_ABI_VERSION\s+4\b", text)          # appended entries: the ABI number stays
    # appended: the new prototypes come after everything the parent commit declared
    assert hdr.index("tfl_optim_reduce_doubles") > hdr.index("tfl_rccl_comm_destroy")
    for k in ("k_optim_pack", "k_optim_unpack", "k_optim_unpack_norm"):
        assert _kernels.KERNEL_SOURCE[k] == "optim.hip+tfl_refresh.hpp"


def test_the_python_surface():
    import inspect
    from fluidnet_amd import dist, optim, run_epoch
    assert "comm" in inspect.signature(optim._Fused.step).parameters
    assert inspect.signature(optim._Fused.step).parameters["comm"].default is None
    assert callable(optim._Fused.reduced_guard) and callable(optim._Fused.sync_parameters)
    assert inspect.signature(run_epoch.Closure.__init__).parameters["comm"].default is None
    assert callable(run_epoch.Closure.sync_parameters) and callable(dist.run_virtual_closures)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
def test_fp64_mean_of_rank_gradients_is_the_whole_batch_gradient(is3D, world):
    model = R.make_model("default", is3D)
    parts = [D.rank_inputs(is3D, r) for r in range(world)]
    mean = D.mean_of([D.loss_grads(model, p) for p in parts])
    whole = D.loss_grads(model, D.whole_batch(parts))
    worst = D.worst_rel_l2(mean, whole)
    print("fp64: mean of %d rank gradients against the whole batch: worst per-tensor rel-L2 %.3e" % (world, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("is3D", [False, True], ids=["2d", "3d"])
def test_pytorch_fp32_holds_the_bar_on_the_yardstick_inputs(is3D):
    """the GPU test holds the reduced gradients of world 2 to R.BAR against the fp64 whole-batch gradient: PyTorch-CPU's fp32
    answer by the same route (per-rank gradients in fp32, the mean by the rule, one rounding) holds it too"""
    model = R.make_model("default", is3D)
    parts = [D.rank_inputs(is3D, r) for r in range(2)]
    whole = D.loss_grads(model, D.whole_batch(parts))
    per_rank = [[(w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64))
                 for w, b in D.loss_grads(model, p, dtype=torch.float32)] for p in parts]
    mean = [(w.astype(np.float32), b.astype(np.float32)) for w, b in D.mean_of(per_rank)]
    rels = R.rel_l2_per_tensor(mean, whole)
    print("PyTorch fp32, per tensor:", ["%.2e / %.2e" % p for p in rels])
    assert max(max(p) for p in rels) <= R.BAR


def test_the_four_mistakes_show_in_the_restatement():
    """2-D, world 2, rank 1's guard set in the guard case: the correct protocol gives the whole-batch gradient of both passes
    and holds every rank back under a guard; each mistake moves the reduced gradient or the parameters by far more than fp64
    rounding"""
    model = R.make_model("default", False)
    main = [D.rank_inputs(False, r) for r in range(2)]
    future = [D.rank_inputs(False, r, seed=131) for r in range(2)]
    g, after = D.restated_step(model, main, future, guards=[0, 0])
    whole = [(a[0] + b[0], a[1] + b[1]) for a, b in zip(D.loss_grads(model, D.whole_batch(main)),
                                                        D.loss_grads(model, D.whole_batch(future), (0.0, 0.0, D.LONG_TERM_DIV_LAMBDA)))]
    assert D.worst_rel_l2(g, whole) <= 1e-12
    assert any(not np.array_equal(w, w0) for (w, _), (w0, _) in zip(after, model.layers))
    for mistake in D.MISTAKES:
        guards = [0, 1] if mistake == "guard-left-local" else [0, 0]
        _, want = D.restated_step(model, main, future, guards)
        _, got = D.restated_step(model, main, future, guards, mistake=mistake, rank=0)
        diff = max(float(np.abs(a[j] - c[j]).max()) for a, c in zip(got, want) for j in (0, 1))
        print("%-34s max |parameter difference| %.3e" % (mistake, diff))
        assert diff > 1e-9, mistake      # (weights of order 0.1 in fp64: rounding is at 1e-17)
    # under a set guard the correct protocol leaves rank 0's parameters alone
    _, held = D.restated_step(model, main, future, guards=[0, 1])
    assert all(np.array_equal(w, np.asarray(w0, np.float64)) and np.array_equal(b, np.asarray(b0, np.float64))
               for (w, b), (w0, b0) in zip(held, model.layers))
