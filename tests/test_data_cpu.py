"""CPU checks of fluidnet_amd.data's host code (scan, the epoch order, the data-parallel shards) against tests/data_ref.py and
torch/lib/data_binary.lua / run_epoch.lua:52-65, of the FluidNetModel.save_npz / from_npz round trip, and of the new entries'
declarations. Data sets are written into tmp_path with io.saveMantaFile."""
import os
import re
import warnings

import numpy as np
import pytest

import data_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tfl_optim_set_state", "tfl_frames_create", "tfl_frames_destroy", "tfl_frames_record_floats", "tfl_frames_put",
       "tfl_frames_gather")


def _numpy_divergence(U, flags):
    """tfluids' velocityDivergence on a 2-D grid (third_party/tfluids.cc: U(i) - U(i + 1) + U(j) - U(j + 1) on fluid cells off
    the border, 0 elsewhere): enough for DataRef on the CPU tests' 2-D sets"""
    div = np.zeros_like(flags)
    ux, uy = U[:, 0], U[:, 1]
    inner = (ux[:, :, 1:-1, 1:-1] - ux[:, :, 1:-1, 2:]) + (uy[:, :, 1:-1, 1:-1] - uy[:, :, 2:, 1:-1])
    div[:, 0, :, 1:-1, 1:-1] = np.where(flags[:, 0, :, 1:-1, 1:-1] == 1.0, inner, 0.0)
    return div


def test_header_python_and_lua_declare_the_new_entries():
    from fluidnet_amd import _kernels, _lib
    text = open(os.path.join(ROOT, "include", "tfluids_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lua = open(os.path.join(ROOT, "fluidnet_amd", "lua", "tfluids_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]", lua.index("ffi.cdef[["))]
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/tfluids_hip.h"
        n = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
        assert re.search(r"\b%s\s*\(" % name, cdef), name + " is not in the Lua cdef"
        assert hdr.index(name) > hdr.index("tfl_optim_sync_parameters")      # appended: the ABI number stays
    assert re.search(r"#define\s+TFL_ABI_VERSION\s+4\b", text)
    assert _kernels.KERNEL_SOURCE["k_frames_gather"] == "frames.hip+tfl_frames.hpp"
    make = open(os.path.join(ROOT, "fluidnet_amd", "csrc", "Makefile")).read()
    assert "frames.hip" in make
    src = open(os.path.join(ROOT, "fluidnet_amd", "csrc", "frames.hip")).read() + open(os.path.join(ROOT, "fluidnet_amd", "csrc", "tfl_frames.hpp")).read()
    assert "getenv" not in src and not re.search(r"\bSw::", src)      # no TFL_* switch


def test_scan_restates_the_reference(tmp_path):
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.data import scan
    conf = data_ref.write_dataset(str(tmp_path), False, (1, 8, 8), [(5, None, -1), (2, None, -1), (4, None, -1)])
    conf["ignoreFrames"] = 2
    with pytest.warns(UserWarning, match="Not enough files in sub-dir .*run_001"):
        sc = scan(conf, "tr")
    assert [r["dir"] for r in sc["runs"]] == ["run_000", "run_002"]                       # the short run is skipped
    assert [os.path.basename(f) for f in sc["runs"][0]["files"]] == ["000002.bin", "000003.bin", "000004.bin"]
    assert [os.path.basename(f) for f in sc["runs"][0]["divFiles"]] == ["000002_divergent.bin", "000003_divergent.bin", "000004_divergent.bin"]
    assert sc["samples"] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]                       # (run, frame) in run order
    ref = data_ref.DataRef(conf, "tr", _numpy_divergence)
    assert [r["dir"] for r in ref.runs] == [r["dir"] for r in sc["runs"]]
    assert ref.samples.tolist() == [list(s) for s in sc["samples"]]
    assert [d[2] for d in ref.decisions] == ["kept", "skipped", "kept"]
    # ignoreFrames = 0: every run, every frame
    conf["ignoreFrames"] = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert len(scan(conf, "tr")["samples"]) == 11
    # a frame without its divergent partner
    os.remove(os.path.join(str(tmp_path), "set", "tr", "run_002", "000001_divergent.bin"))
    with pytest.raises(TfluidsError, match="Main file count not equal to divergence file count"):
        scan(conf, "tr")
    with pytest.raises(TfluidsError, match="couldn't find any run directories"):
        scan(dict(conf, dataset="nothing"), "tr")


def test_the_reference_filter_keeps_a_negative_divergence_and_drops_a_positive_one(tmp_path):
    """the restatement on the layout the GPU tests use: +0.05 drops the run, -1 keeps it (the signed maximum, :127)"""
    conf = data_ref.write_dataset(str(tmp_path), False, (1, 16, 16), [(5, None, -1), (5, (0.05, (0, 7)), 2), (5, (-1.0, (0, 4)), 3)])
    ref = data_ref.DataRef(conf, "tr", _numpy_divergence)
    (_, d0, k0), (_, d1, k1), (_, d2, k2) = ref.decisions
    assert (k0, k1, k2) == ("kept", "dropped", "kept")
    assert abs(d0) < 1e-6 and abs(d1 - 0.05) < 1e-6 and abs(d2) < 1e-6
    assert ref.nsamples() == 10 and ref.samples[5].tolist() == [1, 0]
    b = ref.create_batch([9, 0])
    assert b["UTarget"].shape == (2, 2, 1, 16, 16) and float(_numpy_divergence(b["UTarget"], b["flags"]).min()) == pytest.approx(0.0, abs=1e-6)
    assert float(_numpy_divergence(ref.data[1]["U"], ref.data[1]["flags"]).min()) == pytest.approx(-1.0, abs=1e-6)


@pytest.mark.parametrize("nb,world", [(7, 2), (8, 2), (10, 3), (2, 3), (5, 1)])
def test_shards_are_disjoint_equal_and_cover_the_first_batches(nb, world):
    from fluidnet_amd.data import shard_batches
    parts = [shard_batches(nb, r, world) for r in range(world)]
    assert len({len(p) for p in parts}) == 1 and len(parts[0]) == nb // world
    flat = [i for p in parts for i in p]
    assert len(set(flat)) == len(flat) and sorted(flat) == list(range((nb // world) * world))
    for r, p in enumerate(parts):
        assert p == [r + k * world for k in range(nb // world)]


def test_shard_arguments_are_checked():
    from fluidnet_amd import TfluidsError
    from fluidnet_amd.data import shard_batches
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(TfluidsError):
            shard_batches(4, rank, world)


def test_epoch_order_is_a_permutation_and_a_function_of_the_rng_state():
    from fluidnet_amd.data import epoch_batches, epoch_order
    from fluidnet_amd.run_epoch import RandomStateRng
    n = 37
    a = epoch_order(n, RandomStateRng(5))
    assert sorted(a) == list(range(n)) and a != list(range(n))
    assert epoch_order(n, RandomStateRng(5)) == a and epoch_order(n, RandomStateRng(6)) != a
    # a function of the STATE: the same stream continued gives the next epoch's order, reproducible from a saved state
    rs = np.random.RandomState(11)
    rng = RandomStateRng(rs)
    epoch_order(n, rng)
    saved = rs.get_state()
    second = epoch_order(n, rng)
    rs2 = np.random.RandomState(0)
    rs2.set_state(saved)
    assert epoch_order(n, RandomStateRng(rs2)) == second
    # n - 1 draws and nothing else: the stream stands where n - 1 randint calls leave it
    ra, rb = np.random.RandomState(3), np.random.RandomState(3)
    epoch_order(n, RandomStateRng(ra))
    for i in range(n - 1, 0, -1):
        rb.randint(0, i + 1)
    assert ra.randint(1 << 30) == rb.randint(1 << 30)
    # evaluation: in order, and no draw
    rc = np.random.RandomState(3)
    assert epoch_order(n, RandomStateRng(rc), training=False) == list(range(n))
    assert rc.randint(1 << 30) == np.random.RandomState(3).randint(1 << 30)
    # maxSamplesPerEpoch truncates the drawn order (run_epoch.lua:62-65); batches: the last one short
    assert epoch_order(n, RandomStateRng(5), maxSamplesPerEpoch=10) == a[:10]
    assert epoch_order(n, RandomStateRng(5), maxSamplesPerEpoch=100) == a
    sets = epoch_batches(n, 8, RandomStateRng(5))
    assert [len(s) for s in sets] == [8, 8, 8, 8, 5] and [i for s in sets for i in s] == a
    r0, r1 = epoch_batches(n, 8, RandomStateRng(5), rank=0, world=2), epoch_batches(n, 8, RandomStateRng(5), rank=1, world=2)
    assert r0 == [sets[0], sets[2]] and r1 == [sets[1], sets[3]]


def test_frame_record_layout(tmp_path):
    """the record the loader puts: 2 C + 5 planes in the order of include/tfluids_hip.h, each padded to a multiple of 4 floats"""
    from fluidnet_amd import io
    from fluidnet_amd.data import FrameStore, frame_record
    conf = data_ref.write_dataset(str(tmp_path), True, (3, 5, 7), [(1, None, -1)])
    d = os.path.join(conf["dataDir"], conf["dataset"], "tr", "run_000")
    a, b = io.loadMantaFile(os.path.join(d, "000000.bin")), io.loadMantaFile(os.path.join(d, "000000_divergent.bin"))
    rec = frame_record((a, b))
    assert rec.shape == (11, 108) and rec.dtype == np.float32 and rec.size * 4 == FrameStore.record_bytes(True, 3, 5, 7)
    want = [b[0][0, 0], b[1][0, 0], b[1][0, 1], b[1][0, 2], a[2][0, 0], b[3][0, 0], a[0][0, 0], a[1][0, 0], a[1][0, 1], a[1][0, 2], a[3][0, 0]]
    for plane, w in zip(rec, want):
        assert np.array_equal(plane[:105].view(np.int32), w.reshape(-1).view(np.int32)) and not plane[105:].any()


def _same_model(a, b):
    assert a.is3D == b.is3D and a.pool == b.pool and a.up == b.up and a.opts == b.opts
    assert len(a.layers) == len(b.layers)
    for (w0, b0), (w1, b1) in zip(a.layers, b.layers):
        assert w0.shape == w1.shape and np.array_equal(w0.view(np.int32), w1.view(np.int32)) and np.array_equal(b0.view(np.int32), b1.view(np.int32))
    if a.graph is None:
        assert b.graph is None
        return
    ga, gb = dict(a.graph), dict(b.graph)
    bna, bnb = ga.pop("bn"), gb.pop("bn")
    assert ga == gb and (bna is None) == (bnb is None)
    for ma, mb in zip(bna or [], bnb or []):
        assert set(ma) == set(mb)
        for k in ma:
            if ma[k] is None or k == "eps":
                assert ma[k] == mb[k]
            else:
                assert mb[k].dtype == np.float32 and np.array_equal(np.asarray(ma[k], np.float32).view(np.int32), mb[k].view(np.int32))


def test_save_npz_round_trips_default_custom_and_banked_models(tmp_path):
    from fluidnet_amd import FluidNetModel
    models = {
        "default3d": FluidNetModel.default_3d(seed=3),
        "custom": FluidNetModel.from_mconf(dict(modelType="default", inputChannels=dict(pDiv=True, UDiv=True, div=True, flags=True),
                                                normalizeInputChan="pDiv", normalizeInputFunc="norm", nonlinType="relu6",
                                                addPressureSkip=True), False, seed=4),
        "banked": FluidNetModel.from_mconf(dict(modelType="default", banksNum=2, banksType="dilate", banksAggregateMethod="add"),
                                           True, seed=5),
        "tog-bn": FluidNetModel.from_mconf(dict(modelType="tog", addBatchNorm=True), False, seed=6),
    }
    assert models["banked"].graph["banksNum"] == 2 and models["tog-bn"].graph["bn"] and models["tog-bn"].pool[0] == 2
    for name, m in models.items():
        path = str(tmp_path / (name + ".npz"))
        m.save_npz(path, meta=dict(note=name, epoch=3), extra=dict(optim_m=np.arange(4, dtype=np.float32)))
        assert os.path.exists(path) and not os.path.exists(path + ".tmp")
        back = FluidNetModel.from_npz(path)
        _same_model(m, back)
        assert FluidNetModel.npz_meta(path) == dict(note=name, epoch=3)
        assert np.array_equal(np.load(path)["optim_m"], np.arange(4, dtype=np.float32))
    # a file written without the description (what from_npz read before) still loads, as a linear default-options model
    m = models["default3d"]
    old = str(tmp_path / "old.npz")
    np.savez(old, **{"w%d" % i: w for i, (w, _) in enumerate(m.layers)}, **{"b%d" % i: b for i, (_, b) in enumerate(m.layers)})
    back = FluidNetModel.from_npz(old)
    _same_model(m, back)
    assert FluidNetModel.npz_meta(old) is None
    from fluidnet_amd import TfluidsError
    with pytest.raises(TfluidsError, match="collides"):
        m.save_npz(str(tmp_path / "x.npz"), extra=dict(w0=np.zeros(1)))


def test_the_python_surface():
    import inspect
    from fluidnet_amd import data, optim, train_loop
    assert list(inspect.signature(data.DataBinary.__init__).parameters)[1:] == ["conf", "prefix", "device", "device_bytes"]
    assert inspect.signature(data.DataBinary.__init__).parameters["device_bytes"].default == 32 << 30
    assert list(inspect.signature(data.DataBinary.batches).parameters)[1:] == ["batchSize", "rng", "training", "maxSamplesPerEpoch", "rank", "world"]
    assert list(inspect.signature(train_loop.fit).parameters) == ["conf", "mconf", "tr", "te", "net", "comm", "resume"]
    assert list(inspect.signature(optim._Fused.load_state).parameters)[1:] == ["m", "v", "steps"]
    assert len(train_loop.LOG_NAMES) == 10
