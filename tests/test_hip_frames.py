"""GPU checks of the resident frame store and its one-launch gather (tfl_frames_*, csrc/frames.hip): every gathered plane equals
io.loadMantaFile's arrays BIT FOR BIT (compared as int32 views: NaN payloads, -0, denormals, flag words up to 255), from device
slots, host-mapped slots and a mix, at every alignment case of Z Y X mod 4; what a call does not own is not touched; refusals
name their reason and write nothing; a captured gather replays the same bits.
Frames are written into tmp_path with io.saveMantaFile and read back with io.loadMantaFile: the files are the reference."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Z Y X mod 4 = 3, 2, 0 in 2-D; 1 and 0 in 3-D
GRIDS = [(1, 5, 7), (1, 6, 9), (1, 6, 10), (3, 5, 7), (4, 6, 8)]
CAPACITY, B, N = 6, 4, 3
KEYS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")
SPECIAL = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000], np.uint32)


def _field(rng, shape):
    a = rng.randn(*shape).astype(np.float32)
    flat = a.reshape(-1)
    at = rng.choice(flat.size, size=min(len(SPECIAL), flat.size), replace=False)
    flat.view(np.uint32)[at] = SPECIAL[:len(at)]
    return a


def _write_frames(tmp_path, dims):
    """CAPACITY frame pairs; -> per frame the dict of the seven arrays as loadMantaFile returns them"""
    from fluidnet_amd import io
    Z, Y, X = dims
    is3D = Z > 1
    C = 3 if is3D else 2
    rng = np.random.RandomState(Z * 1000 + Y * 10 + X)
    frames = []
    for f in range(CAPACITY):
        flags = rng.randint(0, 256, (1, 1, Z, Y, X)).astype(np.float32)
        fn, fd = str(tmp_path / ("%06d.bin" % f)), str(tmp_path / ("%06d_divergent.bin" % f))
        io.saveMantaFile(fn, _field(rng, (1, 1, Z, Y, X)), _field(rng, (1, C, Z, Y, X)), flags, _field(rng, (1, 1, Z, Y, X)))
        io.saveMantaFile(fd, _field(rng, (1, 1, Z, Y, X)), _field(rng, (1, C, Z, Y, X)), flags, _field(rng, (1, 1, Z, Y, X)))
        a, b = io.loadMantaFile(fn), io.loadMantaFile(fd)
        assert a[4] == is3D and np.array_equal(a[2], b[2]) and float(a[2].max()) > 200
        frames.append((dict(pDiv=b[0][0], UDiv=b[1][0], flags=a[2][0], densityDiv=b[3][0], pTarget=a[0][0], UTarget=a[1][0],
                            densityTarget=a[3][0]), (a, b)))
    return frames


def _store(frames, dims, device_frames):
    from fluidnet_amd.data import FrameStore, frame_record
    st = FrameStore(DEV, dims[0] > 1, *dims, CAPACITY, device_frames)
    for slot, (_, pair) in enumerate(frames):
        st.put(slot, frame_record(pair))
    st.flush()
    return st


def _buffers(dims, fill=7.0):
    C = 3 if dims[0] > 1 else 2
    return {k: torch.full((B, C if k in ("UDiv", "UTarget") else 1) + tuple(dims), fill, device=DEV) for k in KEYS}


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _check(out, frames, slots, skipped=()):
    for k in KEYS:
        got = _bits(out[k])
        if k in skipped:
            assert (out[k] == 7.0).all(), k
            continue
        for i, s in enumerate(slots):
            assert np.array_equal(got[i], frames[s][0][k].view(np.int32)), (k, i, s)
        assert (out[k][len(slots):] == 7.0).all(), k      # items [n, B) are not touched


@pytest.mark.parametrize("device_frames", [0, 3, 6])
@pytest.mark.parametrize("dims", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_gather_is_bit_exact_from_device_and_host_slots(tmp_path, dims, device_frames):
    frames = _write_frames(tmp_path, dims)
    st = _store(frames, dims, device_frames)
    try:
        for slots in ([5, 0, 3], [2, 4, 1]):               # device_frames = 3: host, device, host / device, host, device
            out = _buffers(dims)
            st.gather(slots, out)
            _check(out, frames, slots)
        out = _buffers(dims)
        st.gather([4, 1, 4], out)                           # a slot twice in one call
        _check(out, frames, [4, 1, 4])
        out = _buffers(dims)
        skipped = ("UDiv", "densityDiv", "pTarget")
        st.gather([0, 5, 2], {k: (None if k in skipped else v) for k, v in out.items()})      # three outputs NULL
        _check(out, frames, [0, 5, 2], skipped)
        # a misaligned destination: a view that starts one item + one float into a larger buffer is still 4-byte aligned
        big = torch.full((B * dims[0] * dims[1] * dims[2] + 1,), 7.0, device=DEV)
        view = big[1:].view(B, 1, *dims)
        st.gather([3, 3, 0], dict(flags=view))
        got = _bits(view)
        for i, s in enumerate([3, 3, 0]):
            assert np.array_equal(got[i], frames[s][0]["flags"].view(np.int32))
        assert float(big[0]) == 7.0 and (view[N:] == 7.0).all()
        # n = 0 and an overwritten slot
        st.gather([], _buffers(dims))
        from fluidnet_amd.data import frame_record
        st.put(1, frame_record(frames[5][1]))
        st.flush()
        out = _buffers(dims)
        st.gather([1], out)
        _check(out, [frames[5]] * 6, [1])
    finally:
        st.close()


def test_refusals_name_their_reason_and_write_nothing(tmp_path):
    from fluidnet_amd import TfluidsError, _lib, tfluids
    dims = (1, 5, 7)
    frames = _write_frames(tmp_path, dims)
    st = _store(frames, dims, 3)
    try:
        out = _buffers(dims)

        def refused(match, slots, tensors):
            with pytest.raises(TfluidsError, match=match):
                st.gather(slots, tensors)
            torch.cuda.synchronize()
            for k in KEYS:
                assert (out[k] == 7.0).all(), k

        refused("slot 6 .*out of range", [0, 6, 1], out)
        refused("slot -1 .*out of range", [-1], out)
        refused("exceeds the batch size B = 4", [0, 1, 2, 3, 4], out)
        refused("exceeds the batch size B = 2 of UDiv", [0, 1, 2], dict(out, UDiv=torch.full((2, 2) + dims, 7.0, device=DEV)))
        refused("wrong shape", [0], dict(out, pDiv=torch.full((B, 1, 1, 7, 5), 7.0, device=DEV)))
        refused("wrong shape", [0], dict(out, UTarget=torch.full((B, 3) + dims, 7.0, device=DEV)))
        refused("CPU tensor", [0], dict(out, flags=torch.full((B, 1) + dims, 7.0)))
        refused("contiguous", [0], dict(out, flags=torch.full((B, 1, 1, 7, 5), 7.0, device=DEV).transpose(3, 4)))
        # the library's own check of where an output lives: a descriptor of HOST memory handed straight to the C entry
        host = torch.full((B, 1) + dims, 7.0)
        lib, ctx = tfluids._context(out["pDiv"])
        desc = _lib.tfl_tensor(host.data_ptr(), B, 1, *dims)
        rc = lib.tfl_frames_gather(ctx, st._h, 1, (ctypes.c_int32 * 1)(0), tfluids._tt(out["pDiv"]), None, ctypes.byref(desc), None, None, None, None)
        assert rc != 0 and "flags is not device memory" in lib.tfl_last_error(ctx).decode()
        torch.cuda.synchronize()
        assert (host == 7.0).all() and (out["pDiv"] == 7.0).all()
        # creation and put
        with pytest.raises(TfluidsError, match="device_frames 7 is not in"):
            from fluidnet_amd.data import FrameStore
            FrameStore(DEV, False, 1, 5, 7, 6, 7)
        with pytest.raises(TfluidsError, match="slot 6 is out of range"):
            st.put(6, np.zeros(st.record_floats, np.float32))
        with pytest.raises(TfluidsError, match="record of 5 floats"):
            st.put(0, np.zeros(5, np.float32))
        assert st.record_floats == 9 * 36
    finally:
        st.close()


@pytest.mark.parametrize("dims", [(1, 5, 7), (4, 6, 8)], ids=["2d", "3d"])
def test_a_captured_gather_replays_the_same_bits(tmp_path, dims):
    frames = _write_frames(tmp_path, dims)
    st = _store(frames, dims, 3)
    try:
        out = _buffers(dims)
        slots = [4, 1, 5]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st.gather(slots, out)          # (warm-up on the side stream, as torch's capture recipe asks)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st.gather(slots, out)
        for k in KEYS:
            out[k].fill_(7.0)
        g.replay()
        _check(out, frames, slots)
        # the recorded slots, not the current ones: an eager gather of other slots in between does not change the replay
        st.gather([0, 0, 0], out)
        g.replay()
        _check(out, frames, slots)
        torch.cuda.synchronize()
        del g
    finally:
        st.close()


def test_more_items_than_one_launch_carries(tmp_path):
    """n = 130 > 128 slot indices per launch: two launches, every item right"""
    dims = (1, 5, 7)
    frames = _write_frames(tmp_path, dims)
    st = _store(frames, dims, 3)
    try:
        n = 130
        slots = [(7 * i) % CAPACITY for i in range(n)]
        U = torch.full((n + 1, 2) + dims, 7.0, device=DEV)
        st.gather(slots, dict(UTarget=U))
        got = _bits(U)
        for i, s in enumerate(slots):
            assert np.array_equal(got[i], frames[s][0]["UTarget"].view(np.int32)), i
        assert (U[n:] == 7.0).all()
    finally:
        st.close()
