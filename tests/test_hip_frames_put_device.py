"""GPU checks of tfl_frames_put_device (k_frames_scatter, csrc/frames.hip): device tensors written into the slots of a frame
store read back BIT FOR BIT through the gather (compared as int32 views: NaN payloads, -0, denormals), in HBM slots, host-mapped
slots and a mix, and equal what put() of frame_record of the same data leaves; two half-puts equal one full put; slots and
planes a call does not name keep their bits; refusals name their reason and write nothing; a captured call replays; more than
128 items carry. (The zero padding of a written plane cannot be read back through the public entries --
the gather never touches it; tests/datagen_layout_host.cpp holds it on the scatter map.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(1, 5, 7), (4, 6, 8)]      # Z Y X mod 4 = 3 (every misalignment of a tensor's planes) and 0
CAPACITY, B = 6, 4
KEYS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")
DIV_HALF, TARGET_HALF = KEYS[:4], KEYS[4:]
SPECIAL = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000], np.uint32)


def _field(rng, shape):
    a = rng.randn(*shape).astype(np.float32)
    flat = a.reshape(-1)
    at = rng.choice(flat.size, size=min(len(SPECIAL), flat.size), replace=False)
    flat.view(np.uint32)[at] = SPECIAL[:len(at)]
    return a


def _inputs(dims, n=B, seed=0):
    """host arrays [n, C | 1, Z, Y, X] of the seven tensors, special bit patterns in each, and their device copies"""
    C = 3 if dims[0] > 1 else 2
    rng = np.random.RandomState(seed + dims[0] * 1000 + dims[1] * 10 + dims[2])
    host = {k: _field(rng, (n, C if k in ("UDiv", "UTarget") else 1) + tuple(dims)) for k in KEYS}
    return host, {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.int32)


def _gather(st, slots, dims):
    C = 3 if dims[0] > 1 else 2
    out = {k: torch.full((len(slots), C if k in ("UDiv", "UTarget") else 1) + tuple(dims), 7.0, device=DEV) for k in KEYS}
    st.gather(slots, out)
    return out


def _store(dims, device_frames, fill=None):
    from fluidnet_amd.data import FrameStore
    st = FrameStore(DEV, dims[0] > 1, *dims, CAPACITY, device_frames)
    if fill is not None:
        for s in range(CAPACITY):
            st.put(s, np.full(st.record_floats, fill, np.float32))
        st.flush()
    return st


def _record(host, i):
    """frame_record of item i: ((p, U, flags, density, is3D), (pDiv, UDiv, flags, densityDiv, is3D))"""
    from fluidnet_amd.data import frame_record
    one = {k: v[i:i + 1] for k, v in host.items()}
    return frame_record(((one["pTarget"], one["UTarget"], one["flags"], one["densityTarget"], None),
                         (one["pDiv"], one["UDiv"], one["flags"], one["densityDiv"], None)))


@pytest.mark.parametrize("device_frames", [0, 3, 6])
@pytest.mark.parametrize("dims", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_put_device_then_gather_is_bit_exact_and_equals_put_of_frame_record(dims, device_frames):
    host, dev = _inputs(dims)
    st, ref = _store(dims, device_frames, fill=5.0), _store(dims, device_frames, fill=5.0)
    try:
        slots = [5, 0, 3, 2]                                 # device_frames = 3: host, device, host, device
        st.put_device(slots, dev)
        for i, s in enumerate(slots):
            ref.put(s, _record(host, i))
        ref.flush()
        got, want = _gather(st, slots, dims), _gather(ref, slots, dims)
        for k in KEYS:
            assert np.array_equal(_bits(got[k]), _bits(host[k])), k
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        # the slots the call did not name keep their bits
        rest = _gather(st, [1, 4], dims)
        for k in KEYS:
            assert (rest[k] == 5.0).all(), k
        # fewer items than the tensors hold: items [n, B) are not read, their slots not written
        st.put_device([1], {k: v[2:] for k, v in dev.items()})
        one = _gather(st, [1, 4], dims)
        for k in KEYS:
            assert np.array_equal(_bits(one[k][0]), _bits(host[k][2])) and (one[k][1] == 5.0).all(), k
        # a misaligned source: a view that starts one float into a larger buffer
        n = dev["flags"].numel()
        big = torch.empty(n + 1, device=DEV)
        big[1:].copy_(dev["pTarget"].reshape(-1))
        st.put_device([4, 1, 0, 2], dict(flags=big[1:].view(dev["flags"].shape)))
        back = _gather(st, [4, 1, 0, 2], dims)
        assert np.array_equal(_bits(back["flags"]), _bits(host["pTarget"]))
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("dims", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_two_half_puts_equal_one_full_put_and_untouched_planes_keep_their_bits(dims):
    host, dev = _inputs(dims, seed=1)
    full, halves = _store(dims, 3, fill=5.0), _store(dims, 3, fill=5.0)
    try:
        slots = [4, 1, 2, 5]
        full.put_device(slots, dev)
        halves.put_device(slots, {k: dev[k] for k in DIV_HALF})
        mid = _gather(halves, slots, dims)
        for k in DIV_HALF:
            assert np.array_equal(_bits(mid[k]), _bits(host[k])), k
        for k in TARGET_HALF:
            assert (mid[k] == 5.0).all(), k                  # the planes of a missing tensor keep what they held
        halves.put_device(slots, {k: dev[k] for k in TARGET_HALF})
        a, b = _gather(full, range(CAPACITY), dims), _gather(halves, range(CAPACITY), dims)
        for k in KEYS:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    finally:
        full.close()
        halves.close()


def test_refusals_name_their_reason_and_write_nothing():
    from fluidnet_amd import TfluidsError
    dims = (1, 5, 7)
    host, dev = _inputs(dims, seed=3)
    st = _store(dims, 3, fill=5.0)
    try:
        def refused(match, slots, tensors):
            with pytest.raises(TfluidsError, match=match):
                st.put_device(slots, tensors)
            torch.cuda.synchronize()
            got = _gather(st, range(CAPACITY), dims)
            for k in KEYS:
                assert (got[k] == 5.0).all(), k

        refused("slot 2 appears twice", [2, 4, 2], dev)
        refused("slot 6 .*out of range", [0, 6, 1], dev)
        refused("slot -1 .*out of range", [-1], dev)
        refused("exceeds the batch size B = 4", [0, 1, 2, 3, 4], dev)
        refused("wrong shape", [0], dict(dev, pDiv=torch.full((B, 1, 1, 7, 5), 7.0, device=DEV)))
        refused("wrong shape", [0], dict(dev, UTarget=torch.full((B, 3) + dims, 7.0, device=DEV)))
        refused("CPU tensor", [0], dict(dev, flags=torch.full((B, 1) + dims, 7.0)))
        refused("contiguous", [0], dict(dev, flags=torch.full((B, 1, 1, 7, 5), 7.0, device=DEV).transpose(3, 4)))
    finally:
        st.close()


@pytest.mark.parametrize("dims", GRIDS, ids=["2d", "3d"])
def test_a_captured_put_device_replays(dims):
    host, dev = _inputs(dims, seed=4)
    st = _store(dims, 3, fill=5.0)
    try:
        slots = [4, 1, 5, 0]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st.put_device(slots, dev)      # (warm-up on the side stream, as torch's capture recipe asks)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st.put_device(slots, dev)
        # new contents in the same tensors: the replay writes them into the recorded slots
        host2, dev2 = _inputs(dims, seed=5)
        for k in KEYS:
            dev[k].copy_(dev2[k])
        g.replay()
        got = _gather(st, slots, dims)
        for k in KEYS:
            assert np.array_equal(_bits(got[k]), _bits(host2[k])), k
        rest = _gather(st, [2, 3], dims)
        for k in KEYS:
            assert (rest[k] == 5.0).all(), k
        torch.cuda.synchronize()
        del g
    finally:
        st.close()


def test_more_items_than_one_launch_carries():
    """n = 130 > 128 slot indices per launch: two launches, every item in its own slot"""
    from fluidnet_amd.data import FrameStore
    dims, n = (1, 5, 7), 130
    rng = np.random.RandomState(6)
    host = rng.randn(n, 2, *dims).astype(np.float32)
    U = torch.from_numpy(host).to(DEV)
    st = FrameStore(DEV, False, *dims, n + 2, 64)
    try:
        slots = [(37 * i) % (n + 2) for i in range(n)]      # a permutation of n distinct slots, HBM and host-mapped
        assert len(set(slots)) == n
        st.put_device(slots, dict(UTarget=U))
        back = torch.full((n, 2) + dims, 7.0, device=DEV)
        st.gather(slots, dict(UTarget=back))
        assert np.array_equal(_bits(back), host.view(np.int32))
    finally:
        st.close()
