"""The training data set of torch/lib/data_binary.lua, resident where the training step runs.

    tr = DataBinary(conf, "tr", "cuda:0")                      # conf: dataDir, dataset, ignoreFrames (default_conf.lua)
    stats = run_epoch(closure, tr.batches(conf["batchSize"], rng))

The reference caches every frame on disk, rebuilds each mini-batch on CPU threads and copies it to the GPU (data_binary.lua:190-251,
413-453, data_parallel.lua, run_epoch.lua:131). Here every frame pair is loaded once (io.loadMantaFile), checked as the reference
checks it, and put into a frame store (tfl_frames_*: HBM slots first, `device_bytes` of them, the rest in pinned host memory the
GPU reads in place); a mini-batch is then ONE kernel launch that writes its seven tensors from the selected slots.

scan(), epoch_order() and shard_batches() are host code without a GPU. Indices are 0-based here (the reference's are 1-based).
Not built: the per-frame disk cache and its ZFP option, the thread-pool loader, calcDataStatistics /
visualizeBatch.
"""
import ctypes
import glob
import os
import warnings

import numpy as np
import torch

from . import io as _io
from . import tfluids
from ._lib import TfluidsError
from .run_epoch import RandomStateRng

DIV_THRESHOLD = 1e-2      # data_binary.lua:29
_OUTPUTS = ("pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget")      # tfl_frames_gather's order


def scan(conf, prefix):
    """data_binary.lua:31-67 without loading a frame: the run directories of <dataDir>/<dataset>/<prefix>/ in sorted order, in
    each the frames `*[0-9].bin` paired in sorted order with `*[0-9]_divergent.bin` (unequal counts: an error); a run with
    #files <= ignoreFrames is skipped with a warning, and the first ignoreFrames frames of the others are dropped.
    Returns {"base", "runs": [{"dir", "files", "divFiles"}], "samples": [(run, frame)] in run order} -- :157-176's list before
    the divergence filter, which needs the frames (DataBinary)."""
    base = os.path.join(conf["dataDir"], conf["dataset"], prefix)
    if not os.path.isdir(base):
        raise TfluidsError("couldn't find any run directories in " + base)
    dirs = sorted(d for d in os.listdir(base) if os.path.isdir(os.path.join(base, d)))
    if not dirs:
        raise TfluidsError("couldn't find any run directories in " + base)
    ignore = int(conf.get("ignoreFrames", 0))
    runs, samples = [], []
    for d in dirs:
        run_dir = os.path.join(base, d)
        files = sorted(glob.glob(os.path.join(run_dir, "*[0-9].bin")))
        div_files = sorted(glob.glob(os.path.join(run_dir, "*[0-9]_divergent.bin")))
        if len(files) != len(div_files):
            raise TfluidsError("Main file count not equal to divergence file count (%s: %d and %d)" % (run_dir, len(files), len(div_files)))
        if len(files) <= ignore:
            warnings.warn("Not enough files in sub-dir %s: skipping it" % run_dir)
            continue
        samples.extend((len(runs), f) for f in range(len(files) - ignore))
        runs.append(dict(dir=d, files=files[ignore:], divFiles=div_files[ignore:]))
    return dict(base=base, runs=runs, samples=samples)


def epoch_order(nsamples, rng=None, training=True, maxSamplesPerEpoch=None):
    """run_epoch.lua:52-65: the sample indices of one epoch. Training: a Fisher-Yates shuffle whose draws come from `rng`
    (randint(lo, hi), both ends included: run_epoch.RandomStateRng) and from nothing else, so the order is a function of the rng's
    state; evaluation: 0 .. nsamples - 1. maxSamplesPerEpoch truncates. (Torch7's own randperm stream is not reproduced: the
    reference's asynchronous loader delivers the batches out of order anyway.)"""
    order = list(range(int(nsamples)))
    if training:
        if rng is None:
            rng = RandomStateRng()
        for i in range(len(order) - 1, 0, -1):
            j = rng.randint(0, i)
            order[i], order[j] = order[j], order[i]
    if maxSamplesPerEpoch is not None and maxSamplesPerEpoch < len(order):
        order = order[:max(int(maxSamplesPerEpoch), 0)]
    return order


def shard_batches(nbatches, rank=0, world=1):
    """the batches of rank `rank` among `world` data-parallel ranks: r, r + world, ... of the common order, the remainder
    dropped, so that every rank has floor(nbatches / world) of them (run_epoch under a comm needs equally many)"""
    if world < 1 or not 0 <= rank < world:
        raise TfluidsError("shard_batches: rank %d of a world of %d" % (rank, world))
    return list(range(rank, (nbatches // world) * world, world))


def epoch_batches(nsamples, batchSize, rng=None, training=True, maxSamplesPerEpoch=None, rank=0, world=1):
    """the sample sets of one epoch for one rank: epoch_order cut into batches of batchSize (the last may be short), sharded"""
    if batchSize < 1:
        raise TfluidsError("batchSize must be positive")
    order = epoch_order(nsamples, rng, training, maxSamplesPerEpoch)
    sets = [order[i:i + batchSize] for i in range(0, len(order), batchSize)]
    return [sets[i] for i in shard_batches(len(sets), rank, world)]


def frame_record(pair):
    """the record of one frame pair for tfl_frames_put: pair = (loadMantaFile(frame), loadMantaFile(divergent frame)) ->
    float32 [2 C + 5][cells rounded up to a multiple of 4]: the planes pDiv, UDiv[C], flags, densityDiv, p, U[C], density
    (copies: the bits arrive as the files hold them), the padding zero"""
    (p, U, flags, density, _), (pDiv, UDiv, _, densityDiv, _) = pair
    cells = flags[0, 0].size
    planes = [pDiv[0, 0]] + list(UDiv[0]) + [flags[0, 0], densityDiv[0, 0], p[0, 0]] + list(U[0]) + [density[0, 0]]
    rec = np.zeros((len(planes), (cells + 3) & ~3), np.float32)
    for i, a in enumerate(planes):
        rec[i, :cells] = np.ascontiguousarray(a, np.float32).reshape(-1)
    return rec


class FrameStore:
    """tfl_frames_* (include/tfluids_hip.h): `capacity` slots of one record each on `device`, the first device_frames of them in
    HBM, the rest in pinned host memory that the gather kernel reads in place."""

    def __init__(self, device, is3D, zdim, ydim, xdim, capacity, device_frames):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TfluidsError("a frame store lives on an MI355X (got %s); there is no CPU path" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.is3D, self.dims = bool(is3D), (int(zdim), int(ydim), int(xdim))
        self.capacity, self.device_frames = int(capacity), int(device_frames)
        self._anchor = torch.empty(1, device=self.device)
        self._h = None
        self._pending = []      # records whose host-to-device copy the stream may not have passed yet
        lib, ctx = tfluids._context(self._anchor)
        self._h = lib.tfl_frames_create(ctx, int(self.is3D), *self.dims, self.capacity, self.device_frames)
        if not self._h:
            raise TfluidsError(lib.tfl_last_error(ctx).decode())
        self.record_floats = int(lib.tfl_frames_record_floats(self._h))

    @staticmethod
    def record_bytes(is3D, zdim, ydim, xdim):
        return 4 * (2 * (3 if is3D else 2) + 5) * ((zdim * ydim * xdim + 3) & ~3)

    def put(self, slot, record):
        """one record (frame_record's array) into a slot; ingest, not a hot path. The array is kept until flush()."""
        rec = np.ascontiguousarray(record, np.float32)
        if rec.size != self.record_floats:
            raise TfluidsError("frame store: a record of %d floats, the store's hold %d" % (rec.size, self.record_floats))
        lib, ctx = tfluids._context(self._anchor)
        tfluids._call(lib, ctx, lib.tfl_frames_put(ctx, self._h, int(slot), rec.ctypes.data_as(ctypes.c_void_p)))
        self._pending.append(rec)

    def flush(self):
        """waits for the puts enqueued so far and lets their host arrays go"""
        if self._pending:
            torch.cuda.current_stream(self.device).synchronize()
            self._pending = []

    def _tensor_args(self, who, tensors):
        args = []
        for name in _OUTPUTS:
            t = tensors.get(name)
            if t is None:
                args.append(None)
                continue
            if not (torch.is_tensor(t) and t.dim() == 5 and t.dtype == torch.float32 and t.is_contiguous()):
                raise TfluidsError("frames %s: %s must be a contiguous float32 [B, C, Z, Y, X] tensor" % (who, name))
            if t.device != self.device:
                raise TfluidsError("frames %s: %s is on %s, the store on %s (a CPU tensor? there is no CPU path)"
                                   % (who, name, t.device, self.device))
            args.append(tfluids._tt(t))
        return args

    def gather(self, slots, tensors):
        """tfl_frames_gather: item i of every tensor in `tensors` (a dict by output name -- pDiv, UDiv, flags, densityDiv,
        pTarget, UTarget, densityTarget; missing or None: skipped) = slot slots[i]. One launch per 128 items, on the current
        stream; nothing waits. A call captured into a graph replays the slots it was recorded with."""
        args = self._tensor_args("gather", tensors)
        slots = [int(s) for s in slots]
        lib, ctx = tfluids._context(self._anchor)
        idx = (ctypes.c_int32 * max(len(slots), 1))(*slots)
        tfluids._call(lib, ctx, lib.tfl_frames_gather(ctx, self._h, len(slots), idx, *args))

    def put_device(self, slots, tensors):
        """tfl_frames_put_device, the gather's mirror: item i of every tensor in `tensors` (a dict by the gather's names; missing
        or None: the planes it feeds keep what they hold) into slot slots[i], HBM and host-mapped slots alike. One launch per 128
        items on the current stream, no host round trip, nothing waits; a slot may appear only once per call. A record can be
        filled in two calls: pDiv / UDiv / flags / densityDiv first, pTarget / UTarget / densityTarget later."""
        args = self._tensor_args("put_device", tensors)
        slots = [int(s) for s in slots]
        lib, ctx = tfluids._context(self._anchor)
        idx = (ctypes.c_int32 * max(len(slots), 1))(*slots)
        tfluids._call(lib, ctx, lib.tfl_frames_put_device(ctx, self._h, len(slots), idx, *args))

    def close(self):
        if self._h:
            lib, ctx = tfluids._context(self._anchor)
            torch.cuda.synchronize(self.device)
            lib.tfl_frames_destroy(ctx, self._h)
            self._h = None
            self._pending = []

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass


def max_target_divergence(store, is3D, dims, first, n, chunk=16):
    """data_binary.lua:122-127 on store slots [first, first + n): the SIGNED maximum of velocityDivergence(U target, flags)
    (the loader's filter, and the generator's: fluidnet_amd.datagen)"""
    dims = tuple(dims)
    c = min(chunk, n)
    U = torch.empty((c, 3 if is3D else 2) + dims, device=store.device)
    flags = torch.empty((c, 1) + dims, device=store.device)
    div = torch.empty_like(flags)
    worst = None
    for i in range(0, n, c):
        m = min(c, n - i)
        store.gather(range(first + i, first + i + m), dict(UTarget=U, flags=flags))
        tfluids.velocityDivergenceForward(U[:m], flags[:m], div[:m])
        cur = div[:m].max()
        worst = cur if worst is None else torch.maximum(worst, cur)
    return float(worst.item())


class DataBinary:
    """torch.DataBinary over a resident frame store. Members as the reference's: runs ([{dir, ntimesteps, xdim, ydim, zdim,
    is3D}], the kept ones), samples (int64 [n, 2]: run, frame; 0-based), nsamples(), is3D, xdim / ydim / zdim. Sample i lives in
    slot i of the store (.store). device_bytes: how much HBM the store may take -- device_frames = as many slots as it holds --
    the frames beyond it live in pinned host memory."""

    def __init__(self, conf, prefix, device="cuda", device_bytes=32 << 30):
        self.dataDir, self.dataset, self.prefix = conf["dataDir"], conf["dataset"], prefix
        sc = scan(conf, prefix)
        self.store = None
        self.runs, samples = [], []
        self.is3D = None
        cursor, capacity = 0, max(len(sc["samples"]), 1)
        for irun, run in enumerate(sc["runs"]):
            for f, (fn, fn_div) in enumerate(zip(run["files"], run["divFiles"])):
                a, b = _io.loadMantaFile(fn), _io.loadMantaFile(fn_div)
                if a[2].shape != b[2].shape or not np.array_equal(a[2], b[2]):
                    raise TfluidsError("ERROR: Flags changed! (%s and %s)" % (fn, fn_div))                     # :77
                if a[4] != b[4]:
                    raise TfluidsError("3D flag is inconsistent! (%s and %s)" % (fn, fn_div))                  # :78
                is3D, nuchans = bool(a[4]), a[1].shape[1]
                if b[1].shape[1] != nuchans:
                    raise TfluidsError("velocity channel counts differ (%s and %s)" % (fn, fn_div))            # :86
                dims = tuple(int(v) for v in a[0].shape[2:])
                if self.is3D is None:
                    if not is3D and dims[0] != 1:
                        raise TfluidsError("2D domains should have unary z-dimension (%s)" % fn)               # :88
                    self.is3D, (self.zdim, self.ydim, self.xdim) = is3D, dims
                    frames = min(capacity, max(int(device_bytes), 0) // FrameStore.record_bytes(is3D, *dims))
                    self.store = FrameStore(device, is3D, *dims, capacity, frames)
                    self.device = self.store.device
                elif is3D != self.is3D:
                    raise TfluidsError("inconsistent 3D flags across run files (%s)" % fn)                     # :102
                elif dims != (self.zdim, self.ydim, self.xdim):
                    raise TfluidsError("frame dims %s differ from the set's %s (%s)" % (dims, (self.zdim, self.ydim, self.xdim), fn))      # :163-165
                self.store.put(cursor + f, frame_record((a, b)))
            n = len(run["files"])
            max_div = self._max_target_divergence(cursor, n)      # (reads the result back: the puts have been passed)
            self.store.flush()
            if max_div > DIV_THRESHOLD:                                                                        # :128-133
                warnings.warn("run %s (i = %d) has a sample with max(div) = %g which is above the allowable threshold (%g)"
                              " --> Removing run from the dataset..." % (run["dir"], irun, max_div, DIV_THRESHOLD))
                continue      # its slots are written again by the next run
            samples.extend((len(self.runs), f) for f in range(n))
            self.runs.append(dict(dir=run["dir"], ntimesteps=n, xdim=self.xdim, ydim=self.ydim, zdim=self.zdim, is3D=self.is3D))
            cursor += n
        if not self.runs:
            raise TfluidsError("no run of %s survived the loader's checks" % sc["base"])
        self.samples = np.asarray(samples, np.int64).reshape(-1, 2)
        self.capacity, self.device_frames = self.store.capacity, self.store.device_frames

    @classmethod
    def from_store(cls, store, runs, is3D, dims):
        """The same surface over a store that was filled on the device (datagen.generate: FrameStore.put_device), without a file
        read. runs: [(name, ntimesteps)] in slot order -- run r's frames lie in the slots behind those of runs 0 .. r - 1, sample i
        in slot i as after __init__. Nothing is checked or filtered here: the generator has applied the divergence threshold.
        The store stays the caller's: the data set reads it and does not copy it, it must outlive the data set's last batch, and
        close() closes THAT store (FrameStore.close may be called twice) -- a caller that goes on using the store does not call it."""
        dims = tuple(int(v) for v in dims)
        if bool(is3D) != store.is3D or dims != tuple(store.dims):
            raise TfluidsError("from_store: is3D / dims %s %s differ from the store's %s %s" % (bool(is3D), dims, store.is3D, store.dims))
        self = cls.__new__(cls)
        self.dataDir = self.dataset = self.prefix = None
        self.store, self.device = store, store.device
        self.is3D, (self.zdim, self.ydim, self.xdim) = bool(is3D), dims
        self.runs, samples = [], []
        for name, n in runs:
            samples.extend((len(self.runs), f) for f in range(int(n)))
            self.runs.append(dict(dir=str(name), ntimesteps=int(n), xdim=self.xdim, ydim=self.ydim, zdim=self.zdim, is3D=self.is3D))
        if not self.runs or not samples:
            raise TfluidsError("from_store: no runs")
        if len(samples) > store.capacity:
            raise TfluidsError("from_store: %d samples, the store holds %d slots" % (len(samples), store.capacity))
        self.samples = np.asarray(samples, np.int64).reshape(-1, 2)
        self.capacity, self.device_frames = store.capacity, store.device_frames
        return self

    def _max_target_divergence(self, first, n, chunk=16):
        return max_target_divergence(self.store, self.is3D, (self.zdim, self.ydim, self.xdim), first, n, chunk)

    def close(self):
        if self.store is not None:
            self.store.close()

    # -- the reference's surface -------------------------------------------------------------------------------------------
    def nsamples(self):
        return int(self.samples.shape[0])

    def AllocateBatchMemory(self, batchSize):
        """data_binary.lua:356-379 on the device: pDiv, pTarget, UDiv, UTarget, densityDiv, densityTarget zero-filled, flags from
        emptyDomain"""
        sh = (int(batchSize), 1, self.zdim, self.ydim, self.xdim)
        shU = (int(batchSize), 3 if self.is3D else 2) + sh[2:]
        b = dict(pDiv=torch.zeros(sh, device=self.device), UDiv=torch.zeros(shU, device=self.device),
                 flags=torch.empty(sh, device=self.device), densityDiv=torch.zeros(sh, device=self.device))
        b["pTarget"], b["UTarget"], b["densityTarget"] = b["pDiv"].clone(), b["UDiv"].clone(), b["densityDiv"].clone()
        tfluids.emptyDomain(b["flags"], self.is3D)
        return b

    def CreateBatch(self, batch, sampleSet):
        """data_binary.lua:413-453: sample sampleSet[i] into item i of the batch's seven tensors -- one tfl_frames_gather call --
        and the batch narrowed to len(sampleSet) items (views of the same buffers; the items behind them are not touched)"""
        ids = [int(s) for s in sampleSet]
        B = batch["UDiv"].size(0)
        if len(ids) > B:
            raise TfluidsError("CreateBatch: %d samples for a batch of %d" % (len(ids), B))
        if (batch["UDiv"].size(1) == 3) != self.is3D:
            raise TfluidsError("Mixing 3D model with 2D data or vice-versa!")
        for s in ids:
            if not 0 <= s < self.nsamples():
                raise TfluidsError("CreateBatch: sample %d is not in [0, %d)" % (s, self.nsamples()))
        self.store.gather(ids, batch)
        return {k: (v[:len(ids)] if k in _OUTPUTS else v) for k, v in batch.items()}

    def batches(self, batchSize, rng=None, training=True, maxSamplesPerEpoch=None, rank=0, world=1):
        """One epoch's mini-batches for run_epoch(closure, ...): a generator over ONE set of batch buffers, which the closure
        updates in place as the reference's batchGPU is -- a batch is valid until the next one is asked for. The order is
        epoch_batches' (drawn from `rng` now, before the first batch, and from it alone); with world > 1 this rank's share."""
        sets = epoch_batches(self.nsamples(), batchSize, rng, training, maxSamplesPerEpoch, rank, world)

        def gen():
            buf = self.AllocateBatchMemory(batchSize)
            for ids in sets:
                yield self.CreateBatch(buf, ids)
        return gen()
