"""Helper of tests/test_scratch_history_cpu.py and tests/test_hip_scratch_history.py: the contract under every entry that takes
scratch memory ("Scratch memory"; profiles/scratch_history.md):

  1. history independence  the results are the same bits whatever the scratch held before the call;
  2. containment           no word outside [scratch, scratch + floats) is written when `floats` is exactly what the size function
                           returned;
  3. alignment as promised an entry that promises 8 bytes gives the same bits with its scratch at 8 mod 16, one that requires 16
                           refuses such a pointer and writes nothing.

check_row() holds one entry on one case to all three. It knows nothing of the library: an entry is a `Target` (below), the memory
comes from a `Backend` -- numpy for the stand-in entry and its mutants (tests/test_scratch_history_cpu.py: the proof that a
defective entry fails), torch on the device for the library's entries (tests/scratch_cases.py). Nothing here needs a GPU to import.

A scratch array is handed out as the interior of an ARENA: G floats of guard, the scratch, G floats of guard (and a few more, so
that the interior can also start 8 bytes off a 16-byte boundary). Every word outside the interior holds a sentinel that depends
on its position; after the call and a synchronise every one of them must still be there. G = 4096 floats keeps the interior on
16 bytes and is larger than the largest over-read the library documents (kWfGuard = 1280 pairs, csrc/tfl_pcg_ws.hpp)."""
import struct
import time

import numpy as np

G = 4096                      # guard floats on either side of a scratch array
SLACK = 4                     # floats behind the tail guard: room for the 8-mod-16 placement
NAN_BITS = 0x7FC00000         # the pre-state "nan": torch.full(..., nan), what scal3_sparse_run.run_stale fills with first
BIG = 1e30                    # ... and what it fills with second
SENTINEL = 0x7FA00000         # guard word at arena index i: SENTINEL | (i & 0xFFFFF) (a NaN whose payload is its position)
MISALIGN = 2                  # floats: an interior that begins 8 bytes behind a 16-byte boundary

# pre-states, in the order they run. "zero" is the clean run; it runs twice (the control).
FILLS = ("nan", "1e30")
LEFTOVERS = ("leftover-scene", "leftover-larger", "leftover-foreign")
PRESTATES = FILLS + LEFTOVERS


class Span:
    """n floats of `arena` from index `start` on: what an entry gets as its scratch pointer and size. An entry may of course
    compute any address from it -- the arena is there so that the test sees where it went."""

    def __init__(self, arena, start, n):
        self.arena, self.start, self.n = arena, int(start), int(n)

    def view(self):
        return self.arena[self.start:self.start + self.n]


class Target:
    """One entry on one case. Subclasses say what scratch the entry takes and run it.

      slots        names of the scratch arrays the entry takes (most take one)
      prestates    the pre-states that apply, a subset of PRESTATES
      align        slot -> 8 (the header promises that much: 8 mod 16 must give the same bits), 16 (the header requires it: 8 mod
                   16 must be refused) or None (the entry carves tensors out of the slot itself and promises nothing)
      short        slots for which the header documents that a scratch one float short is refused with nothing written
      excluded     {slot: [(offset, floats, why)]} regions the entry documents as state carried from call to call (none today)

      need(which)  {slot: floats} the size functions return for `which` = "case" | "scene" | "larger" | "foreign"
      run(which, spans)          runs the entry with spans = {slot: Span}, returns {name: array | float | int}. The inputs
                                 are built fresh for every call; "scene" / "larger" / "foreign" are the runs that leave leftovers.
      run_refused(spans, accepted=False)   calls the entry on the case with outputs pre-filled; returns a list of complaints: the
                                 call was not refused, or an output changed. (The helper checks the scratch and the guards
                                 itself.) A slot of `spans` that is short or misaligned is the one to be refused for: an entry
                                 that takes none of those is not called. accepted=True is the control: the spans are whole and
                                 aligned, the very same calls must succeed, and a complaint is a call that did not."""
    slots = ("ws",)
    prestates = PRESTATES
    align = {"ws": 8}
    short = ()
    excluded = {}

    def need(self, which):
        raise NotImplementedError

    def run(self, which, spans):
        raise NotImplementedError

    def run_refused(self, spans, accepted=False):
        raise NotImplementedError


# ---- memory ---------------------------------------------------------------------------------------------------------------
class NumpyBackend:
    name = "numpy"

    def alloc(self, n):
        return np.zeros(int(n), np.float32)

    def _words(self, a):
        return a.view(np.uint32)

    def _pattern(self, lo, hi):
        return (np.arange(lo, hi, dtype=np.int64) & 0xFFFFF).astype(np.uint32) | np.uint32(SENTINEL)

    def fill_sentinel(self, a, lo, hi):
        self._words(a)[lo:hi] = self._pattern(lo, hi)

    def fill_bits(self, a, lo, hi, bits):
        self._words(a)[lo:hi] = np.uint32(bits)

    def fill_value(self, a, lo, hi, v):
        a[lo:hi] = np.float32(v)

    def bad_sentinels(self, a, lo, hi):
        """arena indices in [lo, hi) that no longer hold their sentinel (the first few)"""
        bad = np.nonzero(self._words(a)[lo:hi] != self._pattern(lo, hi))[0]
        return [int(lo + i) for i in bad[:8]], int(bad.size)

    def snapshot(self, a, lo, hi):
        return self._words(a)[lo:hi].copy()

    def changed(self, a, lo, hi, snap):
        bad = np.nonzero(self._words(a)[lo:hi] != snap)[0]
        return [int(lo + i) for i in bad[:8]], int(bad.size)

    def sync(self):
        pass


class TorchBackend:
    """the same on a device; torch is imported when the first arena is made"""
    name = "torch"

    def __init__(self, device="cuda:0"):
        self.device = device

    def alloc(self, n):
        import torch
        a = torch.zeros(int(n), dtype=torch.float32, device=self.device)
        assert a.data_ptr() % 16 == 0
        return a

    def _words(self, a):
        import torch
        return a.view(torch.int32)

    def _pattern(self, lo, hi):
        import torch
        return (torch.arange(lo, hi, dtype=torch.int64, device=self.device) & 0xFFFFF).to(torch.int32) | SENTINEL

    def fill_sentinel(self, a, lo, hi):
        self._words(a)[lo:hi] = self._pattern(lo, hi)

    def fill_bits(self, a, lo, hi, bits):
        self._words(a)[lo:hi] = int(bits)

    def fill_value(self, a, lo, hi, v):
        a[lo:hi] = float(v)

    def bad_sentinels(self, a, lo, hi):
        import torch
        bad = torch.nonzero(self._words(a)[lo:hi] != self._pattern(lo, hi)).flatten()
        return [int(lo + i) for i in bad[:8].tolist()], int(bad.numel())

    def snapshot(self, a, lo, hi):
        return self._words(a)[lo:hi].clone()

    def changed(self, a, lo, hi, snap):
        import torch
        bad = torch.nonzero(self._words(a)[lo:hi] != snap).flatten()
        return [int(lo + i) for i in bad[:8].tolist()], int(bad.numel())

    def sync(self):
        import torch
        torch.cuda.synchronize()


# ---- the comparator -------------------------------------------------------------------------------------------------------
def _bits(v):
    """a canonical, bit-faithful form of one result: arrays as (dtype, shape, bytes), floats by their fp64 bits, ints as ints"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        v = np.ascontiguousarray(v)
        return ("array", str(v.dtype), tuple(v.shape), v.tobytes())
    if isinstance(v, (bool, int, np.integer)):
        return ("int", int(v))
    if isinstance(v, (float, np.floating)):
        return ("float", struct.pack("<d", float(v)))
    if isinstance(v, (tuple, list)):
        return ("seq", tuple(_bits(x) for x in v))
    if v is None:
        return ("none",)
    raise TypeError("same_bits: cannot compare a %s" % type(v).__name__)


def same_bits(got, clean):
    """[] when the two result dicts (named tensors, float returns, iteration counts, range_errors, traceErrors,
    pcgLastIterations, ...) hold the same bits, otherwise one line per name that differs. NaN equals NaN of the same bits; +0.0
    differs from -0.0."""
    out = []
    for k in sorted(set(got) | set(clean)):
        if k not in got or k not in clean:
            out.append("%s: only in the %s run" % (k, "clean" if k in clean else "other"))
            continue
        a, b = _bits(got[k]), _bits(clean[k])
        if a == b:
            continue
        if a[0] == "array" and b[0] == "array" and a[1:3] == b[1:3]:
            x, y = np.frombuffer(a[3], np.uint8), np.frombuffer(b[3], np.uint8)
            item = np.dtype(a[1]).itemsize
            n = int((x.reshape(-1, item) != y.reshape(-1, item)).any(axis=1).sum())
            out.append("%s: %d of %d elements differ" % (k, n, x.size // item))
        else:
            out.append("%s: %r != %r" % (k, got[k] if a[0] != "array" else a[1:3], clean[k] if b[0] != "array" else b[1:3]))
    return out


# ---- one row ----------------------------------------------------------------------------------------------------------------
class Arenas:
    """one arena per slot, each large enough for the largest run of the row"""

    def __init__(self, backend, target):
        self.be, self.target = backend, target
        self.needs = {w: dict(target.need(w)) for w in ("case",) + tuple(
            {"leftover-scene": "scene", "leftover-larger": "larger", "leftover-foreign": "foreign"}[p]
            for p in target.prestates if p in LEFTOVERS)}
        for w, nd in self.needs.items():
            assert set(nd) == set(target.slots), (w, nd)
            assert all(int(v) >= 1 for v in nd.values()), (w, nd)
        self.cap = {s: max(int(nd[s]) for nd in self.needs.values()) for s in target.slots}
        self.arena = {s: backend.alloc(G + self.cap[s] + G + SLACK) for s in target.slots}

    def lo(self, s, off):
        """where the interior of slot s begins in its arena: a slot that promises no alignment is never moved"""
        return G + (off if self.target.align.get(s) is not None else 0)

    def spans(self, which, off):
        return {s: Span(self.arena[s], self.lo(s, off), int(self.needs[which][s])) for s in self.target.slots}

    def sentinel_outside(self, off, n_of):
        """every word outside the interior of n_of[slot] floats gets its sentinel"""
        for s, a in self.arena.items():
            self.be.fill_sentinel(a, 0, self.lo(s, off))
            self.be.fill_sentinel(a, self.lo(s, off) + n_of[s], a.shape[0])

    def guard_failures(self, off, n_of, what):
        out = []
        for s, a in self.arena.items():
            for name, lo, hi in (("before", 0, self.lo(s, off)), ("behind", self.lo(s, off) + n_of[s], a.shape[0])):
                idx, n = self.be.bad_sentinels(a, lo, hi)
                if n:
                    out.append("%s: %d word(s) %s the scratch %r were written, first at float %+d of it"
                               % (what, n, name, s, idx[0] - self.lo(s, off)))
        return out


def check_row(target, backend, log=None, clean_out=None):
    """Holds `target` to the contract; returns the list of failures ([]: the row passes). log: a list that receives one
    (step, seconds) pair per run; clean_out: a dict that receives the clean run's results (for the caller's sanity checks)."""
    be = backend
    A = Arenas(be, target)
    fails = []
    need = A.needs["case"]
    excluded = target.excluded

    def timed(name, fn):
        t0 = time.perf_counter()
        try:
            return fn()
        finally:
            be.sync()
            if log is not None:
                log.append((name, time.perf_counter() - t0))

    def prepare(prestate, off):
        """the arenas as the case run finds them under `prestate`"""
        for s, a in A.arena.items():
            be.fill_sentinel(a, 0, a.shape[0])
            lo, hi = A.lo(s, off), A.lo(s, off) + need[s]
            if prestate in ("zero", "leftover-foreign"):
                be.fill_bits(a, lo, hi, 0)
            elif prestate == "nan":
                be.fill_bits(a, lo, hi, NAN_BITS)
            elif prestate == "1e30":
                be.fill_value(a, lo, hi, BIG)
        if prestate in LEFTOVERS:
            which = {"leftover-scene": "scene", "leftover-larger": "larger", "leftover-foreign": "foreign"}[prestate]
            for s, a in A.arena.items():        # the earlier run starts on zeros, like a fresh allocation
                be.fill_bits(a, A.lo(s, off), A.lo(s, off) + A.needs[which][s], 0)
            timed(prestate + ":before", lambda: target.run(which, A.spans(which, off)))
            be.sync()
            A.sentinel_outside(off, need)       # a larger earlier run legitimately wrote behind the case's scratch

    def attempt(prestate, off=0):
        prepare(prestate, off)
        out = timed(prestate, lambda: target.run("case", A.spans("case", off)))
        be.sync()
        fails.extend(A.guard_failures(off, need, prestate if not off else prestate + " at 8 mod 16"))
        return out

    clean = attempt("zero")
    if clean_out is not None:
        clean_out.update(clean)
    again = attempt("zero")
    control = same_bits(again, clean)
    if control:
        fails.append("control: the clean run differs from itself: " + "; ".join(control))
    for p in target.prestates:
        d = same_bits(attempt(p), clean)
        if d:
            fails.append("%s: differs from the clean run: %s" % (p, "; ".join(d)))

    def refused_run(what, off, short):
        """a call that must be refused: outputs (the target looks), scratch and guards (we look) unchanged. short: the slot
        that is one float short (None: none)"""
        for s, a in A.arena.items():
            be.fill_sentinel(a, 0, a.shape[0])
            be.fill_value(a, A.lo(s, off), A.lo(s, off) + need[s], 7.0)
        snaps = {s: be.snapshot(a, A.lo(s, off), A.lo(s, off) + need[s]) for s, a in A.arena.items()}
        spans = A.spans("case", off)
        if short is not None:
            spans[short] = Span(A.arena[short], A.lo(short, off), need[short] - 1)
        for c in timed(what, lambda: target.run_refused(spans)):
            fails.append("%s: %s" % (what, c))
        be.sync()
        fails.extend(A.guard_failures(off, need, what))
        for s, a in A.arena.items():
            idx, n = be.changed(a, A.lo(s, off), A.lo(s, off) + need[s], snaps[s])
            if n:
                fails.append("%s: the refused call wrote %d word(s) of the scratch %r, first at float %d" % (what, n, s, idx[0] - A.lo(s, off)))

    # alignment as promised (every slot moved at once; a target whose slots promise different things splits itself)
    kinds = {target.align.get(s) for s in target.slots} - {None}
    assert len(kinds) <= 1, "one alignment promise per target (slots that promise nothing aside: they stay where they are)"
    kind = kinds.pop() if kinds else None
    if kind == 8:
        for p in ("zero", "nan"):
            d = same_bits(attempt(p, MISALIGN), clean)
            if d:
                fails.append("%s at 8 mod 16: differs from the clean run: %s" % (p, "; ".join(d)))
    else:
        assert kind in (16, None), kind
    if kind == 16 or target.short:
        # the control of the refusals: the same path with every scratch whole and on 16 bytes must be ACCEPTED -- a call
        # refused for another reason (a wrong argument of the test's own) would otherwise pass as "refused, nothing written"
        for s, a in A.arena.items():
            be.fill_sentinel(a, 0, a.shape[0])
            be.fill_bits(a, A.lo(s, 0), A.lo(s, 0) + need[s], 0)
        for c in timed("accepted", lambda: target.run_refused(A.spans("case", 0), accepted=True)):
            fails.append("the control of the refusals: %s" % c)
        be.sync()
        fails.extend(A.guard_failures(0, need, "the control of the refusals"))
    if kind == 16:
        refused_run("8 mod 16", MISALIGN, None)
    for s in target.short:      # one slot at a time: a size check missing on one of two arrays must show
        refused_run("one float short" if len(target.slots) == 1 else "%s one float short" % s, 0, s)
    assert not excluded, "no entry documents a region that carries state; name it in the row before excluding it"
    return fails
