"""The scratch-memory contract (tests/scratch_history.py) without a GPU:

  completeness  every function of include/tfluids_hip.h with a `workspace` or `tape` parameter is in the case table
                (tests/scratch_cases.py) or in its exclusion list with a reason, and every getTempStorage call site of
                fluidnet_amd/*.py is reached by a row;
  provenance    every row's case is found in the existing table it names -- "equal to the clean run" then means "equal to a
                result that is already held to the oracle or to an fp64 bound";
  mutants       the helper run on a small numpy stand-in entry with one defect at a time: it flags each mutant and passes the
                clean stand-in. This is the proof that the device test would fail on a real defect; no defect is ever put on
                the device."""
import ast
import os
import re

import numpy as np
import pytest

import scratch_cases as C
import scratch_history as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- completeness -------------------------------------------------------------------------------------------------------------
def header_entries():
    """names of the header's functions that take a `workspace` or a `tape` pointer"""
    text = open(os.path.join(ROOT, "include", "tfluids_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(tfl_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bfloat\s*\*\s*(workspace|tape)\b", m.group(2)):
            out.append(m.group(1))
    return sorted(set(out))


def test_the_header_parser_finds_the_entries_it_should():
    found = header_entries()
    for name in ("tfl_solveLinearSystemPCG", "tfl_solveLinearSystemPCGBatched", "tfl_normalizePressureMean", "tfl_fluidCriterion",
                 "tfl_velocityDivergenceNorm", "tfl_model_forward", "tfl_model_forward_train", "tfl_model_backward",
                 "tfl_model_backward_input", "tfl_simulate_step", "tfl_simulate_project", "tfl_simulate_step_items",
                 "tfl_simulate_project_items", "tfl_simulate_step_slab"):
        assert name in found, name
    assert "tfl_pcg_workspace_floats" not in found and "tfl_advectScalar" not in found


def test_every_entry_with_scratch_is_in_the_table_or_excluded_with_a_reason():
    covered = {e for r in C.ROWS for e in r.entries}
    header = set(header_entries())
    assert not covered - header - set(C.TMP_ONLY_ENTRIES), "rows name functions the header does not declare: %s" % sorted(covered - header)
    for name, why in C.EXCLUDED.items():
        assert name in header, "%s is excluded but the header has no such entry" % name
        assert name not in covered, "%s is both covered and excluded" % name
        assert len(why.split()) >= 4, "%s: the exclusion needs a reason" % name
    missing = header - covered - set(C.EXCLUDED)
    assert not missing, "entries that take scratch and have neither a row nor an exclusion: %s" % sorted(missing)


def temp_storage_call_sites():
    """(file, enclosing function) of every getTempStorage call in fluidnet_amd/*.py, the definition aside"""
    out = []
    pkg = os.path.join(ROOT, "fluidnet_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())
        for node in ast.walk(tree):
            if not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            for sub in ast.walk(node):
                if isinstance(sub, ast.Call):
                    f = sub.func
                    name = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)
                    if name == "getTempStorage" and node.name != "getTempStorage":
                        # the innermost function that holds the call
                        inner = [n for n in ast.walk(node) if isinstance(n, ast.FunctionDef) and n is not node and sub in list(ast.walk(n))]
                        if not inner:
                            out.append((fn, node.name))
    return sorted(set(out))


def test_every_temp_storage_call_site_is_reached_by_a_row():
    sites = temp_storage_call_sites()
    assert ("tfluids.py", "advectScalar") in sites and ("simulate.py", "simulate_native") in sites, sites
    reached = {s for r in C.ROWS for s in r.call_sites}
    unknown = reached - set(sites)
    assert not unknown, "rows name call sites that do not exist: %s" % sorted(unknown)
    missing = set(sites) - reached - set(C.EXCLUDED_CALL_SITES)
    assert not missing, "getTempStorage call sites no row reaches: %s" % sorted(missing)
    for site, why in C.EXCLUDED_CALL_SITES.items():
        assert site in sites and len(why.split()) >= 4, site


# ---- provenance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", C.ROWS, ids=[r.id for r in C.ROWS])
def test_the_case_of_every_row_is_in_the_table_it_names(row):
    assert row.sources, row.id
    for src in row.sources:
        assert C.in_source(src), "%s: %r is not in %s" % (row.id, src[1:], src[0])


def test_row_ids_are_unique_and_prestates_are_known():
    ids = [r.id for r in C.ROWS]
    assert len(ids) == len(set(ids))
    for r in C.ROWS:
        assert set(r.prestates) <= set(H.PRESTATES), r.id
        assert {"nan", "1e30", "leftover-scene", "leftover-larger"} <= set(r.prestates), r.id      # every row sees all of these
        assert ("leftover-foreign" in r.prestates) == r.shared_tmp, r.id                           # ... and shared scratch the foreign ones


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def test_same_bits_is_bit_equality():
    a = dict(p=np.array([0.0, 1.0, np.nan], np.float32), res=1e-5, iters=7)
    assert H.same_bits(dict(a), a) == []
    b = dict(a, p=np.array([-0.0, 1.0, np.nan], np.float32))
    assert H.same_bits(b, a) == ["p: 1 of 3 elements differ"]
    nan2 = np.array([0.0, 1.0, np.nan], np.float32)
    nan2.view(np.uint32)[2] ^= 1
    assert H.same_bits(dict(a, p=nan2), a) == ["p: 1 of 3 elements differ"]
    assert H.same_bits(dict(a, iters=8), a) and H.same_bits(dict(a, res=np.nextafter(1e-5, 1)), a)
    assert H.same_bits({k: v for k, v in a.items() if k != "res"}, a) == ["res: only in the clean run"]
    assert H.same_bits(dict(a, p=a["p"].astype(np.float64)), a)


# ---- the stand-in entry and its mutants ---------------------------------------------------------------------------------------------
# What it computes: the sum of every non-empty row of a [Y, X] array and the total. How: like the library's entries do --
#   [0]                 magic word of the row table      [1, 1 + Y)        row table: where each row begins in x (depends on X)
#   [1 + Y]             the accumulator                  then Y partials   one {value} per row, written for non-empty rows only
#   then Y tags         1 = "this row's partial is of this call"          then 4 + 3 floats: a 16-byte aligned vector of 4 with
#                                                                          the slack its run-time round-up needs (pcg_wf_pad)
MAGIC = np.float32(12345.0)
DEFECTS = ("read_unwritten", "accumulate_onto_assumed_zero", "stale_tag", "write_past_the_end", "write_before_the_start",
           "trusts_an_old_table", "round_up_without_slack")
VEC, VEC_SLACK = 4, 3


def standin_need(shape):
    Y, _ = shape
    return 1 + Y + 1 + Y + Y + VEC + VEC_SLACK


def standin(x, span, defect=None):
    a, s0 = span.arena, span.start
    Y, X = x.shape
    table, acc, part, tags, vec = 1, 1 + Y, 2 + Y, 2 + 2 * Y, 2 + 3 * Y
    assert span.n >= standin_need(x.shape)
    if defect == "write_past_the_end":
        a[s0 + span.n] = 1.0
    if defect == "write_before_the_start":
        a[s0 - 1] = 1.0
    # the row table is a function of the shape alone: the clean entry rebuilds it every call, the mutant keeps one it finds
    if not (defect == "trusts_an_old_table" and a[s0] == MAGIC):
        a[s0 + table:s0 + table + Y] = np.arange(Y, dtype=np.float32) * X
        a[s0] = MAGIC
    if defect != "accumulate_onto_assumed_zero":
        a[s0 + acc] = 0.0
    if defect != "stale_tag":
        a[s0 + tags:s0 + tags + Y] = 0.0
    flat = x.ravel()
    for j in range(Y):                                   # the producers: non-empty rows only
        at = int(a[s0 + table + j])
        row = flat[at:at + X]
        if row.any():
            a[s0 + part + j] = np.float32(row.astype(np.float64).sum())
            a[s0 + tags + j] = 1.0
    out = np.zeros(Y, np.float32)
    for j in range(Y):                                   # the consumer
        if a[s0 + tags + j] == 1.0 or defect == "read_unwritten":
            out[j] = a[s0 + part + j]
        a[s0 + acc] = np.float32(a[s0 + acc] + out[j])
    # a vector that needs 16 bytes inside a scratch that promises 8: rounded up at run time, paid for by VEC_SLACK floats
    pad = (4 - ((s0 + vec) & 3)) & 3
    at = s0 + vec + pad + (VEC_SLACK if defect == "round_up_without_slack" else 0)
    a[at:at + VEC] = flat[:VEC]
    return dict(rows=out, total=float(a[s0 + acc]), head=a[at:at + VEC].copy())


def _x(shape, seed, empty_rows):
    x = np.random.RandomState(seed).uniform(-1, 1, shape).astype(np.float32)
    x[list(empty_rows)] = 0.0
    return x


class StandIn(H.Target):
    """the case has empty rows; the other scene of the same shape has none (more "components"); the larger grid is wider and
    taller, so that every region lies elsewhere"""
    prestates = ("nan", "1e30", "leftover-scene", "leftover-larger")
    short = ("ws",)
    X = {"case": _x((6, 5), 1, (1, 4)), "scene": _x((6, 5), 2, ()), "larger": _x((9, 7), 3, (2,))}

    def __init__(self, defect=None):
        self.defect = defect

    def need(self, which):
        return {"ws": standin_need(self.X[which].shape)}

    def run(self, which, spans):
        return standin(self.X[which], spans["ws"], self.defect)

    def run_refused(self, spans, accepted=False):
        refused = spans["ws"].n < standin_need(self.X["case"].shape)      # ... before anything is written
        if accepted:
            return ["the call was not accepted"] if refused else []
        return [] if refused else ["the call was not refused"]


def test_the_helper_passes_the_clean_stand_in():
    log = []
    assert H.check_row(StandIn(), H.NumpyBackend(), log) == []
    steps = [s for s, _ in log]
    assert steps.count("zero") == 3 and "leftover-larger:before" in steps and "accepted" in steps and "one float short" in steps      # the control twice, once at 8 mod 16


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_helper_flags_every_mutant(defect):
    fails = H.check_row(StandIn(defect), H.NumpyBackend())
    assert fails, defect
    text = "\n".join(fails)
    assert not text.startswith("control"), text       # every mutant is deterministic: found by a pre-state, not by the control
    if defect == "write_past_the_end":
        assert "behind the scratch 'ws' were written, first at float +%d" % standin_need((6, 5)) in text
    if defect == "write_before_the_start":
        assert "before the scratch 'ws' were written, first at float -1" in text
    if defect == "trusts_an_old_table":               # a defect that only the larger grid's leftovers show
        assert all(f.startswith("leftover-larger:") for f in fails), fails
    if defect == "round_up_without_slack":            # a defect that only the 8-mod-16 placement shows
        assert all("at 8 mod 16" in f for f in fails), fails
        assert any("behind the scratch" in f for f in fails), fails
    if defect == "stale_tag":                         # neither fill satisfies the tag compare: only real leftovers do
        assert any(f.startswith("leftover-scene:") for f in fails) and not any(f.startswith(("nan", "1e30")) for f in fails), fails
    if defect in ("read_unwritten", "accumulate_onto_assumed_zero"):
        assert any(f.startswith("nan") for f in fails) and any(f.startswith("1e30") for f in fails), fails


def test_a_target_that_does_not_refuse_is_flagged():
    class Accepts(StandIn):
        def run_refused(self, spans, accepted=False):
            spans["ws"].arena[spans["ws"].start] = 0.0      # ... and writes
            return [] if accepted else ["the call was not refused"]
    fails = H.check_row(Accepts(), H.NumpyBackend())
    assert any("not refused" in f for f in fails) and any("the refused call wrote 1 word" in f for f in fails), fails


def test_a_16_byte_entry_must_refuse_8_mod_16():
    class Needs16(StandIn):
        align = {"ws": 16}

        def run_refused(self, spans, accepted=False):
            refused = bool(spans["ws"].start % 4 or spans["ws"].n < standin_need((6, 5)))
            if accepted:
                return ["the call was not accepted"] if refused else []
            return [] if refused else ["the call was not refused"]
    assert H.check_row(Needs16(), H.NumpyBackend()) == []

    class Takes8(Needs16):
        def run_refused(self, spans, accepted=False):
            refused = spans["ws"].n < standin_need((6, 5))
            if accepted:
                return ["the call was not accepted"] if refused else []
            return [] if refused else ["the call was not refused"]
    assert any(f.startswith("8 mod 16: the call was not refused") for f in H.check_row(Takes8(), H.NumpyBackend()))


def test_a_refusal_for_another_reason_is_flagged():
    """the control of the refusals: an entry the test calls wrongly refuses everything, the whole scratch included"""
    class RefusesAll(StandIn):
        def run_refused(self, spans, accepted=False):
            return ["the call was not accepted"] if accepted else []
    fails = H.check_row(RefusesAll(), H.NumpyBackend())
    assert fails == ["the control of the refusals: the call was not accepted"], fails


def test_a_short_scratch_is_tried_one_slot_at_a_time():
    """an entry with two arrays that checks the size of the first only"""
    class Two(H.Target):
        slots, prestates, short, align = ("a", "b"), ("nan", "1e30", "leftover-scene", "leftover-larger"), ("a", "b"), {"a": 8, "b": 8}
        checks = ("a", "b")
        seen = None

        def need(self, which):
            return {"a": 5, "b": 7}

        def run(self, which, spans):
            for s in self.slots:
                spans[s].view()[:] = 1.0
            return dict(x=1.0)

        def run_refused(self, spans, accepted=False):
            short = [s for s in self.slots if spans[s].n < self.need("case")[s]]
            self.seen.append(tuple(short))
            refused = any(s in self.checks for s in short)
            if accepted:
                return ["the call was not accepted"] if refused else []
            return [] if refused else ["the call was not refused"]
    t = Two()
    t.seen = []
    assert H.check_row(t, H.NumpyBackend()) == []
    assert t.seen == [(), ("a",), ("b",)], t.seen
    t = Two()
    t.seen, t.checks = [], ("a",)
    assert H.check_row(t, H.NumpyBackend()) == ["b one float short: the call was not refused"]
