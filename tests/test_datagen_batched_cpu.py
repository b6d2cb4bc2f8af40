"""The host side of the generator's batched form (fluidnet_amd/datagen.py generate(batch_runs=R)), without a GPU:
the mix of forces and emitters in the plans the GPU tests batch (tests/datagen_batched_cases.py), the wave scheduler over a fake
runner -- the order of runs and report, a retried run in a later wave, the raise after MAX_ATTEMPTS, a partial last wave, R = 1 --
and the workspace table of the step on items in a stand-alone program under AddressSanitizer and UBSan
(tests/step_items_ws_host.cpp)."""
import os
import subprocess

import pytest

import datagen_batched_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plans_of_the_gpu_tests_mix_every_case():
    axes, buoy, vort, emit = C.mix(C.plans(False, (1, 32, 32)))
    assert set(axes[:6]) == {(-1.0, 0.0, 0.0)} and set(axes[6:]) == {(0.0, 1.0, 0.0)}      # two gravity axes: runs 0-5 against 6-7
    assert buoy == [0, 1, 2, 3, 7] and vort == [0, 1, 2, 6, 7]                                # each on and off, both off in 4 and 5
    assert sorted(set(range(8)) - set(buoy) - set(vort)) == [4, 5]
    assert emit == [2, 0, 0, 1, 1, 0, 0, 0]                                                   # 0 / 1 / 2 emitters
    axes, buoy, vort, emit = C.mix(C.plans(True, (12, 16, 20)))
    assert len(set(axes)) >= 4 and len({tuple(abs(v) for v in a) for a in axes}) == 3       # four directions and more, all three axes
    assert buoy == [1, 6] and sorted(set(range(8)) - set(vort)) == [3, 5, 7]
    assert [i for i, n in enumerate(emit) if n] == [0, 3, 4]
    # the items of the step tests keep a mix of their own: a force on and off, an item with neither (2-D), an emitter on some
    for is3D, dims in C.CASES:
        _, b, v, e = C.mix(C.plans(is3D, dims, C.STEP_PLANS))
        assert 0 < len(b) < 4 and 0 < len(v) < 4 and 0 < sum(1 for n in e if n) < 4, (dims, b, v, e)
    # with emitterSpeed some items carry a UBC pair and some do not
    moving = [any(any(c != 0.0 for c in em["vel"]) for em in p["emitters"]) for p in C.plans(False, (1, 32, 32), emitterSpeed=0.5)]
    assert any(moving) and not all(moving)


class _Runner:
    """max_div per (run, attempt) from a table; everything else is 0"""

    def __init__(self, table=None):
        self.table, self.waves, self.kept = dict(table or {}), [], []

    def __call__(self, wave):
        self.waves.append(list(wave))
        return [self.table.get(e, 0.0) for e in wave]

    def keep(self, j, run):
        self.kept.append((len(self.waves) - 1, j, run))


def _serial(first_run, nruns, table, threshold):
    """the serial generator's loop (fluidnet_amd/datagen.py generate) over the same table"""
    from fluidnet_amd import datagen
    runs, report = [], []
    for i in range(nruns):
        run = first_run + i
        for attempt in range(datagen.MAX_ATTEMPTS):
            d = table.get((run, attempt), 0.0)
            kept = threshold is None or d <= threshold
            report.append(dict(run=run, attempt=attempt, max_div=d, kept=kept))
            if kept:
                break
        else:
            raise AssertionError
        runs.append(run)
    return runs, report


def test_waves_give_the_serial_order_and_retry_in_a_later_wave():
    from fluidnet_amd import datagen
    table = {(3, 0): 9.0, (3, 1): 9.0, (5, 0): 7.0, (11, 0): 8.0}
    r = _Runner(table)
    kept, report, notes = datagen.schedule_waves(3, 10, 4, r, 1.0, r.keep)
    assert (kept, report) == _serial(3, 10, table, 1.0)
    # 10 runs in waves of 4, 4, 2 (the partial wave), then the retries: (3, 1), (5, 1), (11, 1) in one wave, then (3, 2)
    assert r.waves == [[(3, 0), (4, 0), (5, 0), (6, 0)], [(7, 0), (8, 0), (9, 0), (10, 0)], [(11, 0), (12, 0), (3, 1), (5, 1)],
                       [(11, 1), (3, 2)]]
    assert [len(w) for w in r.waves] == [4, 4, 4, 2]
    # every kept entry is handed to the sink behind its own wave, under its index in that wave
    assert sorted(r.kept) == sorted((w, j, run) for w, wave in enumerate(r.waves) for j, (run, a) in enumerate(wave) if table.get((run, a), 0.0) <= 1.0)
    assert notes == ["generated run %d (attempt %d) has max(div) = %g above the threshold %g: generating it again" % (run, a, table[(run, a)], 1.0)
                     for run, a in ((3, 0), (3, 1), (5, 0), (11, 0))]
    # no filter: nothing is retried, whatever the divergence
    r = _Runner(table)
    kept, report, notes = datagen.schedule_waves(3, 10, 4, r, None)
    assert kept == list(range(3, 13)) and all(e["kept"] for e in report) and notes == [] and len(r.waves) == 3


def test_waves_raise_the_serial_error_after_max_attempts():
    from fluidnet_amd import TfluidsError, datagen
    table = {(1, a): 5.0 for a in range(datagen.MAX_ATTEMPTS)}
    r = _Runner(table)
    with pytest.raises(TfluidsError, match="generate: run 1 exceeded the divergence threshold %d times" % datagen.MAX_ATTEMPTS):
        datagen.schedule_waves(0, 3, 2, r, 1.0)
    assert [e for w in r.waves for e in w if e[0] == 1] == [(1, a) for a in range(datagen.MAX_ATTEMPTS)]
    # one attempt fewer above the threshold: the run is kept at its last attempt
    del table[(1, datagen.MAX_ATTEMPTS - 1)]
    kept, report, _ = datagen.schedule_waves(0, 3, 2, _Runner(table), 1.0)
    assert (kept, report) == _serial(0, 3, table, 1.0) and report[-2] == dict(run=1, attempt=datagen.MAX_ATTEMPTS - 1, max_div=0.0, kept=True)


@pytest.mark.parametrize("nruns,R", [(5, 4), (8, 8), (3, 32), (4, 1)])
def test_waves_partial_and_single(nruns, R):
    from fluidnet_amd import datagen
    table = {(2, 0): 3.0}
    r = _Runner(table)
    kept, report, _ = datagen.schedule_waves(0, nruns, R, r, 1.0)
    assert (kept, report) == _serial(0, nruns, table, 1.0)
    assert all(1 <= len(w) <= R for w in r.waves) and sum(len(w) for w in r.waves) == nruns + 1
    assert [len(w) for w in r.waves[:-1]] == [R] * (len(r.waves) - 1) or R > nruns
    if R == 1:      # one run at a time: every wave is one entry, the retry comes behind the last run
        assert r.waves == [[(i, 0)] for i in range(nruns)] + [[(2, 1)]]


def test_generate_refuses_a_batch_it_cannot_hold():
    from fluidnet_amd import TfluidsError, datagen
    g = datagen.default_gconf(False, (1, 16, 16))
    for R in (0, 33):
        with pytest.raises(TfluidsError, match="batch_runs = %d, 1 to 32" % R):
            datagen.generate(g, "tr", 1, 1, out_dir="unused", batch_runs=R)


def test_step_items_ws_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_items_ws_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "step_items_ws_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "step items workspace OK" in out.stdout, out.stdout + out.stderr
