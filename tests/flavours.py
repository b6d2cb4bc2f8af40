"""The two flavours of the HIP library (fluidnet_amd/csrc/Makefile): the product library libtfluids_hip.so carries one kernel
per job; libtfluids_hip_exp.so (-DTFL_EXPERIMENTS, `make exp`) also carries the earlier and the measured-slower kernel forms
and reads the switches that select them. A test that forces such a form runs in a CHILD process against the second one
(TFL_LIBRARY, fluidnet_amd/_lib.py): the library is chosen when it is loaded, once per process."""
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "fluidnet_amd", "libtfluids_hip_exp.so")
SWITCH_TABLE = os.path.join(ROOT, "fluidnet_amd", "csrc", "tfl_switches.hpp")

# TFL_* variables the library does not read: the Python hosts and bench.py do
HOST_SIDE = frozenset(("TFL_LIBRARY", "TFL_WALL_PLAN", "TFL_DIST_BACKEND", "TFL_RANKS_SHARE_GPU", "TFL_SLAB_GRAPH"))


@functools.lru_cache(maxsize=None)
def switch_rows():
    """the rows of the library's switch table: {variable: (id, flavour, when, meaning)}"""
    rows = re.findall(r'^\s*X\((\w+),\s*"(TFL_[A-Z0-9_]+)",\s*(PRODUCT|EXP),\s*(ONCE|PER_CALL),\s*"([^"]*)"\)', open(SWITCH_TABLE).read(), flags=re.M)
    assert rows, SWITCH_TABLE
    return {name: (ident, flavour, when, meaning) for ident, name, flavour, when, meaning in rows}


def experiment_switches():
    """switches only the EXPERIMENTS flavour reads"""
    return frozenset(name for name, row in switch_rows().items() if row[1] == "EXP")


def is_experiments_process():
    return os.path.basename(os.environ.get("TFL_LIBRARY", "")) == os.path.basename(EXP_LIB)


def child_env(env, extra=None):
    """`env` + `extra`; when `extra` holds a switch of the EXPERIMENTS flavour the child loads that library. A TFL_* key that the
    library's table does not name would be ignored by either library: the test would compare a kernel with itself."""
    e = dict(env)
    e.update(extra or {})
    unknown = [k for k in (extra or {}) if k.startswith("TFL_") and k not in switch_rows() and k not in HOST_SIDE]
    assert not unknown, "no such switch in fluidnet_amd/csrc/tfl_switches.hpp: %s" % unknown
    if experiment_switches() & set(extra or {}):
        if not os.path.exists(EXP_LIB):
            import pytest
            pytest.skip("fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)")
        e["TFL_LIBRARY"] = EXP_LIB
    return e


def experiments_flavour(fn):
    """Decorator: the test body switches kernel forms inside one process (monkeypatch.setenv + a new model), so the whole test
    runs in a child pytest process that loads the EXPERIMENTS flavour; the parent only checks that the child passed."""
    @functools.wraps(fn)
    def wrapper(*a, **kw):
        if is_experiments_process():
            return fn(*a, **kw)
        import pytest
        if not os.path.exists(EXP_LIB):
            pytest.skip("fluidnet_amd/libtfluids_hip_exp.so is not built (make -C fluidnet_amd/csrc exp)")
        nodeid = os.environ["PYTEST_CURRENT_TEST"].rsplit(" ", 1)[0]
        env = dict(os.environ, TFL_LIBRARY=EXP_LIB)
        out = subprocess.run([sys.executable, "-m", "pytest", nodeid, "-q", "-s", "-x", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                             env=env, capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
        print(out.stdout)       # what the child printed (shown under -s)
    return wrapper
