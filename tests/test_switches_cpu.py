"""The library's environment switches (fluidnet_amd/csrc/tfl_switches.hpp: one table, one reader). The reader runs in a
stand-alone program under AddressSanitizer and UBSan, tests/switches_host.cpp, compiled here for the host in both flavours and
run as its own process; the rest holds the table, its copy in INTEGRATION.md and tests/flavours.py together."""
import os
import re
import subprocess

import pytest

import flavours

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidnet_amd", "csrc")


@pytest.mark.parametrize("define", [[], ["-DTFL_EXPERIMENTS"]], ids=["product", "experiments"])
def test_switches_host_program_under_sanitizers(tmp_path, define):
    exe = str(tmp_path / "switches_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + define +
                          [os.path.join(ROOT, "tests", "switches_host.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TFL_")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "switches OK" in out.stdout, out.stdout + out.stderr
    assert ("EXPERIMENTS" if define else "product") in out.stdout, out.stdout


def table_lines():
    text = open(flavours.SWITCH_TABLE).read()
    return [l for l in text[text.index("#define TFL_SWITCH_TABLE(X)"):text.index("// clang-format on")].splitlines() if l.strip().startswith("X(")]


def test_one_file_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["tfl_switches.hpp"], readers
    assert "#include <hip" not in open(flavours.SWITCH_TABLE).read()


def test_every_row_parses_and_names_are_unique():
    lines = table_lines()
    names = re.findall(r'"(TFL_[A-Z0-9_]+)"', "\n".join(re.sub(r',\s*"[^"]*"\)\s*\\?$', "", l) for l in lines))       # (meanings cut off)
    ids = [re.match(r"\s*X\((\w+),", l).group(1) for l in lines]
    assert len(lines) == len(names) == len(flavours.switch_rows()) > 40, (len(lines), len(names), len(flavours.switch_rows()))
    assert len(set(names)) == len(names) and len(set(ids)) == len(ids)
    for name, (ident, flavour, when, meaning) in flavours.switch_rows().items():
        assert name == "TFL_" + ident and meaning.strip() and "|" not in meaning, name
    # the text-valued rows are read per call: no pointer getenv returned is kept
    for name in ("TFL_CONV_PATH", "TFL_ADVECT_MODE", "TFL_RCCL_LIBRARY"):
        assert flavours.switch_rows()[name][2] == "PER_CALL", name
    assert flavours.switch_rows()["TFL_NO_VEC4"][1:3] == ("EXP", "ONCE")


def integration_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 4e."):text.index("## 5.")]
    return re.findall(r"^\| `(TFL_[A-Z0-9_]+)` \| (\w+) \| (\w+) \| (.*) \|$", sec, flags=re.M), sec


def test_integration_md_shows_the_same_table():
    doc, sec = integration_table()
    rows = flavours.switch_rows()
    assert [d[0] for d in doc] == list(rows), "INTEGRATION.md 4e lists other rows than tfl_switches.hpp (or in another order)"
    for name, flavour, when, meaning in doc:
        assert (flavour, when, meaning) == rows[name][1:], name
    table = "\n".join(l for l in sec.splitlines() if l.startswith("|"))
    assert set(re.findall(r"TFL_[A-Z0-9_]+", table)) <= set(rows), sorted(set(re.findall(r"TFL_[A-Z0-9_]+", table)) - set(rows))
    for name in flavours.HOST_SIDE:         # named in their own paragraph, as not read by the library
        assert name not in rows and name not in table and "`%s" % name in sec, name


def test_flavours_takes_the_experiment_switches_from_the_table(monkeypatch):
    exp = {re.search(r'"(TFL_[A-Z0-9_]+)"', l).group(1) for l in table_lines() if re.search(r'",\s*EXP,', l)}
    assert flavours.experiment_switches() == exp and 0 < len(exp) < len(flavours.switch_rows())
    monkeypatch.setattr(flavours.os.path, "exists", lambda p: True)
    base = {"PATH": "/bin"}
    for name in sorted(flavours.switch_rows()):
        e = flavours.child_env(base, {name: "1", "OTHER": "x"})
        assert e[name] == "1" and e["OTHER"] == "x" and e["PATH"] == "/bin"
        assert (e.get("TFL_LIBRARY") == flavours.EXP_LIB) == (name in exp), name
    assert "TFL_LIBRARY" not in flavours.child_env(base) and "TFL_LIBRARY" not in flavours.child_env(base, {})
    assert "TFL_LIBRARY" not in flavours.child_env(base, {"TFL_WALL_PLAN": "0", "TFL_VEL3_KZ": "2"})
    assert base == {"PATH": "/bin"}
    # a switch that is no row would be ignored by either library: refused, not run against the product library
    for name in ("TFL_M16_", "TFL_VEL3_KZ_C", "TFL_NO_SUCH_SWITCH"):
        with pytest.raises(AssertionError):
            flavours.child_env(base, {name: "1"})
