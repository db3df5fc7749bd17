"""Every ``DQ4ML_*`` environment variable the engine reads has a row in the "Environment knobs"
table of docs/DESIGN.md, and the table names nothing the engine does not read: a knob cannot be
added, or outlive its code, without the table saying what it is."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the call forms of an env read: os.environ.get / os.environ[...], getenv, scanfuse.env(b"..."),
# and the utils/diag.py helpers (ablation, flag); include guards and #ifdef macros match none
_READ = re.compile(r"""(?:environ\.get\(|environ\[|getenv\(|\benv\(b|\bdiag\.\w+\()\s*["'](DQ4ML_[A-Z0-9_]+)["']""")
_ROW = re.compile(r"^\|\s*`(DQ4ML_[A-Z0-9_]+)`\s*\|")


def _read_names():
    names = set()
    for base, _, files in os.walk(os.path.join(ROOT, "net")):
        for fn in files:
            if fn.endswith((".py", ".hip", ".cpp", ".h")):
                with open(os.path.join(base, fn), encoding="utf-8") as f:
                    names.update(_READ.findall(f.read()))
    return names


def _table_names():
    with open(os.path.join(ROOT, "docs", "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    section = text.split("### Environment knobs", 1)[1].split("\n## ", 1)[0]
    rows = [m.group(1) for m in map(_ROW.match, section.splitlines()) if m]
    assert len(rows) == len(set(rows)), "a knob has two rows"
    return set(rows)


def test_diagnostic_builds_are_refused_without_the_gate(monkeypatch):
    import pytest

    from net.jgp.labs.sparkdq4ml_amd.utils import diag

    monkeypatch.delenv("DQ4ML_DIAG", raising=False)
    monkeypatch.delenv("DQ4ML_CUT_STAMPS", raising=False)
    monkeypatch.delenv("DQ4ML_CUT_ABLATE", raising=False)
    assert diag.flag("DQ4ML_CUT_STAMPS") is False and diag.ablation("DQ4ML_CUT_ABLATE") == 0
    monkeypatch.setenv("DQ4ML_CUT_STAMPS", "1")
    monkeypatch.setenv("DQ4ML_CUT_ABLATE", "2")
    for read in (lambda: diag.flag("DQ4ML_CUT_STAMPS"), lambda: diag.ablation("DQ4ML_CUT_ABLATE")):
        with pytest.raises(RuntimeError, match="DQ4ML_DIAG=1"):
            read()
    monkeypatch.setenv("DQ4ML_DIAG", "1")
    assert diag.flag("DQ4ML_CUT_STAMPS") is True and diag.ablation("DQ4ML_CUT_ABLATE") == 2


def test_design_table_lists_exactly_the_knobs_read():
    read, table = _read_names(), _table_names()
    assert "DQ4ML_DIAG" in read and "DQ4ML_SCAN_ABL" in read and "DQ4ML_FUSE_ROUTES" in read  # each call form matches
    assert read - table == set(), "read under net/ but missing from docs/DESIGN.md's table"
    assert table - read == set(), "in docs/DESIGN.md's table but read nowhere under net/"
