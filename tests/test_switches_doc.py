"""The environment switches of the native library are read in ONE file, csrc/switches.hpp, and INTEGRATION.md's table
"Run-time switches" names exactly the switches that file reads."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "fmm-bem-relaxed_amd", "csrc")
NAME = re.compile(r"FMMBEM_[A-Z0-9_]*[A-Z0-9]")


def _read(*parts):
    with open(os.path.join(*parts), encoding="utf-8") as f:
        return f.read()


def _switches_read():
    """the names switches.hpp hands to getenv: its string literals"""
    return set(re.findall(r'"(FMMBEM_[A-Z0-9_]+)"', _read(CSRC, "switches.hpp")))


def _doc():
    """(names in the rows of the table, names in the "Removed" sentence)"""
    text = _read(ROOT, "INTEGRATION.md")
    section = text[text.index("## Run-time switches"):]
    nxt = section.find("\n## ", 1)
    section = section if nxt < 0 else section[:nxt]
    rows = [l for l in section.splitlines() if l.startswith("|") and not l.startswith("| Python side") and not l.startswith("|---") and
            not l.startswith("| variable")]
    assert len(rows) > 20
    removed = section[section.index("\nRemoved"):]
    # what the public header defines (status codes, enumerators) is no switch, whichever row mentions it
    api = set(re.findall(r"^\s*(?:#define\s+)?(FMMBEM_[A-Z0-9_]+)\b(?:\s*=|\s+\S|\s*,|\s*$)", _read(ROOT, "include", "fmmbem.h"), re.M))
    return set(NAME.findall("\n".join(rows))) - api, set(NAME.findall(removed))


def test_getenv_lives_in_switches_hpp_only():
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if name == "switches.hpp" or not os.path.isfile(path) or name.endswith((".o", ".isa")):   # (objects name the libc symbol)
            continue
        with open(path, "rb") as f:
            assert b"getenv" not in f.read(), name
    assert "getenv" in _read(CSRC, "switches.hpp")


def test_table_names_what_the_header_reads():
    read = _switches_read()
    assert len(read) > 30
    rows, removed = _doc()
    assert rows == read, (sorted(rows - read), sorted(read - rows))
    assert not (read & removed), sorted(read & removed)
