"""The TRRE_* environment switches: the source and DESIGN.md §4.10 name the same set, and the library reads them in one place.

Plain file reading: no build, no GPU.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trre_amd", "csrc")
READERS = {"switches.hpp", "cli.cpp"}           # the library's one header; the command line, a binary of its own


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".hpp", ".hip", ".h")):
            with open(os.path.join(CSRC, name), encoding="utf-8") as f:
                yield name, f.read()


def _table_names():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    start = text.index("### 4.10 The switches, one table")
    section = text[start:text.index("\n## ", start)]
    rows = [line for line in section.splitlines() if line.startswith("| `TRRE_")]
    names = [re.match(r"\| `(TRRE_[A-Z0-9_]+)` \|", row).group(1) for row in rows]
    assert len(names) == len(set(names)), "a switch is listed twice"
    for row in rows:
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert len(cells) == 5 and all(cells), row
        assert cells[3] in ("once", "per call", "command line"), row
    return set(names)


def test_getenv_only_in_the_switches_header_and_the_cli():
    seen = {name for name, text in _sources() if "getenv" in text}
    assert seen == READERS, seen


def test_design_table_lists_exactly_the_switches_read():
    read = set()
    for name, text in _sources():
        if name in READERS:
            read |= set(re.findall(r'getenv\(\s*"(TRRE_[A-Z0-9_]+)"', text))
            # every call names its variable in place: nothing is read through a name the search above cannot see
            assert len(re.findall(r"getenv\(", text)) == len(re.findall(r'getenv\(\s*"TRRE_[A-Z0-9_]+"\s*\)', text)), name
    assert len(read) >= 30
    table = _table_names()
    assert read == table, (sorted(read - table), sorted(table - read))


def test_per_call_switches_are_the_accessor_functions():
    with open(os.path.join(CSRC, "switches.hpp"), encoding="utf-8") as f:
        text = f.read()
    per_call = set(re.findall(r'^inline [^\n]*_now\(\) \{[^\n]*getenv\("(TRRE_[A-Z0-9_]+)"\)', text, re.M))
    assert per_call == {"TRRE_LAZY_MAX_BYTES", "TRRE_LAZY_SEED_STATES", "TRRE_NFT_FOLD", "TRRE_GEN_MAX_REV"}
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        design = f.read()
    listed = set(re.findall(r"^\| `(TRRE_[A-Z0-9_]+)` \|[^\n]*\| per call \|", design, re.M))
    assert listed == per_call
