"""Packed strings (include/trre_mi355x.h: trre_scan_device_strings) without a GPU.

The device path rests on one identity.  String i is the content of one line, so the STAGED text b"".join(r + b"\\n") holds
exactly the strings' lines, and its scan is the concatenation of R(r_i + b"\\n").  Every line prints one framing '\\n' and, for
the programs the path takes, no other: R(r_i + b"\\n") ends just past output newline R_i = number of '\\n' in the staged text
up to and with string i's closing one, and out_i is that piece without its last byte.  It is pinned here on the oracle over
every golden scan vector, cut at random points, behind line ends and into lines with their ends stripped, with empty strings,
strings holding '\\n' and NUL, and nrec = 0.  Then what needs no device: the symbol, the refusals."""
import ctypes
import random

import pytest

import golden_lib
import trre_amd
from oracle_lib import Oracle, OracleError
from trre_amd import api

IN, OUT, OFF = 0x10000000, 0x20000000, 0x30000000


def strings_rc(p, d_ooff=OFF + 8):
    """fake device pointers and overlapping offset arrays: every program taken is refused (TRRE_E_ARG) after the pattern checks
    and before anything touches a device"""
    m = ctypes.c_size_t(12345)
    rc = api.lib().trre_scan_device_strings(p._h, IN, 1000, OFF, 10, OUT, 2000, d_ooff, ctypes.byref(m), None)
    assert m.value == 0
    return rc


def prints_newline(p):
    rc = strings_rc(p)
    assert rc in (api.E_UNSUPPORTED, api.E_ARG), rc
    return rc == api.E_UNSUPPORTED


def cut(rng, data):
    """the vector as strings: cut anywhere and right behind some line ends (those strings hold '\\n'), some of them empty; or
    some of its lines with the line ends stripped"""
    if rng.random() < 0.3:
        lines = data.split(b"\n")
        return [lines[rng.randrange(len(lines))] for _ in range(rng.randrange(0, 7))]
    n = len(data)
    cuts = [rng.randrange(n + 1) for _ in range(rng.randrange(0, 10))]
    nls = [i + 1 for i, c in enumerate(data) if c == 10]
    if nls:
        cuts += rng.sample(nls, min(len(nls), rng.randrange(0, 4)))
    if cuts and rng.random() < 0.4:
        cuts += [rng.choice(cuts)] * 2
    off = [0] + sorted(cuts) + [n]
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_unframing_identity_on_golden_vectors():
    rng = random.Random(909)
    progs = {}
    n_cases = compared = diverged = newline_printing = n_empty = n_nl = n_nul = n_none = 0
    for pat, name, data, engine, exp in golden_lib.cases():
        n_cases += 1
        key = (pat, engine)
        if key not in progs:
            progs[key] = (prints_newline(trre_amd.Program(pat, engine)), Oracle(pat, engine))
        refused, o = progs[key]
        if refused:
            newline_printing += 1
            continue
        recs = cut(rng, data)
        fresh = engine == "dft"                # (its tables grow with what it has seen: a fresh one per input, as a fresh process)
        try:
            want = [(Oracle(pat, engine) if fresh else o).scan(r + b"\n")[:-1] for r in recs]
            framed = (Oracle(pat, engine) if fresh else o).scan(b"".join(r + b"\n" for r in recs))
        except OracleError:
            diverged += 1
            continue
        staged = b"".join(r + b"\n" for r in recs)
        nl = [i for i, c in enumerate(framed) if c == 10]
        got, start, at = [], 0, 0
        for r in recs:
            at += len(r) + 1
            rank = staged[:at].count(b"\n")
            end = nl[rank - 1] + 1                                   # just past output newline R_i
            assert framed[end - 1:end] == b"\n"
            got.append(framed[start:end - 1])
            start = end
        assert start == len(framed), (pat, name, engine)
        assert got == want, (pat, name, engine, recs)
        compared += 1
        n_none += not recs
        n_empty += b"" in recs
        n_nl += any(b"\n" in r for r in recs)
        n_nul += any(b"\0" in r for r in recs)
    assert compared + diverged + newline_printing == n_cases == 930, (compared, diverged, newline_printing, n_cases)
    assert compared > 700 and diverged > 0, (compared, diverged, newline_printing)
    assert n_none > 5 and n_empty > 50 and n_nl > 100 and n_nul > 5, (n_none, n_empty, n_nl, n_nul)


def test_specification_by_hand():
    o = Oracle("[a:A-z:Z]", "dft")
    want = {b"": b"", b"cat": b"CAT", b"a\nb": b"A\nB", b"a\0b": b"A", b"q\n": b"Q\n", b"\n\n": b"\n\n"}
    for r, w in want.items():
        assert o.scan(r + b"\n")[:-1] == w, r
    assert Oracle(":x", "nft").scan(b"\n")[:-1] == b"x"             # an empty string is an empty line, and this one prints


def test_library_exports_strings_symbol():
    assert hasattr(api.lib(), "trre_scan_device_strings")
    assert hasattr(trre_amd.Program, "scan_strings") and hasattr(trre_amd.Program, "map_strings")


def test_modes_other_than_scan_are_refused():
    for mode in ("match", "scan_all", "match_all"):
        assert strings_rc(trre_amd.Program("a:b", "nft", mode)) == api.E_UNSUPPORTED
        assert "scan mode only" in api.lib().trre_last_error().decode()


def test_newline_printing_programs_are_refused_and_copies_taken():
    assert prints_newline(trre_amd.Program("a:\n", "nft"))
    assert "newline" in api.lib().trre_last_error().decode()
    for pat, engine in (("[a:A-z:Z]", "dft"), (".", "nft"), ("a:xyz", "dft"), ("[aie]:", "nft"), (":x", "nft")):
        assert not prints_newline(trre_amd.Program(pat, engine)), pat


def test_overlaps_and_nulls_are_refused():
    p = trre_amd.Program("[a:A-z:Z]", "dft")
    m = ctypes.c_size_t()
    f = api.lib().trre_scan_device_strings
    assert strings_rc(p, OFF + 8) == api.E_ARG                                                      # the offset arrays overlap
    assert f(p._h, IN, 1000, IN + 500, 10, OUT, 2000, OFF, ctypes.byref(m), None) == api.E_ARG      # offsets inside the input
    assert f(p._h, IN, 1000, OFF, 10, IN + 10, 2000, OFF + 4096, ctypes.byref(m), None) == api.E_ARG  # partial data overlap
    assert f(p._h, None, 1000, OFF, 10, OUT, 2000, OFF + 4096, ctypes.byref(m), None) == api.E_ARG
    assert f(p._h, IN, 1000, None, 10, OUT, 2000, OFF + 4096, ctypes.byref(m), None) == api.E_ARG
    assert f(p._h, IN, 1000, OFF, 10, None, 2000, OFF + 4096, ctypes.byref(m), None) == api.E_ARG
