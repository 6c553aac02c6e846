"""Replaced strings (include/trre_mi355x.h: trre_sub_device_strings; Program.sub_strings / sub_list) without a GPU: the
yardstick of tests/sub_lib.py against the examples written out by hand, against re.sub, and against the plain reference scan
(selecting every match must give what the reference prints for the line); and what the new compile mode is made of, through
the C ABI."""
import re

import pytest

import sub_lib
import trre_amd
from oracle_lib import Oracle
from trre_amd import api


def one(program, acceptor, rec, first, count):
    return sub_lib.Yardstick(program, acceptor, [rec]).per_string(first, count)[0]


def test_library_exports_sub_symbol():
    assert hasattr(api.lib(), "trre_sub_device_strings") and api.MODE_SUB == 16
    for name in ("sub_strings", "sub_list"):
        assert hasattr(trre_amd.Program, name)


def test_the_examples_by_hand():
    cd = ("(cat:dog|dog:cat)", "(cat|dog)")
    for sel, want in (((0, 1), b"dog dog cat"), ((1, 1), b"cat cat cat"), ((1, -1), b"cat cat dog"), ((0, -1), b"dog cat dog")):
        assert one(*cd, b"cat dog cat", *sel) == want, sel
    xy = ("x*:y", "x*")
    for sel, want in (((0, -1), b"ybyby"), ((0, 1), b"ybb"), ((2, 1), b"bby"), ((3, 1), b"bb"), ((0, 0), b"bb")):
        assert one(*xy, b"bb", *sel) == want, sel
    assert one("[aie]:", "[aie]", b"a\0ie", 0, -1) == b"\0ie"
    assert one(",:;", ",", b"a,b\0c,d", 0, -1) == b"a;b\0c,d"
    out, off, n = sub_lib.Yardstick(*xy, [b"bb", b"", b"xx"]).expect(0, 1)
    assert (out, off, n) == (b"ybb" + b"y" + b"y", [0, 3, 4, 5], 3)
    out, off, n = sub_lib.Yardstick(*xy, [b"bb", b"", b"xx"]).expect(1, -1)
    assert (out, off, n) == (b"byby" + b"" + b"xxy", [0, 4, 4, 7], 3)


def test_nothing_selected_is_the_input():
    recs = sub_lib.corpus()
    for program, acceptor in sub_lib.PROGRAMS:
        y = sub_lib.Yardstick(program, acceptor, recs)
        for sel in ((0, 0), (1 << 62, -1), ((1 << 63) - 1, 1)):
            out, off, n = y.expect(*sel)
            assert out == b"".join(recs) and n == 0 and sub_lib.per_string(out, off) == recs, (program, sel)


# the pairs whose output is a literal: (program, acceptor, Python's pattern, Python's replacement)
LITERAL = [("a:xyz", "a", b"a", b"xyz"), (" +: ", " +", b" +", b" "), ("[a-z]+ing:X", "[a-z]+ing", b"[a-z]+ing", b"X"),
           ("(a|b)*c:x", "(a|b)*c", b"(?:a|b)*c", b"x"), ("[0-9]+:N", "[0-9]+", b"[0-9]+", b"N"), ("[aie]:", "[aie]", b"[aie]", b""),
           (",:;", ",", b",", b";")]


def test_the_expectation_is_re_sub():
    """first = 0 with count = c >= 1 is re.sub(p, r, s, count=c), and count < 0 is re.sub(p, r, s), on the NUL-free strings of the
    corpus.  Left out: (cat:dog|dog:cat), whose replacement depends on the match, and .*(cat:dog).*(a|b){4}, which replaces an
    inner group; x*:y, because Python lets an empty match follow a non-empty one at the same place and the scan loop does not
    ('xx': Python finds 'xx' and '', the scan loop 'xx' alone); count == 0, which Python reads as "all"; first > 0, which re.sub
    does not have (checked against a loop over re.finditer instead, below).  Python's leftmost match is the scan loop's, and its
    greedy length is the reference's for these patterns: each is one greedy class run or a literal."""
    recs = [r for r in sub_lib.corpus() if b"\0" not in r] + [b"a,b,,c", b",", b"12ab345", b"hotdog singing", b"  lead  trail "]
    for program, acceptor, pat, repl in LITERAL:
        y = sub_lib.Yardstick(program, acceptor, recs)
        for count in (1, 2, 3, -1):
            want = [re.sub(pat, repl, r, count=max(count, 0)) for r in recs]
            assert y.per_string(0, count) == want, (program, count)
        for first, count in ((1, 1), (2, -1), (1, 2)):
            want = []
            for r in recs:
                out, at = b"", 0
                for k, m in enumerate(re.finditer(pat, r)):
                    if sub_lib.selected(k, first, count):
                        out += r[at:m.start()] + repl
                        at = m.end()
                want.append(out + r[at:])
            assert y.per_string(first, count) == want, (program, first, count)


@pytest.mark.parametrize("program,acceptor", sub_lib.PROGRAMS + [(",:;", ",")])
def test_every_match_selected_is_the_plain_scan(program, acceptor):
    """(0, -1) on a string without a NUL is, byte for byte, the line the reference prints for it in scan mode"""
    recs = [r for r in sub_lib.corpus() if b"\0" not in r]
    plain = Oracle(program, "nft").scan(b"".join(r + b"\n" for r in recs)).split(b"\n")
    assert plain.pop() == b"" and len(plain) == len(recs)
    assert sub_lib.Yardstick(program, acceptor, recs).per_string(0, -1) == plain


def test_the_corpus_proves_something():
    recs = sub_lib.corpus()
    first_kind = second_kind = 0
    for program, acceptor in sub_lib.PROGRAMS:
        a, b = sub_lib.corpus_figures(sub_lib.Yardstick(program, acceptor, recs))
        if program == sub_lib.ONCE:
            assert (a, b) == (0, 0)
        elif (program, acceptor) in sub_lib.ADDED:
            assert a >= 1, program
        else:
            first_kind, second_kind = first_kind + a, second_kind + b
    assert first_kind >= 400 and second_kind >= 400, (first_kind, second_kind)


def test_the_mode_is_refused_for_the_deterministic_engine():
    with pytest.raises(trre_amd.TrreError) as e:
        trre_amd.Program("a:b", "dft", "sub")
    assert e.value.code == api.E_UNSUPPORTED and "non-deterministic engine only" in str(e.value)


@pytest.mark.parametrize("program,acceptor", sub_lib.PROGRAMS)
def test_the_tables_are_those_of_the_spans_and_the_find_program(program, acceptor):
    """which 0 (the backward DFA) and 7 (the markers' table) as a spans program answers them, 5 the find program's texts table,
    which that program walks over a backward DFA byte-identical to the spans program's"""
    sub, spans, find = (trre_amd.Program(program, "nft", m) for m in ("sub", "spans", "find"))
    assert sub._guided(0, 7) == spans._guided(0, 7) and all(sub._guided(0, 7))
    assert sub._guided(5) == find._guided(5) and sub._guided(5)[0]
    assert sub._guided(0) == find._guided(0)
    assert sub._guided(6) == (b"",)
    assert sub.info.guided_rev_states == spans.info.guided_rev_states


def test_the_layouts():
    states = {trre_amd.Program(p, "nft", "sub").info.guided_rev_states for p, _ in [sub_lib.PROGRAMS[8]] + sub_lib.ADDED}
    assert sorted((s > 256) + (s > 16) for s in states) == [0, 1, 2], states
