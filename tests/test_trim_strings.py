"""Trimmed strings (include/trre_mi355x.h: trre_trim_device_strings; Program.trim_strings / trim_ranges / trim_list) without a
GPU: the definition of tests/trim_lib.py — lo = max{e_j : s_j == 0}, hi = min{s_j : e_j == len} on the oracle's spans — by hand,
against Python's re (re.match(P, s).end() on the left, re.search(P + rb'\\Z', s).start() on the right) for six acceptors on random
strings, and against bytes.strip / lstrip / rstrip; a guard that those strings exercise the rule; and the paired patterns: a
program with output trims as its input projection."""
import random
import re

import pytest

import span_lib
import trim_lib
import trre_amd
from span_lib import PAIRS, Spanner, Weak
from trim_lib import BOTH, LEFT, RIGHT
from trre_amd import api

# acceptor, the same pattern for re, what the random strings are made of
ACCEPTORS = [("x*", rb"x*", (b"x", b"b")), (" +", rb" +", (b" ", b"a")), ("[ \t]+", rb"[ \t]+", (b" ", b"\t", b"a", b"b")),
             ("(cat|dog)", rb"(?:cat|dog)", (b"cat", b"dog", b"x", b"g")), ("[0-9]+", rb"[0-9]+", (b"1", b"2", b"a", b"b")),
             ("a+", rb"a+", (b"a", b"b"))]


def strings(seed, parts, count=400):
    rng = random.Random(seed)
    return [b"".join(rng.choice(parts) for _ in range(rng.randrange(0, 7))) for _ in range(count)]


def by_re(repat, s, flags):
    """the entry as Python's re gives it: one match anchored at the start, one anchored at the end"""
    lo, hi = 0, len(s)
    if flags & LEFT:
        m = re.match(repat, s)
        lo = m.end() if m else 0
    if flags & RIGHT:
        m = re.search(repat + rb"\Z", s)
        hi = m.start() if m else len(s)
    return s[lo:max(lo, hi)]


def test_library_exports_trim_symbol():
    assert hasattr(api.lib(), "trre_trim_device_strings")
    for name in ("trim_strings", "trim_ranges", "trim_list"):
        assert hasattr(trre_amd.Program, name)
    assert (api.TRIM_LEFT, api.TRIM_RIGHT) == (LEFT, RIGHT)


def test_side_is_checked_before_the_library_is_called():
    p = trre_amd.Program(" +", "nft", "spans")
    for side in ("", "BOTH", "middle", None, 3):
        for call in (lambda: p.trim_list([b" a "], side=side), lambda: p.trim_strings(None, None, side=side),
                     lambda: p.trim_ranges(None, None, side=side)):
            with pytest.raises(ValueError):
                call()


def test_by_hand():
    def both(pat, lines):
        return trim_lib.trimmed(lines, Spanner(pat).lines(lines), BOTH)
    assert Spanner("x*")(b"xxbxx") == [(0, 2), (2, 2), (3, 5), (5, 5)]                 # two matches end at 5: the min decides
    assert both("x*", [b"xxbxx", b"bxx", b"xx", b"xxb\0xx", b"", b"b"]) == [b"b", b"b", b"", b"b\0xx", b"", b"b"]
    assert both(" +", [b"  a  b  ", b" a\0 ", b"   ", b"a"]) == [b"a  b", b"a\0 ", b"", b"a"]
    assert both("(cat|dog)", [b"catxdog", b"xcat", b"catx", b"dogcat", b"catdogcat"]) == [b"x", b"x", b"x", b"", b"dog"]
    assert both("[0-9]+", [b"12ab34", b"ab", b"7"]) == [b"ab", b"ab", b""]
    lines = [b"  a  b  ", b"xx", b" a\0 "]
    sp = Spanner(" +").lines(lines)
    assert trim_lib.trimmed(lines, sp, LEFT) == [b"a  b  ", b"xx", b"a\0 "]
    assert trim_lib.trimmed(lines, sp, RIGHT) == [b"  a  b", b"xx", b" a\0 "]           # a NUL: never trimmed on the right
    # one match is the whole string: lo = len, hi = 0, the entry s[len:len]
    assert trim_lib.bounds(b"   ", Spanner(" +")(b"   "), True, True) == (3, 3)
    assert trim_lib.bounds(b"dogcat", Spanner("(cat|dog)")(b"dogcat"), True, True) == (3, 3)
    assert trim_lib.expect([b" a", b"", b"b  "], [[(0, 1)], [], [(1, 3)]], BOTH) == (b"ab", [0, 1, 1, 2], [1, 2, 2], [2, 2, 3])


@pytest.mark.parametrize("which", range(len(ACCEPTORS)))
def test_the_rule_against_re(which):
    """400 random short strings per acceptor: the rule on the oracle's spans is what re's two anchored matches give, for every
    side; the strings exercise it — at least a quarter are changed by each side, at least a tenth are left whole — and a string
    with two matches ending at its end is there exactly for the acceptors that accept the empty string"""
    pat, repat, parts = ACCEPTORS[which]
    lines = strings(700 + which, parts)
    spans = Spanner(pat).lines(lines)
    for flags in (LEFT, RIGHT, BOTH):
        got = trim_lib.trimmed(lines, spans, flags)
        assert got == [by_re(repat, l, flags) for l in lines], (pat, flags)
        out, oo, begin, end = trim_lib.expect(lines, spans, flags)
        data, off = span_lib.pack(lines)
        assert [out[oo[i]:oo[i + 1]] for i in range(len(lines))] == got == [data[b:e] for b, e in zip(begin, end)]
        assert all(off[i] <= begin[i] <= end[i] <= off[i + 1] for i in range(len(lines)))
    left, right, both = (trim_lib.trimmed(lines, spans, f) for f in (LEFT, RIGHT, BOTH))
    n_left = sum(a != l for a, l in zip(left, lines))
    n_right = sum(a != l for a, l in zip(right, lines))
    n_whole = sum(a == l for a, l in zip(both, lines))
    assert n_left >= 100 and n_right >= 100 and n_whole >= 40, (pat, n_left, n_right, n_whole)
    two_at_the_end = sum(1 for l, w in zip(lines, spans) if sum(1 for _, e in w if e == len(l)) == 2)
    assert all(sum(1 for _, e in w if e == len(l)) <= 2 and sum(1 for s, _ in w if s == 0) <= 1 for l, w in zip(lines, spans))
    assert (two_at_the_end >= 1) == (re.fullmatch(repat, b"") is not None), (pat, two_at_the_end)


def test_against_bytes_strip():
    lines = strings(711, (b" ", b"\t", b"a", b"b", b"c d"))
    spans = Spanner("[ \t]+").lines(lines)
    assert trim_lib.trimmed(lines, spans, BOTH) == [l.strip(b" \t") for l in lines]
    assert trim_lib.trimmed(lines, spans, LEFT) == [l.lstrip(b" \t") for l in lines]
    assert trim_lib.trimmed(lines, spans, RIGHT) == [l.rstrip(b" \t") for l in lines]
    assert sum(l != l.strip(b" \t") for l in lines) >= 100


def test_a_program_with_output_trims_as_its_input_projection():
    """PAIRS: the program and its projection have the same matches on every line — as many, with the same bytes outside them
    (span_lib.Weak works on any program) — so the projection's spans are the yardstick of the program's trim: what it prints plays
    no part"""
    rng = random.Random(712)
    for prog, acc in PAIRS:
        lines = [bytes(rng.choice(b"abcdefgh ingxt059") for _ in range(rng.randrange(0, 12))) for _ in range(150)] + \
                [b"catdog", b"  a  ", b"xxbxx", b"12ab34", b"sing", b"aaa", b"", b"xcat aabb", b"the cat sat abab."]
        spans = Spanner(acc).lines(lines)
        assert Weak(prog).lines(lines) == [(len(w), span_lib.gaps(l, w)) for l, w in zip(lines, spans)], prog
        for flags in (LEFT, RIGHT, BOTH):
            got = trim_lib.trimmed(lines, spans, flags)
            assert all(l.find(g) >= 0 and len(g) <= len(l) for g, l in zip(got, lines)), prog
        assert any(g != l for g, l in zip(trim_lib.trimmed(lines, spans, BOTH), lines)), prog
