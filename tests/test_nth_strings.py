"""Match k of every string (include/trre_mi355x.h: trre_nth_device_strings; Program.nth_strings / nth_list) without a GPU: the
yardstick of tests/nth_lib.py — find(s) by the oracle (tests/find_lib.py), indexed as Python indexes a list — against the
examples written out by hand and against re.search / re.findall for the patterns where Python's matches are the scan loop's."""
import re

import nth_lib
import sub_lib
import trre_amd
from find_lib import Finder
from test_sub_strings import LITERAL
from trre_amd import api


def entry(pat, s, k):
    return nth_lib.pick(Finder(pat)(s), k)


def test_library_exports_nth_symbol():
    assert hasattr(api.lib(), "trre_nth_device_strings")
    for name in ("nth_strings", "nth_list"):
        assert hasattr(trre_amd.Program, name)


def test_the_examples_by_hand():
    # empty matches count: an empty output with the bit set is not an absent match
    assert [entry("x*", b"bb", k) for k in range(4)] == [b"", b"", b"", None]
    assert [entry("x*", b"bb", k) for k in (-1, -3, -4, -(1 << 63))] == [b"", b"", None, None]
    assert entry("[aie]:", b"kiwi", 0) == b"" and entry("[aie]:", b"kiwi", 1) == b"" and entry("[aie]:", b"kiwi", 2) is None
    # the search ends at a NUL
    assert [entry("(cat|dog)", b"a cat\0dog", k) for k in (0, 1, -2)] == [b"cat", None, None]
    assert [entry("(cat:dog|dog:cat)", b"cat dog cat", k) for k in (0, 1, -1)] == [b"dog", b"cat", b"dog"]
    # an empty string: what an empty line's one attempt prints, or nothing
    assert entry(":x", b"", 0) == b"x" and entry(":x", b"", -1) == b"x" and entry(":x", b"", 1) is None
    assert entry("a+", b"", 0) is None and entry("a+", b"", -1) is None
    # the three arrays
    lists = Finder("x*").lines([b"bb", b"", b"xxbx"])
    assert lists == [[b"", b"", b""], [b""], [b"xx", b"", b"x", b""]]
    assert nth_lib.expect(lists, 0) == (b"xx", [0, 0, 0, 2], [True, True, True])
    assert nth_lib.expect(lists, 2) == (b"x", [0, 0, 0, 1], [True, False, True])
    assert nth_lib.expect(lists, -4) == (b"xx", [0, 0, 0, 2], [False, False, True])
    assert nth_lib.expect(lists, -(1 << 63)) == (b"", [0, 0, 0, 0], [False] * 3)
    assert nth_lib.per_string(*nth_lib.expect(lists, 1)) == [b"", None, b""]
    assert nth_lib.bitmap([True, False, True]) == bytes([5, 0, 0, 0, 0, 0, 0, 0])


def test_the_expectation_is_re_search_and_findall():
    """under an identity pattern a match's output is the match: entry 0 is re.search(p, s).group(), entry k is
    re.findall(p, s)[k], on the NUL-free strings of the sub tests' corpus — for the acceptors whose Python matches are the scan
    loop's (each one greedy class run or a literal: test_sub_strings.LITERAL)"""
    recs = [r for r in sub_lib.corpus() if b"\0" not in r] + [b"a,b,,c", b",", b"12ab345", b"hotdog singing", b"  lead  trail "]
    n_valid = n_absent = 0
    for _, acceptor, pat, _ in LITERAL:
        lists = Finder(acceptor).lines(recs)
        found = [[m.group() for m in re.finditer(pat, r)] for r in recs]
        assert lists == found, acceptor
        for k in (0, 1, 2, -1, -2, 5, -(1 << 63)):
            got = nth_lib.per_string(*nth_lib.expect(lists, k))
            assert got == [nth_lib.pick(f, k) for f in found], (acceptor, k)
            n_valid += sum(g is not None for g in got)
            n_absent += sum(g is None for g in got)
        first = [m.group() if m else None for m in (re.search(pat, r) for r in recs)]
        assert nth_lib.per_string(*nth_lib.expect(lists, 0)) == first, acceptor
    assert n_valid > 100 and n_absent > 100, (n_valid, n_absent)
