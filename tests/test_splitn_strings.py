"""Split strings at the first or last matches only (include/trre_mi355x.h: trre_splitn_device_strings, trre_fieldn_device_strings;
Program.split_strings / field_strings with limit= and from_end=) without a GPU: the yardstick of tests/splitn_lib.py by hand, and
against Python where the syntax coincides — re.split(p, s, maxsplit=L) for L >= 1, s.split(sep, L) and s.rsplit(sep, L) for
literal separators, str.partition and str.rpartition.  The spans come from the oracle (span_lib.Spanner).  Apart from the first
test, which asks the binding for the symbols and the keywords, this file checks the YARDSTICK and nothing of the library: the
library's own rule (records_block.hpp: splitn_cuts) is held against this yardstick by tests/test_splitn_shim.py, its kernels on the
host there and on the device by tests/test_gpu_splitn_strings.py."""
import inspect
import random
import re

import field_lib
import splitn_lib
import trre_amd
from span_lib import Spanner
from splitn_lib import INT64_MAX, INT64_MIN, pieces
from trre_amd import api


def test_the_binding_has_the_symbols_and_the_keywords():
    for name in ("trre_splitn_device_strings", "trre_fieldn_device_strings"):
        assert hasattr(api.lib(), name)
    for name in ("split_strings", "split_list", "field_strings", "field_list"):
        sig = inspect.signature(getattr(trre_amd.Program, name))
        for key, default in (("limit", -1), ("from_end", False)):
            assert sig.parameters[key].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[key].default == default, (name, key)


def test_the_rule():
    """limit is compared, never added or negated"""
    for c in range(6):
        for limit in (0, 1, 2, 5, 6, INT64_MAX, -1, INT64_MIN):
            for from_end in (False, True):
                got = [splitn_lib.cuts(r, c, limit, from_end) for r in range(c)]
                cc = c if limit < 0 else min(c, limit)
                assert got == ([False] * (c - cc) + [True] * cc if from_end else [True] * cc + [False] * (c - cc)), (c, limit, from_end)


def test_by_hand():
    eq, dot, xs = Spanner("="), Spanner("\\."), Spanner("x*")
    assert pieces(b"a=b=c", eq(b"a=b=c"), 1, False) == [b"a", b"b=c"]
    assert pieces(b"a=b=c", eq(b"a=b=c"), 1, True) == [b"a=b", b"c"]
    assert pieces(b"a=b=c", eq(b"a=b=c"), 0, False) == [b"a=b=c"] == pieces(b"a=b=c", eq(b"a=b=c"), 0, True)
    for limit in (2, 3, INT64_MAX, -1, INT64_MIN):
        for from_end in (False, True):
            assert pieces(b"a=b=c", eq(b"a=b=c"), limit, from_end) == [b"a", b"b", b"c"]
    assert pieces(b"x.tar.gz", dot(b"x.tar.gz"), 1, True) == [b"x.tar", b"gz"]
    assert pieces(b"x.tar.gz", dot(b"x.tar.gz"), 1, False) == [b"x", b"tar.gz"]
    assert pieces(b"noext", dot(b"noext"), 1, True) == [b"noext"]
    # 'x*' on "bb": the empty matches at 0, 1 and 2 — an empty cutting match yields an empty piece, one that does not cut nothing
    assert xs(b"bb") == [(0, 0), (1, 1), (2, 2)]
    front = {0: [b"bb"], 1: [b"", b"bb"], 2: [b"", b"b", b"b"], 3: [b"", b"b", b"b", b""], 4: [b"", b"b", b"b", b""]}
    back = {0: [b"bb"], 1: [b"bb", b""], 2: [b"b", b"b", b""], 3: [b"", b"b", b"b", b""], 4: [b"", b"b", b"b", b""]}
    for limit in range(5):
        assert pieces(b"bb", xs(b"bb"), limit, False) == front[limit], limit
        assert pieces(b"bb", xs(b"bb"), limit, True) == back[limit], limit


def test_a_nul_and_everything_behind_it_stays_in_the_last_piece():
    comma = Spanner(",")
    line = b"a,b\0c,d"
    assert comma(line) == [(1, 2)]
    assert pieces(line, comma(line), 1, False) == [b"a", b"b\0c,d"] == pieces(line, comma(line), 1, True)
    assert pieces(line, comma(line), 0, True) == [line]
    assert pieces(b"\0,x", comma(b"\0,x"), 1, False) == [b"\0,x"]
    assert pieces(b"a,b,c\0", comma(b"a,b,c\0"), 1, True) == [b"a,b", b"c\0"]
    assert pieces(b"a,b,c\0", comma(b"a,b,c\0"), 1, False) == [b"a", b"b,c\0"]


def soup(rng, alphabet, count, longest):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randrange(longest))) for _ in range(count)]


def test_against_re_split_with_maxsplit():
    rng = random.Random(7)
    for pat, py, alphabet in ((",", b",", b"ab,"), ("[0-9]+", b"[0-9]+", b"ab12 "), (" +", b" +", b"xy  "), ("(cat|dog)", b"(?:cat|dog)", b"catdog ")):
        lines = soup(rng, alphabet, 120, 14) + [b""]
        spans = Spanner(pat).lines(lines)
        for L in (1, 2, 3, 7):
            assert [pieces(l, w, L, False) for l, w in zip(lines, spans)] == [re.split(py, l, maxsplit=L) for l in lines], (pat, L)
        assert [pieces(l, w, -1, False) for l, w in zip(lines, spans)] == [re.split(py, l) for l in lines], pat


def test_against_str_split_rsplit_and_partition():
    rng = random.Random(8)
    for sep, pat, alphabet in ((b"=", "=", b"ab="), (b".", "\\.", b"xy."), (b", ", ", ", b"a, ,")):
        lines = soup(rng, alphabet, 150, 12) + [b"", sep, sep + sep]
        spans = Spanner(pat).lines(lines)
        for L in (0, 1, 2, 3, 20):
            assert [pieces(l, w, L, False) for l, w in zip(lines, spans)] == [l.split(sep, L) for l in lines], (sep, L)
            if len(sep) == 1:              # (a longer separator that overlaps itself is found from the right by rsplit, from the left here)
                assert [pieces(l, w, L, True) for l, w in zip(lines, spans)] == [l.rsplit(sep, L) for l in lines], (sep, L)
        for l, w in zip(lines, spans):
            head, mid, tail = l.partition(sep)
            assert [field_lib.pick(pieces(l, w, 1, False), k) for k in (0, 1)] == [head, tail if mid else None], l
            if len(sep) == 1:
                head, mid, tail = l.rpartition(sep)
                assert [field_lib.pick(pieces(l, w, 1, True), k) for k in (0, 1)] == ([head, tail] if mid else [l, None]), l


def test_expect_and_the_field_by_index():
    lines = [b"a=b=c", b"", b"=", b"k=v"]
    spans = Spanner("=").lines(lines)
    assert splitn_lib.expect(lines, spans, 1, False) == (b"ab=ckv", [0, 1, 4, 4, 4, 4, 5, 6], [0, 2, 3, 5, 7])
    assert splitn_lib.expect(lines, spans, 0, True) == (b"a=b=c=k=v", [0, 5, 5, 6, 9], [0, 1, 2, 3, 4])
    assert splitn_lib.expect_field(lines, spans, 1, 1, False) == (b"b=cv", [0, 3, 3, 3, 4], [True, False, True, True])
    assert splitn_lib.expect_field(lines, spans, 0, 1, True) == (b"a=bk", [0, 3, 3, 3, 4], [True, True, True, True])
    assert splitn_lib.expect_field(lines, spans, -2, 1, True) == splitn_lib.expect_field(lines, spans, 0, 1, True)[:2] + ([True, False, True, True],)
    assert splitn_lib.expect_field(lines, spans, 2, 1, False) == (b"", [0, 0, 0, 0, 0], [False] * 4)
    # field k of the limited split by the header's index arithmetic: kk, m0 and the spans' ends
    for limit in splitn_lib.limits_of(2):
        for from_end in (False, True):
            for k in (0, 1, -1, -2, 2, 3, -3, -4, INT64_MIN, INT64_MAX):
                for l, w in zip(lines, spans):
                    c = len(w)
                    cc = c if limit < 0 else min(c, limit)
                    m0 = c - cc if from_end else 0
                    kk = k if k >= 0 else cc + 1 + k
                    want = None
                    if 0 <= kk <= cc:
                        want = l[(0 if kk == 0 else w[m0 + kk - 1][1]):(len(l) if kk == cc else w[m0 + kk][0])]
                    assert field_lib.pick(pieces(l, w, limit, from_end), k) == want, (l, limit, from_end, k)
