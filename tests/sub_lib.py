"""What the sub-mode tests share (tests/test_sub_strings.py, tests/test_gpu_sub_strings.py): the yardstick, the programs and the
corpus.

The yardstick is composed in Python from the reference through the oracle, never the engine and never the shim: the spans of a
string come from span_lib.Spanner under the program's input projection, the outputs of its matches from find_lib.Finder under
the program itself (the string cut at its first NUL, as the search sees it), and the two must agree on the number of matches of
every string.  Match r of a string is selected when first <= r and (count < 0 or r - first < count); the output is the string
with every selected match replaced by its output — an output that holds a NUL ends before it, as fputs prints it — and everything
else kept, a NUL and what is behind it included."""
import random

import find_lib
import span_lib

# a program with output <-> its input projection: the pairs of the span tests, and the two other symbol layouts (in this build the
# backward automata of the last three have 35, 16 and 772 states: a byte per symbol, nibbles, 16-bit symbols)
ONCE = ".*(cat:dog).*(a|b){4}"                       # matches at most once per string
ADDED = [("((a|b)*a(a|b){5}):X", "(a|b)*a(a|b){5}"), ("([a-h]{8}(a|b)[a-z ]*):W", "[a-h]{8}(a|b)[a-z ]*")]
PROGRAMS = span_lib.PAIRS + ADDED

TOKENS = [b"cat", b"dog", b"sing", b"thing", b"aabbaa", b"abab", b"12", b"7", b" ", b"  ", b"xx", b"abcdefgha", b"c", b"aie",
          b"aaaaaab", b"0", b"q", b"t"]
NUL_STRINGS = [b"", b"a\0cat", b"\0", b"cat\0", b"cat dog\0cat", b"1 2\0 3"]
SELECTIONS = [(0, -1), (0, 1), (1, 1), (2, -1), (0, 0), (5, 2), ((1 << 63) - 1, 1), (0, -(1 << 63))]


def corpus():
    rng = random.Random(291)
    return [b"".join(rng.choice(TOKENS) for _ in range(rng.randrange(9))) for _ in range(300)] + NUL_STRINGS


def selected(r, first, count):
    return first <= r and (count < 0 or r - first < count)


def printed(o):
    """what fputs prints of a match's output"""
    k = o.find(b"\0")
    return o if k < 0 else o[:k]


def sub(rec, spans, outs, first, count):
    """one string: spans relative to it, outs its matches' outputs"""
    assert len(spans) == len(outs), (rec, spans, outs)
    out, at = b"", 0
    for r, ((s, e), o) in enumerate(zip(spans, outs)):
        if selected(r, first, count):
            out += rec[at:s] + printed(o)
            at = e
    return out + rec[at:]


def expect(recs, spans, outs, first, count):
    """(the outputs concatenated, their nrec + 1 offsets, the number of selected matches)"""
    per = [sub(r, s, o, first, count) for r, s, o in zip(recs, spans, outs)]
    off = [0]
    for x in per:
        off.append(off[-1] + len(x))
    return b"".join(per), off, sum(selected(r, first, count) for s in spans for r in range(len(s)))


class Yardstick:
    """the spans and the outputs of a list of strings under (program, acceptor), once; then expect() for any selection"""

    def __init__(self, program, acceptor, recs):
        self.recs = list(recs)
        self.spans = span_lib.Spanner(acceptor).lines(self.recs)
        self.outs = find_lib.Finder(program).lines([span_lib.cut(r) for r in self.recs])
        for r, s, o in zip(self.recs, self.spans, self.outs):
            assert len(s) == len(o), (program, r, s, o)

    def expect(self, first, count):
        return expect(self.recs, self.spans, self.outs, first, count)

    def per_string(self, first, count):
        return [sub(r, s, o, first, count) for r, s, o in zip(self.recs, self.spans, self.outs)]


def corpus_figures(y):
    """(strings where (0, 1) differs from (0, -1); strings where (1, 1) differs from both the input and (0, -1))"""
    every, one, second = y.per_string(0, -1), y.per_string(0, 1), y.per_string(1, 1)
    return (sum(a != b for a, b in zip(one, every)),
            sum(s != r and s != a for s, r, a in zip(second, y.recs, every)))


def per_string(out, off):
    return [out[off[i]:off[i + 1]] for i in range(len(off) - 1)]
