"""What the spans-mode tests share (tests/test_span_strings.py, tests/test_gpu_span_strings.py): the yardstick.

The yardstick is the reference through the oracle, never the engine.  For a pattern P without output (no ':' in it: a pure
acceptor) the oracle's scan of W = (:A)(P)(:B), A = 0x01, B = 0x02, on a line copies every input byte and brackets every
match: the markers stripped give the line back — asserted on every line used — and then, for match j of the line,
    start_j = pos(A_j) - 2 j,    end_j = pos(B_j) - 2 j - 1.
For a program with output the yardstick is its input projection, written by hand (PAIRS): the acceptor that consumes what the
program consumes.  A line is cut at its first NUL before the oracle sees it: the reference's search ends there.

The wide, weaker check works on any program: the number of A..B pieces of W's output on a line is the number of matches, and
what W's output holds outside its A..B pieces is the raw bytes — the bytes of the line outside its spans."""
import find_lib
from find_lib import A, B, _b, wrapped
from oracle_lib import Oracle

# a program with output <-> its input projection
PAIRS = [("(cat:dog|dog:cat)", "(cat|dog)"), ("a:xyz", "a"), (" +: ", " +"), ("[a-z]+ing:X", "[a-z]+ing"), ("(a|b)*c:x", "(a|b)*c"),
         ("[0-9]+:N", "[0-9]+"), ("x*:y", "x*"), ("[aie]:", "[aie]"), (".*(cat:dog).*(a|b){4}", ".*(cat).*(a|b){4}")]
# the three symbol layouts (a byte per symbol; the last nibble-packed size; 16-bit symbols): the first through its pair, the
# other two are acceptors themselves
LAYOUTS = [(".*(cat:dog).*(a|b){4}", ".*(cat).*(a|b){4}"), ("(a|b)*a(a|b){5}", "(a|b)*a(a|b){5}"), (find_lib.WIDE, find_lib.WIDE)]


def is_acceptor(pat):
    return b":" not in _b(pat)


def cut(line):
    """the part of a string the reference's search sees"""
    k = line.find(b"\0")
    return line if k < 0 else line[:k]


class Spanner:
    """spans by the oracle under an acceptor, for lines that hold no marker byte and no newline: per line a list of (start, end)
    relative to the line"""

    def __init__(self, acceptor):
        assert is_acceptor(acceptor), acceptor
        self.pat = acceptor
        self.o = Oracle(wrapped(acceptor), "nft")
        self.seen = {}

    def lines(self, lines):
        """OracleError when the reference does not survive the scan"""
        assert not any(b"\n" in l or A in l or B in l for l in lines)
        if not lines:
            return []
        cuts = [cut(l) for l in lines]
        per = self.o.scan(b"".join(l + b"\n" for l in cuts)).split(b"\n")
        assert per.pop() == b"" and len(per) == len(lines), (self.pat, len(per), len(lines))
        got = []
        for l, w in zip(cuts, per):
            assert w.replace(A, b"").replace(B, b"") == l, (self.pat, l, w)           # the identity the arithmetic rests on
            spans, j, at = [], 0, 0
            while True:
                a = w.find(A, at)
                if a < 0:
                    assert B not in w[at:], (self.pat, l, w)
                    break
                b = w.find(B, a + 1)
                assert b > a and A not in w[a + 1:b] and B not in w[at:a], (self.pat, l, w)
                spans.append((a - 2 * j, b - 2 * j - 1))
                j, at = j + 1, b + 1
            got.append(spans)
        return got

    def __call__(self, line):
        if line not in self.seen:
            self.seen[line] = self.lines([line])[0]
        return self.seen[line]


class Weak:
    """for any program: per line (number of matches, the raw bytes between and around them), from W's output"""

    def __init__(self, pat):
        self.pat = pat
        self.o = Oracle(wrapped(pat), "nft")

    def lines(self, lines):
        assert not any(b"\n" in l or A in l or B in l for l in lines)
        if not lines:
            return []
        per = self.o.scan(b"".join(cut(l) + b"\n" for l in lines)).split(b"\n")
        assert per.pop() == b"" and len(per) == len(lines), (self.pat, len(per), len(lines))
        got = []
        for w in per:
            raw, n, at = b"", 0, 0
            while True:
                a = w.find(A, at)
                if a < 0:
                    raw += w[at:]
                    break
                b = w.find(B, a + 1)
                assert b > a, (self.pat, w)
                raw += w[at:a]
                n, at = n + 1, b + 1
            got.append((n, raw))
        return got


def gaps(line, spans):
    """the bytes of a line (cut at its NUL) outside its spans"""
    l, out, at = cut(line), b"", 0
    for s, e in spans:
        out += l[at:s]
        at = e
    return out + l[at:]


def pack(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off


def expect(per, off):
    """the call's three arrays from per-string relative spans: (starts, ends, list offsets), positions absolute"""
    starts = [off[i] + s for i, w in enumerate(per) for s, _ in w]
    ends = [off[i] + e for i, w in enumerate(per) for _, e in w]
    lo = [0]
    for w in per:
        lo.append(lo[-1] + len(w))
    return starts, ends, lo


def relative(starts, ends, lo, off):
    """the inverse: per-string relative spans from the call's arrays"""
    return [[(starts[j] - off[i], ends[j] - off[i]) for j in range(lo[i], lo[i + 1])] for i in range(len(off) - 1)]


def golden_acceptors():
    """the usable golden vectors whose pattern is an acceptor: {pattern: [(name, lines)]}"""
    usable, _, _, _ = find_lib.vectors()
    by = {}
    for pat, name, data in usable:
        if is_acceptor(pat):
            by.setdefault(pat, []).append((name, find_lib.lines_of(data)))
    return by
