"""What the find-mode tests share (tests/test_find_strings.py, tests/test_gpu_find_strings.py): the yardstick.

find(s), the list of the outputs of the scan loop's successful attempts on the line s, is read off the oracle: with A = 0x01,
B = 0x02 and W = (:A)(P)(:B), every successful attempt of P prints A, its output, B, so the pieces between A and B in what the
oracle prints for W are find(s) — provided neither the data nor the program's own output holds a marker byte, and provided W
scans like P, which is checked: the wrapped output with the markers stripped is the plain oracle's output, and the markers
nest.  A program that prints no '\\n' of its own prints exactly one per line, so one scan of many lines splits into the lines'."""
import golden_lib
from oracle_lib import Oracle, OracleError

A, B = b"\x01", b"\x02"
# patterns beyond the golden set: more than 16 backward states (a byte per symbol), exactly 16 (the last nibble-packed size), more
# than 256 (16-bit symbols) — in this build 19, 16 and 772
WIDE = "[a-h]{8}(a|b)[a-z ]*"
EXTRA = [".*(cat:dog).*(a|b){4}", "(a|b)*a(a|b){5}", WIDE]


def _b(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def wrapped(pat):
    return b"(:" + A + b")(" + _b(pat) + b")(:" + B + b")"


def pieces(line_out):
    """the pieces between A and B of one line's wrapped output, or None when the markers do not nest"""
    out, at = [], 0
    while True:
        a = line_out.find(A, at)
        if a < 0:
            return out if B not in line_out[at:] else None
        if B in line_out[at:a]:
            return None
        b = line_out.find(B, a + 1)
        if b < 0 or A in line_out[a + 1:b]:
            return None
        out.append(line_out[a + 1:b])
        at = b + 1


class Finder:
    """find() by the oracle, for lines that hold no marker byte"""

    def __init__(self, pat):
        self.pat = pat
        self.o = Oracle(wrapped(pat), "nft")
        self.seen = {}

    def lines(self, lines):
        """[find(l) for l in lines], by one scan; OracleError when the reference does not survive it"""
        assert not any(b"\n" in l or A in l or B in l for l in lines)
        if not lines:
            return []
        out = self.o.scan(b"".join(l + b"\n" for l in lines))
        per = out.split(b"\n")
        assert per.pop() == b"" and len(per) == len(lines), (self.pat, len(per), len(lines))
        got = [pieces(x) for x in per]
        assert None not in got, self.pat
        return got

    def __call__(self, line):
        if line not in self.seen:
            self.seen[line] = self.lines([line])[0]
        return self.seen[line]


def lines_of(data):
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


_vectors = None


def vectors():
    """The NFT golden scan vectors, sorted by the yardstick: (usable, dead, left_out, n) — usable: (pattern, name, data) on which
    the identity holds; dead: the ones the reference does not survive; left_out: (pattern, name, why) — a marker byte in the
    pattern, the data or the output, or the identity fails (the reference's grammar reads a trailing colon differently inside
    parentheses: 'ab:')."""
    global _vectors
    if _vectors is None:
        usable, dead, left_out, n = [], [], [], 0
        plain, wrap = {}, {}
        for pat, name, data, engine, exp in golden_lib.cases():
            if engine != "nft":
                continue
            n += 1
            if exp is None:
                dead.append((pat, name, data))
                continue
            if A in _b(pat) or B in _b(pat) or A in data or B in data or A in exp or B in exp:
                left_out.append((pat, name, "marker"))
                continue
            try:
                if pat not in wrap:
                    wrap[pat] = Oracle(wrapped(pat), "nft")
                w = wrap[pat].scan(data)
            except OracleError:
                left_out.append((pat, name, "wrapped fails"))
                continue
            ok = w.replace(A, b"").replace(B, b"") == exp and all(pieces(x) is not None for x in w.split(b"\n"))
            if ok:
                usable.append((pat, name, data))
            else:
                left_out.append((pat, name, "identity"))
        _vectors = (usable, dead, left_out, n)
    return _vectors


def prints_newline(pat):
    """can the program print a '\\n' of its own (then a scan's output does not split into its lines')"""
    return b"\n" in _b(pat).split(b":", 1)[-1] if b":" in _b(pat) else False
