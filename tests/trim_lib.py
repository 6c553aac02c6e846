"""What the trim tests share (tests/test_trim_strings.py, tests/test_trim_shim.py, tests/test_gpu_trim_strings.py): the yardstick.

The yardstick is the reference through the oracle, never the engine: tests/span_lib.py's Spanner gives a string's spans under
the wrapped acceptor (the string cut at its first NUL), and the rule of include/trre_mi355x.h is applied to them with len the
UNCUT length:
    lo = max{ e_j : s_j == 0 }    (the left side asked for; default 0)
    hi = min{ s_j : e_j == len }  (the right side asked for; default len)
and the entry is s[lo : max(lo, hi)]."""
LEFT, RIGHT = 1, 2
BOTH = LEFT | RIGHT
SIDES = {"left": LEFT, "right": RIGHT, "both": BOTH}


def bounds(line, spans, left, right):
    """(lo, hi) of one string, relative to it, hi already max(lo, hi)"""
    n = len(line)
    lo = max([e for s, e in spans if s == 0], default=0) if left else 0
    hi = min([s for s, e in spans if e == n], default=n) if right else n
    return lo, max(lo, hi)


def trimmed(lines, spans, flags):
    """per string its entry"""
    got = []
    for l, w in zip(lines, spans):
        lo, hi = bounds(l, w, bool(flags & LEFT), bool(flags & RIGHT))
        got.append(l[lo:hi])
    return got


def expect(lines, spans, flags):
    """the call's four arrays from the strings and their spans: (out bytes, out offsets, begin, end), begin and end absolute"""
    out, oo, begin, end, at = b"", [0], [], [], 0
    for l, w in zip(lines, spans):
        lo, hi = bounds(l, w, bool(flags & LEFT), bool(flags & RIGHT))
        out += l[lo:hi]
        oo.append(len(out))
        begin.append(at + lo)
        end.append(at + hi)
        at += len(l)
    return out, oo, begin, end


def trim_lines(spanner, lines, flags):
    """the call's four arrays for `lines`, the spans from the oracle (span_lib.Spanner)"""
    return expect(lines, spanner.lines(lines), flags)
