"""What the filter tests share (tests/test_filter_strings.py, tests/test_gpu_filter_strings.py): the yardstick.

The yardstick is the reference through the oracle, never the engine: tests/span_lib.py's Spanner gives a string's spans under
the wrapped acceptor, and by the definition of include/trre_mi355x.h string i is kept exactly when it has at least one span —
with invert, exactly when it has none.  A kept string is the UNCUT string: the search ends at a NUL, the copy does not."""


def keep(spans, invert=False):
    """per string: is it kept"""
    return [(len(w) > 0) != bool(invert) for w in spans]


def expect(lines, spans, invert=False):
    """the call's three arrays from the strings and their spans: (out bytes, out offsets, rows)"""
    out, oo, rows = b"", [0], []
    for i, (l, k) in enumerate(zip(lines, keep(spans, invert))):
        if k:
            out += l
            oo.append(len(out))
            rows.append(i)
    return out, oo, rows


def filter_lines(spanner, lines, invert=False):
    """the call's three arrays for `lines`, the spans from the oracle (span_lib.Spanner)"""
    return expect(lines, spanner.lines(lines), invert)


def kept_strings(out, oo):
    """the inverse: the kept strings from the call's arrays"""
    return [out[oo[r]:oo[r + 1]] for r in range(len(oo) - 1)]
