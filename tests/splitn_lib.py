"""What the limited-split tests share (tests/test_splitn_strings.py, tests/test_splitn_shim.py, tests/test_gpu_splitn_strings.py):
the yardstick.

The yardstick is the reference through the oracle, never the engine: tests/span_lib.py's Spanner gives a string's spans
(s_0,e_0) .. (s_{c-1},e_{c-1}) under the wrapped acceptor, the cut rule of include/trre_mi355x.h is applied here, in Python —
match r cuts exactly when limit < 0, or from the front and r < limit, or from the end and c - r <= limit — and tests/split_lib.py's
cut_pieces cuts the UNCUT string at the CUTTING spans only: a match that does not cut stays in its piece, and the last piece
keeps a NUL and everything behind it.  Field k is Python's own indexing of that list."""
import field_lib
import split_lib
from split_lib import cut_pieces

INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def cuts(r, c, limit, from_end):
    """THE RULE: does match r of a string's c matches cut"""
    if limit < 0:
        return True
    return c - r <= limit if from_end else r < limit


def cutting(spans, limit, from_end):
    """the spans that cut, in order"""
    c = len(spans)
    return [w for r, w in enumerate(spans) if cuts(r, c, limit, from_end)]


def pieces(line, spans, limit, from_end):
    """the cc + 1 pieces of the uncut string `line`"""
    return cut_pieces(line, cutting(spans, limit, from_end))


def split_lines(spanner, lines, limit, from_end):
    """per string the list of its pieces, the spans from the oracle (span_lib.Spanner)"""
    return [pieces(l, w, limit, from_end) for l, w in zip(lines, spanner.lines(lines))]


def expect(lines, spans, limit, from_end):
    """the split form's three arrays: (out bytes, piece offsets, list offsets)"""
    return split_lib.expect([pieces(l, w, limit, from_end) for l, w in zip(lines, spans)])


def expect_field(lines, spans, k, limit, from_end):
    """the field form's three arrays: (out bytes, out offsets, valid)"""
    out, oo, valid = b"", [0], []
    for l, w in zip(lines, spans):
        f = field_lib.pick(pieces(l, w, limit, from_end), k)
        out += f or b""
        oo.append(len(out))
        valid.append(f is not None)
    return out, oo, valid


def limits_of(c):
    """the limits worth a run on strings of up to c matches"""
    return sorted({0, 1, 2, max(c - 1, 0), c, c + 1, INT64_MAX, -1, INT64_MIN})
