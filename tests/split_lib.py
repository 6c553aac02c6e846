"""What the split tests share (tests/test_split_strings.py, tests/test_gpu_split_strings.py): the yardstick.

The yardstick is the reference through the oracle, never the engine: tests/span_lib.py's Spanner gives a string's spans
(s_0,e_0) .. (s_{c-1},e_{c-1}) under the wrapped acceptor, and the pieces are cut here, in Python, from the UNCUT string s by the
definition of include/trre_mi355x.h: s[0:s_0], s[e_0:s_1], .., s[e_{c-1}:len(s)] — the last piece keeps a NUL and everything
behind it, since the search ends there and finds no span beyond."""


def cut_pieces(line, spans):
    """the c + 1 pieces of the uncut string `line` under its c ordered, disjoint spans"""
    out, at = [], 0
    for s, e in spans:
        assert at <= s <= e <= len(line), (line, spans)
        out.append(line[at:s])
        at = e
    out.append(line[at:])
    return out


def split_lines(spanner, lines):
    """per string the list of its pieces, the spans from the oracle (span_lib.Spanner)"""
    return [cut_pieces(l, sp) for l, sp in zip(lines, spanner.lines(lines))]


def expect(per):
    """the call's three arrays from per-string pieces: (out bytes, piece offsets, list offsets)"""
    out, po, lo = b"", [0], [0]
    for pieces in per:
        for piece in pieces:
            out += piece
            po.append(len(out))
        lo.append(lo[-1] + len(pieces))
    return out, po, lo


def per_string(out, po, lo):
    """the inverse: per-string pieces from the call's arrays"""
    return [[out[po[k]:po[k + 1]] for k in range(lo[i], lo[i + 1])] for i in range(len(lo) - 1)]


def nul_tail(line):
    """whatever lies from a string's first NUL on (the part the search does not see)"""
    k = line.find(b"\0")
    return b"" if k < 0 else line[k:]
