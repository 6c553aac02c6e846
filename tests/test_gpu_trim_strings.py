"""Trimmed strings on the GPU (include/trre_mi355x.h: trre_trim_device_strings; Program.trim_strings / trim_ranges / trim_list)
against the oracle: every string without the match at its start and the match at its end.  Every expectation is the oracle's
spans under the wrapped acceptor (tests/span_lib.py) with the rule of tests/trim_lib.py.  Each case goes through
Program.trim_strings and trim_ranges and once through the C ABI with sentinel-filled arrays of exactly the room asked for — the
bytes behind d_out[out_len], the words behind d_out_off[nrec], d_begin[nrec - 1] and d_end[nrec - 1] stay as they were.  On top of
the oracle, never instead of it: d_out is the gather of d_in by the device's own (begin, end)."""
import ctypes
import random

import pytest

import field_lib
import filter_lib
import span_lib
import split_lib
import trim_lib
import trre_amd
from gpu_column_lib import (BFILL, FILL, PAD, assert_prefix, assert_untouched, blob, carve, dev, lst, off_dev, pack, sequence, soup, to_dev,
                            words)
from span_lib import LAYOUTS, PAIRS, Spanner
from test_gpu_filter_strings import POOL          # the filter tests' pool, NULs and empties in it
from trim_lib import BOTH, LEFT, RIGHT
from trre_amd import api

pytestmark = pytest.mark.gpu

SIDES = ((LEFT, "left"), (RIGHT, "right"), (BOTH, "both"))


def raw(p, values, n, offsets, nrec, flags, cap, null=False, views=True, out=None, ooff=None, begin=None, end=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *out_len, d_out, d_out_off, d_begin, d_end); d_out lies `out_mis` past
    a 16-byte boundary; null: the size query, without d_out and d_out_off; views=False: without d_begin and d_end"""
    if out is None:
        out = carve(cap, out_mis)
    if ooff is None:
        ooff = words(nrec + 1 + PAD)
    if begin is None:
        begin = words(nrec + PAD)
    if end is None:
        end = words(nrec + PAD)
    m = ctypes.c_size_t(77)
    rc = api.lib().trre_trim_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, flags,
                                            None if null else out.data_ptr(), cap, None if null else ooff.data_ptr(),
                                            begin.data_ptr() if views else None, end.data_ptr() if views else None, ctypes.byref(m), None)
    return rc, m.value, out, ooff, begin, end


def check(p, spans, recs, label, sides=SIDES, mis=0, out_mis=0):
    """for every side: Program.trim_strings, trim_ranges and the C ABI with exact room, with the views and without, against the
    strings' spans; and the cross-check on top"""
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    got = {}
    for flags, side in sides:
        want = trim_lib.expect(recs, spans, flags)
        need = len(want[0])
        out, oo = p.trim_strings(values, offsets, side)
        assert lst(oo) == want[1], (label, side)
        assert blob(out) == want[0], (label, side)
        begin, end = p.trim_ranges(values, offsets, side)
        assert (lst(begin), lst(end)) == (want[2], want[3]), (label, side)
        rc, m, out2, oo2, b2, e2 = raw(p, values, len(data), offsets, nrec, flags, need, out_mis=out_mis)
        assert (rc, m) == (0, need), (label, side, rc, m, api.lib().trre_last_error())
        assert_prefix(out2, want[0], (label, side))
        assert_prefix(oo2, want[1], (label, side))
        assert_prefix(b2, want[2], (label, side))
        assert_prefix(e2, want[3], (label, side))
        # on top: the output is the gather of the input by the device's own ranges
        gb, ge = lst(b2[:nrec]), lst(e2[:nrec])
        assert blob(out2[:need]) == b"".join(data[b:e] for b, e in zip(gb, ge)), (label, side)
        assert all(off[i] <= gb[i] <= ge[i] <= off[i + 1] for i in range(nrec)), (label, side)
        rc, m, out3, oo3, b3, e3 = raw(p, values, len(data), offsets, nrec, flags, need, views=False, out_mis=out_mis)
        assert (rc, m) == (0, need), (label, side, rc, m)
        assert_prefix(out3, want[0], (label, side))
        assert_prefix(oo3, want[1], (label, side))
        assert_untouched(b3, (label, side))
        assert_untouched(e3, (label, side))
        got[flags] = want
    return got


def test_paired_patterns_and_layouts():
    """the pairs and the three symbol layouts on a few hundred random short strings and the pool with NULs and empties, all three
    sides, against the yardstick: a program with output trims as its input projection"""
    rng = random.Random(291)
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"  a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0",
             b"cat\0", b"catdog", b"xxbxx", b"   ", b"dogcat", b" a\0 "]
    extra += [b"abc", b"bacx", b"singing"]
    layouts, changed, total = set(), 0, 0
    for prog, acc in PAIRS + LAYOUTS:
        recs = soup(rng, b"abcdefgh ingxt059", 250) + soup(rng, b"a x1cb", 100, 8) + extra + POOL
        p, spanner = trre_amd.Program(prog, "nft", "spans"), Spanner(acc)
        got = check(p, spanner.lines(recs), recs, prog, mis=rng.randrange(16), out_mis=rng.randrange(16))
        # the yardstick's own entries: every program trims at least the string written for it above and leaves the empty one whole
        entries = [got[BOTH][0][got[BOTH][1][i]:got[BOTH][1][i + 1]] for i in range(len(recs))]
        here = sum(a != b for a, b in zip(entries, recs))
        assert 1 <= here < len(recs), (prog, here)
        changed, total = changed + here, total + len(recs)
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and changed * 20 >= total, (layouts, changed, total)


def test_edges():
    """nrec = 0; one empty string; 70 000 empty strings under 'x*' and ' +'; nrec of 63, 64, 65; d_in misaligned by 1 .. 15 with
    d_out at odd addresses; a left match over tile edges with a right one inside a tile; one string of 20 000 spaces, ab, 20 000
    spaces; NULs"""
    import torch
    rng = random.Random(292)
    star, plus = (trre_amd.Program(q, "nft", "spans") for q in ("x*", " +"))
    xs, ps = Spanner("x*"), Spanner(" +")
    # nrec == 0: d_out_off[0] and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for flags, side in SIDES:
        out, oo = star.trim_strings(empty, zero, side)
        assert out.numel() == 0 and lst(oo) == [0]
        begin, end = star.trim_ranges(empty, zero, side)
        assert lst(begin) == [] and lst(end) == []
        assert star.trim_list([], side) == []
        rc, m, out, oo, b, e = raw(star, empty, 0, zero, 0, flags, 0)
        assert (rc, m) == (0, 0) and lst(oo) == [0] + [FILL] * PAD and bool((out == BFILL).all())
        assert_untouched(b)
        assert_untouched(e)
        rc, m, _, oo, b, e = raw(star, empty, 0, zero, 0, flags, 0, null=True)
        assert (rc, m) == (0, 0)
        for t in (oo, b, e):
            assert_untouched(t)
    # one empty string: no match under ' +', the one empty match under 'x*'
    for p, sp in ((plus, ps), (star, xs)):
        got = check(p, [sp(b"")], [b""], "one empty")
        assert all(got[f] == (b"", [0, 0], [0], [0]) for f in (LEFT, RIGHT, BOTH))
    # no entry has bytes with nrec > 0 and the null size query: TRRE_OK, the ranges written
    rc, m, _, oo, b, e = raw(plus, to_dev(b"   "), 3, off_dev([0, 3]), 1, BOTH, 0, null=True)
    assert (rc, m) == (0, 0) and lst(b) == [3] + [FILL] * PAD and lst(e) == [3] + [FILL] * PAD
    assert_untouched(oo)
    # 70 000 empty strings: one tile of the input
    many = [b""] * 70000
    for p, sp in ((star, xs), (plus, ps)):
        got = check(p, [sp(b"")] * 70000, many, "70 000 empty", sides=((BOTH, "both"),))
        assert got[BOTH] == (b"", [0] * 70001, [0] * 70000, [0] * 70000)
    # the left match crosses tile edges, the right one does not
    long = [b"b", b" " * 40000 + b"a" + b" " * 7, b" a"]
    got = check(plus, ps.lines(long), long, "40 000 spaces")
    assert got[BOTH] == (b"baa", [0, 1, 2, 3], [0, 40001, 40010], [1, 40002, 40011])
    assert got[LEFT][0] == b"ba" + b" " * 7 + b"a" and got[RIGHT][0] == b"b" + b" " * 40000 + b"a a"
    # one string over three tiles, trimmed by more than a tile on each side
    inner = [b" " * 20000 + b"ab" + b" " * 20000]
    got = check(plus, ps.lines(inner), inner, "ab of 40 002", mis=5, out_mis=3)
    assert got[BOTH] == (b"ab", [0, 2], [20000], [20002]) and got[LEFT][1] == [0, 20002] and got[RIGHT][1] == [0, 20002]
    # NULs: never trimmed on the right, trimmed on the left, the NUL and what follows kept
    nuls = [b" a\0 ", b"\0 ", b" \0", b"", b"  a  b  ", b"   ", b" \0 a "]
    got = check(plus, ps.lines(nuls), nuls, "nuls")
    assert plus.trim_list(nuls) == [b"a\0 ", b"\0 ", b"\0", b"", b"a  b", b"", b"\0 a "]
    assert plus.trim_list(nuls, "right") == [b" a\0 ", b"\0 ", b" \0", b"", b"  a  b", b"", b" \0 a "]
    assert plus.trim_list(nuls, side="left") == [b"a\0 ", b"\0 ", b"\0", b"", b"a  b  ", b"", b"\0 a "]
    # x* by hand: two matches end at the string's end, the min decides
    assert star.trim_list([b"xxbxx", b"bxx", b"xx", b"xxb\0xx", b"", b"b"]) == [b"b", b"b", b"", b"b\0xx", b"", b"b"]
    cats, spanner = trre_amd.Program("(cat|dog)", "nft", "spans"), Spanner("(cat|dog)")
    assert cats.trim_list([b"catxdog", b"xcat", b"catx", b"dogcat"]) == [b"x", b"x", b"x", b""]
    assert trre_amd.Program("[0-9]+", "nft", "spans").trim_list([b"12ab34"]) == [b"ab"]
    # nrec around a wave; d_in at every misalignment, d_out at odd addresses
    for nrec in (63, 64, 65):
        recs = [rng.choice(POOL + [b"catxdog", b"dogcat", b"xcat"]) for _ in range(nrec)]
        check(cats, spanner.lines(recs), recs, ("nrec", nrec))
    recs = [rng.choice(POOL + [b"catxdog", b"dogcat", b"xcat", b"catx"]) for _ in range(200)]
    spans = spanner.lines(recs)
    for mis in range(1, 16):
        check(cats, spans, recs, ("mis", mis), sides=(SIDES[mis % 3],), mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])


def test_capacity_and_sizes():
    """the null size query, cap = 0 and cap = out_len - 1: TRRE_E_CAPACITY, *out_len and the ranges right, d_out and d_out_off all
    sentinel; exact room succeeds"""
    rng = random.Random(293)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    recs = [bytes(rng.choice(b"0123456789xy ") for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
    spans = spanner.lines(recs)
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data), off_dev(off)
    for flags, side in SIDES:
        want = trim_lib.expect(recs, spans, flags)
        need = len(want[0])
        assert 0 < need < len(data) and sum(b != o for b, o in zip(want[2], off)) >= (300 if flags & LEFT else 0), (side, need)

        def refused(rc, m, out, oo, b, e):
            assert (rc, m) == (api.E_CAPACITY, need), (side, rc, m)
            assert_untouched(out, side)
            assert_untouched(oo, side)
            assert_prefix(b, want[2], side)
            assert_prefix(e, want[3], side)

        refused(*raw(p, values, len(data), offsets, nrec, flags, 0, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, flags, 0))
        refused(*raw(p, values, len(data), offsets, nrec, flags, need - 1))
        rc, m, out, oo, b, e = raw(p, values, len(data), offsets, nrec, flags, need)
        assert (rc, m) == (0, need), (side, rc, m)
        assert_prefix(out, want[0], side)
        assert_prefix(oo, want[1], side)
        assert_prefix(b, want[2], side)
        assert_prefix(e, want[3], side)


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, flags=BOTH, **kw):
        rc, m, out, oo, b, e = raw(p, vals, len(data), offs, 4, flags, cap, **kw)
        assert rc == rc_want and m == 0, (rc, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("ooff", oo), ("begin", b), ("end", e)):
            if name not in kw:
                assert_untouched(t, name)
        assert lst(offsets) == off and blob(values) == data

    for mode in ("scan", "match", "find"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    for flags in (0, 4, 7):
        untouched(api.E_ARG, p, flags=flags)
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        for flags in (LEFT, BOTH):
            untouched(api.E_ARG, p, offs=off_dev(bad), flags=flags)                              # bad offsets: nothing written
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, ooff=as_words(values[:40]))                                          # d_in / d_out_off
    untouched(api.E_ARG, p, begin=as_words(values[560:600]))                                     # d_in / d_begin
    untouched(api.E_ARG, p, end=offsets)                                                         # d_off / d_end
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, ooff=shared[64:])             # d_out / d_out_off
    untouched(api.E_ARG, p, begin=shared, end=shared[3:])                                        # d_begin / d_end
    untouched(api.E_ARG, p, ooff=shared, end=shared[4:])                                         # d_out_off / d_end
    assert bool((shared == FILL).all())
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, m, out, oo, b, e = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, BOTH, 700)
        assert rc == api.E_ARG and m == 0 and "newline" in api.lib().trre_last_error().decode()
        for t in (out, oo, b, e):
            assert_untouched(t, at)
    # ... and the same strings go through: [12 x 50], [], [12 x 250], [ab]: a string of digits is one match
    rc, m, out, oo, b, e = raw(p, values, len(data), offsets, 4, BOTH, 700)
    assert (rc, m) == (0, 2) and lst(oo[:5]) == [0, 0, 0, 0, 2] and blob(out[:2]) == b"ab"
    assert lst(b[:4]) == [100, 100, 600, 600] and lst(e[:4]) == [100, 100, 600, 602]
    assert bool((out[2:] == BFILL).all()) and bool((oo[5:] == FILL).all()) and bool((b[4:] == FILL).all()) and bool((e[4:] == FILL).all())


def test_interleaved_with_the_other_span_calls_on_one_program():
    """trim_strings, field_strings, filter_strings, split_strings, span_strings and trim_strings again, back to back on ONE
    program, over gpu_column_lib.sequence's sizes.  The buffers the calls share only grow and every pass carves them anew: every
    result stays right"""
    seq = sequence(295, b"1a2", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)), framed=False)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    for label in ("tiny", "large", "none", "one tile", "one tile and a byte", "large again"):
        recs = seq[label]
        spans = spanner.lines(recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        want_spans = span_lib.expect(spans, off)
        want_split = split_lib.expect([split_lib.cut_pieces(l, sp) for l, sp in zip(recs, spans)])
        want_filter = filter_lib.expect(recs, spans)
        for (f1, s1), (f2, s2), k in ((SIDES[2], SIDES[0], 1), (SIDES[1], SIDES[2], 0)):
            out, oo = p.trim_strings(values, offsets, s1)
            assert (blob(out), lst(oo)) == trim_lib.expect(recs, spans, f1)[:2], (label, s1)
            out, oo, valid = p.field_strings(values, offsets, k)
            assert (blob(out), lst(oo), lst(valid)) == field_lib.expect(recs, spans, k), (label, k)
            out, oo, rows = p.filter_strings(values, offsets)
            assert (blob(out), lst(oo), lst(rows)) == want_filter, label
            out, po, lo = p.split_strings(values, offsets)
            assert (blob(out), lst(po), lst(lo)) == want_split, label
            st, en, lo = p.span_strings(values, offsets)
            assert (lst(st), lst(en), lst(lo)) == want_spans, label
            begin, end = p.trim_ranges(values, offsets, s2)
            out, oo = p.trim_strings(values, offsets, s2)
            assert (blob(out), lst(oo), lst(begin), lst(end)) == trim_lib.expect(recs, spans, f2), (label, s2)
