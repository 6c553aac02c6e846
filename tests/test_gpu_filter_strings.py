"""Filtered strings on the GPU (include/trre_mi355x.h: trre_filter_device_strings; Program.filter_strings / filter_list) against
the oracle: the strings with a match kept whole, the rest dropped, and the rows that were kept.  Every expectation is the oracle's
spans under the wrapped acceptor (tests/span_lib.py), turned into the three arrays in Python (tests/filter_lib.py).  Each case goes
once through Program.filter_strings and once through the C ABI with sentinel-filled arrays of exactly the size asked for — the
bytes behind d_out[out_len] and the words behind d_out_off[n_kept] and d_rows[n_kept - 1] stay as they were — plain and inverted."""
import ctypes
import random

import pytest

import filter_lib
import span_lib
import split_lib
import trre_amd
from gpu_column_lib import BFILL, FILL, PAD, assert_prefix, assert_untouched, blob, carve, dev, lst, off_dev, pack, sequence, soup, to_dev, words
from span_lib import LAYOUTS, PAIRS, Spanner
from trre_amd import api

pytestmark = pytest.mark.gpu

POOL = [b"", b"cat", b"a cat and a dog", b"xyz", b"\0 cat", b"do\0g cat", b"catdogcat", b"c" * 40]


def raw(p, values, n, offsets, nrec, cap, rcap, invert=False, null=False, out=None, ooff=None, rows=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_kept, *out_len, d_out, d_out_off, d_rows); d_out lies `out_mis` past
    a 16-byte boundary"""
    if out is None:
        out = carve(cap, out_mis)
    if ooff is None:
        ooff = words(rcap + 1 + PAD)
    if rows is None:
        rows = words(rcap + PAD)
    k, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_filter_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, api.FILTER_INVERT if invert else 0,
                                              None if null else out.data_ptr(), cap, None if null else ooff.data_ptr(),
                                              None if null else rows.data_ptr(), rcap, ctypes.byref(k), ctypes.byref(m), None)
    return rc, k.value, m.value, out, ooff, rows


def check(p, spans, recs, label, mis=0, out_mis=0):
    """plain and inverted: one call through Program.filter_strings and one through the C ABI with exact room, against the
    strings' spans; rows against count_strings.  Returns the plain expectation"""
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    counts = lst(p.count_strings(values, offsets)) if nrec else []
    assert counts == [len(w) for w in spans], label
    wants = []
    for invert in (False, True):
        want = filter_lib.expect(recs, spans, invert)
        wants.append(want)
        need, kept = len(want[0]), len(want[2])
        assert want[2] == [i for i, c in enumerate(counts) if (c > 0) != invert], (label, invert)
        out, oo, rows = p.filter_strings(values, offsets, invert=invert)
        assert lst(rows) == want[2], (label, invert)
        assert lst(oo) == want[1], (label, invert)
        assert blob(out) == want[0], (label, invert)
        rc, k, m, out2, oo2, rows2 = raw(p, values, len(data), offsets, nrec, need, kept, invert=invert, out_mis=out_mis)
        assert (rc, k, m) == (0, kept, need), (label, invert, rc, k, m, api.lib().trre_last_error())
        for t, w in zip((out2, oo2, rows2), want):
            assert_prefix(t, w, (label, invert))
    assert sorted(wants[0][2] + wants[1][2]) == list(range(nrec)), label
    return wants[0]


def test_golden_and_paired_patterns():
    """golden acceptor vectors (first 2 000 lines), the pairs and the three symbol layouts against the yardstick; no case skipped"""
    rng = random.Random(91)
    golden = span_lib.golden_acceptors()
    assert len(golden) >= 18, len(golden)
    cases = [(pat, pat, name, lines[:2000]) for pat, vs in golden.items() for name, lines in vs]
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
    for prog, acc in PAIRS + LAYOUTS:
        cases.append((prog, acc, "pair", soup(rng, b"abcdefgh ingxt059", 300) + extra))
    progs, layouts, n_kept, n_dropped = {}, set(), 0, 0
    for prog, acc, name, recs in cases:
        if prog not in progs:
            progs[prog] = (trre_amd.Program(prog, "nft", "spans"), Spanner(acc))
        p, spanner = progs[prog]
        want = check(p, spanner.lines(recs), recs, (prog, name), mis=rng.randrange(16), out_mis=rng.randrange(16))
        n_kept += len(want[2])
        n_dropped += len(recs) - len(want[2])
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and n_kept > 2000 and n_dropped > 2000, (layouts, n_kept, n_dropped)


def test_edges():
    """nrec = 0; one empty string, kept and dropped; 70 000 empty strings under 'x*' (all kept, no byte) and under 'a+' (none
    kept); 'a+' and inverted 'b+' on ['', 40 000 a, 'ba']; a dropped 40 000-byte string between two kept bytes; a NUL ends the
    search and the copy keeps it; nrec of 63, 64, 65; d_in misaligned by 1 .. 15 with d_out at odd addresses; ',' by hand"""
    import torch
    rng = random.Random(92)
    star, plus = trre_amd.Program("x*", "nft", "spans"), trre_amd.Program("a+", "nft", "spans")
    xs, ap = Spanner("x*"), Spanner("a+")
    # nrec == 0: d_out_off[0] and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for invert in (False, True):
        out, oo, rows = star.filter_strings(empty, zero, invert=invert)
        assert out.numel() == 0 and lst(oo) == [0] and lst(rows) == []
        assert star.filter_list([], invert=invert) == ([], [])
        rc, k, m, out, oo, rows = raw(star, empty, 0, zero, 0, 0, 0, invert=invert)
        assert (rc, k, m) == (0, 0, 0) and lst(oo) == [0] + [FILL] * PAD and lst(rows) == [FILL] * PAD and bool((out == BFILL).all())
        rc, k, m, _, _, _ = raw(star, empty, 0, zero, 0, 0, 0, invert=invert, null=True)
        assert (rc, k, m) == (0, 0, 0)
    # one empty string: kept under a pattern that matches it, dropped under one that does not (and the reverse, inverted)
    assert check(star, [xs(b"")], [b""], "one empty, kept") == (b"", [0, 0], [0])
    assert check(plus, [ap(b"")], [b""], "one empty, dropped") == (b"", [0], [])
    # nothing kept with nrec > 0 and the null size query: TRRE_OK, both sizes 0
    rc, k, m, _, _, _ = raw(plus, empty, 0, off_dev([0, 0]), 1, 0, 0, null=True)
    assert (rc, k, m) == (0, 0, 0)
    # 70 000 empty strings: one tile of the input, every row
    many = [b""] * 70000
    assert check(star, [xs(b"")] * 70000, many, "70 000 empty, x*") == (b"", [0] * 70001, list(range(70000)))
    assert check(plus, [ap(b"")] * 70000, many, "70 000 empty, a+") == (b"", [0], [])
    # one string across three tiles, kept and dropped
    long = [b"", b"a" * 40000, b"ba"]
    assert check(plus, ap.lines(long), long, "40 000 a") == (b"a" * 40000 + b"ba", [0, 40000, 40002], [1, 2])
    bp = Spanner("b+")
    want = filter_lib.expect(long, bp.lines(long), invert=True)
    assert want == (b"a" * 40000, [0, 0, 40000], [0, 1])
    check(trre_amd.Program("b+", "nft", "spans"), bp.lines(long), long, "b+ on 40 000 a")
    between = [b"a", b"b" * 40000, b"a"]
    assert check(plus, ap.lines(between), between, "dropped 40 000") == (b"aa", [0, 1, 2], [0, 2])
    # a NUL ends the search; a kept string is copied whole
    cats, spanner = trre_amd.Program("(cat|dog)", "nft", "spans"), Spanner("(cat|dog)")
    nuls = [b"\0cat dog", b"a cat\0dog", b"cat dog\0", b"\0", b"cat", b"dog\0\0cat"]
    want = check(cats, spanner.lines(nuls), nuls, "nuls")
    assert want[2] == [1, 2, 4, 5] and want[0] == b"a cat\0dogcat dog\0catdog\0\0cat"
    assert cats.filter_list(nuls) == ([nuls[1], nuls[2], nuls[4], nuls[5]], [1, 2, 4, 5])
    assert cats.filter_list(nuls, invert=True) == ([nuls[0], nuls[3]], [0, 3])
    # nrec around a wave; d_in at every misalignment, d_out at odd addresses
    for nrec in (63, 64, 65):
        recs = [rng.choice(POOL) for _ in range(nrec)]
        check(cats, spanner.lines(recs), recs, ("nrec", nrec))
    rng94 = random.Random(94)
    recs = [rng94.choice(POOL) for _ in range(200)]
    spans = spanner.lines(recs)
    kept = sum(1 for w in spans if w)
    assert kept >= 20 and 200 - kept >= 20, kept
    for mis in range(1, 16):
        check(cats, spans, recs, ("mis", mis), mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])
    # by hand
    comma = trre_amd.Program(",", "nft", "spans")
    hand = [b"a,b,,c", b"", b",", b"no comma"]
    assert comma.filter_list(hand) == ([b"a,b,,c", b","], [0, 2])
    assert comma.filter_list(hand, invert=True) == ([b"", b"no comma"], [1, 3])
    assert check(comma, Spanner(",").lines(hand), hand, "by hand") == (b"a,b,,c,", [0, 6, 7], [0, 2])


def test_capacity_and_sizes():
    """the null size query, cap = out_len - 1 with room for the rows, row_cap = n_kept - 1 with room for the bytes:
    TRRE_E_CAPACITY, both sizes right, all three arrays all sentinel; exact room succeeds"""
    rng = random.Random(93)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    recs = [bytes(rng.choice(b"0123456789xy ") for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
    spans = spanner.lines(recs)
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data), off_dev(off)
    for invert in (False, True):
        want = filter_lib.expect(recs, spans, invert)
        need, kept = len(want[0]), len(want[2])
        assert kept >= 300 and nrec - kept >= 300 and need > 0, (invert, kept)

        def refused(rc, k, m, out, oo, rows):
            assert (rc, k, m) == (api.E_CAPACITY, kept, need), (invert, rc, k, m)
            for t in (out, oo, rows):
                assert_untouched(t, invert)

        refused(*raw(p, values, len(data), offsets, nrec, 0, 0, invert=invert, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, need - 1, kept, invert=invert))
        refused(*raw(p, values, len(data), offsets, nrec, need, kept - 1, invert=invert))
        refused(*raw(p, values, len(data), offsets, nrec, need + 100, 0, invert=invert))
        rc, k, m, out, oo, rows = raw(p, values, len(data), offsets, nrec, need, kept, invert=invert)
        assert (rc, k, m) == (0, kept, need), (invert, rc, k, m)
        for t, w in zip((out, oo, rows), want):
            assert_prefix(t, w, invert)


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, rcap=64, **kw):
        rc, k, m, out, oo, rows = raw(p, vals, len(data), offs, 4, cap, rcap, **kw)
        assert rc == rc_want and (k, m) == (0, 0), (rc, k, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("ooff", oo), ("rows", rows)):
            if name not in kw:
                assert_untouched(t, name)
        assert lst(offsets) == off and blob(values) == data

    for mode in ("scan", "match", "find"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        untouched(api.E_ARG, p, offs=off_dev(bad))                                               # bad offsets: nothing written
        untouched(api.E_ARG, p, offs=off_dev(bad), invert=True)
    # every pairwise overlap of the five arrays
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, out=values[601:], cap=1)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, ooff=as_words(values[:520]))                                         # d_in / d_out_off
    untouched(api.E_ARG, p, rows=as_words(values[:512]))                                         # d_in / d_rows
    untouched(api.E_ARG, p, out=offsets.view(torch.uint8), cap=40)                               # d_off / d_out
    untouched(api.E_ARG, p, ooff=offsets, rcap=4)                                                # d_off / d_out_off
    untouched(api.E_ARG, p, rows=offsets, rcap=5)                                                # d_off / d_rows
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, ooff=shared[64:], rcap=8)     # d_out / d_out_off
    untouched(api.E_ARG, p, out=shared.view(torch.uint8)[512:], cap=64, rows=shared[60:], rcap=8)     # d_out / d_rows
    untouched(api.E_ARG, p, ooff=shared, rows=shared[8:], rcap=8)                                # d_out_off / d_rows
    assert bool((shared == FILL).all())
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, k, m, out, oo, rows = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, 700, 64)
        assert rc == api.E_ARG and (k, m) == (0, 0) and "newline" in api.lib().trre_last_error().decode()
        for t in (out, oo, rows):
            assert_untouched(t, at)
    # ... and the same strings go through: [12 x 50], [], [12 x 250], [ab]
    rc, k, m, out, oo, rows = raw(p, values, len(data), offsets, 4, 700, 64)
    assert (rc, k, m) == (0, 2, 600) and lst(oo[:3]) == [0, 100, 600] and lst(rows[:2]) == [0, 2]
    assert blob(out[:600]) == data[:600] and bool((out[600:] == BFILL).all()) and bool((oo[3:] == FILL).all()) and bool((rows[2:] == FILL).all())
    rc, k, m, out, oo, rows = raw(p, values, len(data), offsets, 4, 700, 64, invert=True)
    assert (rc, k, m) == (0, 2, 2) and lst(oo[:3]) == [0, 0, 2] and lst(rows[:2]) == [1, 3] and blob(out[:2]) == b"ab"
    assert bool((out[2:] == BFILL).all()) and bool((oo[3:] == FILL).all()) and bool((rows[2:] == FILL).all())


def test_interleaved_with_the_span_and_split_calls_on_one_program():
    """span_strings, filter_strings, split_strings, filter_strings(invert=True), count_strings back to back on ONE program: a
    330 KiB input, a tiny one, none, an input of exactly one tile and of one tile and a byte, the large one again.  The buffers the
    calls share only grow and every pass carves them anew: every result stays right"""
    seq = sequence(95, b"a1b", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)), framed=False)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    for label in ("large", "tiny", "none", "one tile", "one tile and a byte", "large again"):
        recs = seq[label]
        spans = spanner.lines(recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        want_spans = span_lib.expect(spans, off)
        want_split = split_lib.expect([split_lib.cut_pieces(l, sp) for l, sp in zip(recs, spans)])
        want, want_inv = filter_lib.expect(recs, spans), filter_lib.expect(recs, spans, invert=True)
        for step in range(2):
            st, en, lo = p.span_strings(values, offsets)
            assert (lst(st), lst(en), lst(lo)) == want_spans, (label, step)
            out, oo, rows = p.filter_strings(values, offsets)
            assert (blob(out), lst(oo), lst(rows)) == want, (label, step)
            out, po, lo = p.split_strings(values, offsets)
            assert (blob(out), lst(po), lst(lo)) == want_split, (label, step)
            out, oo, rows = p.filter_strings(values, offsets, invert=True)
            assert (blob(out), lst(oo), lst(rows)) == want_inv, (label, step)
            assert lst(p.count_strings(values, offsets)) == [len(w) for w in spans], (label, step)
