"""Split strings on the GPU (include/trre_mi355x.h: trre_split_device_strings; Program.split_strings / split_list) against the
oracle: every string cut at every match, a list of pieces per string.  Every expectation is the oracle's spans under the wrapped
acceptor (tests/span_lib.py), the pieces cut in Python from the uncut string (tests/split_lib.py).  Each case goes once through
Program.split_strings and once through the C ABI with sentinel-filled arrays of exactly the size asked for: the bytes behind
d_out[out_len] and the words behind d_piece_off[n_pieces] and d_list_off[nrec] stay as they were."""
import ctypes
import random

import pytest

import find_lib
import span_lib
import split_lib
import trre_amd
from find_lib import Finder, lines_of
from gpu_column_lib import BFILL, FILL, PAD, assert_prefix, assert_untouched, blob, carve, dev, lst, off_dev, pack, sequence, soup, to_dev, words
from span_lib import LAYOUTS, PAIRS, Spanner, Weak
from split_lib import cut_pieces, split_lines
from trre_amd import api

pytestmark = pytest.mark.gpu



def raw(p, values, n, offsets, nrec, cap, pcap, null=False, out=None, poff=None, loff=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_pieces, *out_len, d_out, d_piece_off, d_list_off); d_out lies
    `out_mis` past a 16-byte boundary"""
    if out is None:
        out = carve(cap, out_mis)
    if poff is None:
        poff = words(pcap + 1 + PAD)
    if loff is None:
        loff = words(nrec + 1 + PAD)
    k, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_split_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, None if null else out.data_ptr(), cap,
                                             None if null else poff.data_ptr(), pcap, loff.data_ptr(), ctypes.byref(k), ctypes.byref(m), None)
    return rc, k.value, m.value, out, poff, loff


def check(p, per, recs, label, mis=0, out_mis=0):
    """one call through Program.split_strings and one through the C ABI with exact room, against the per-string pieces `per`"""
    data, off = pack(recs)
    want = split_lib.expect(per)
    need, pieces, nrec = len(want[0]), len(want[1]) - 1, len(recs)
    assert pieces == want[2][-1] and sum(map(len, recs)) >= need
    values, offsets = to_dev(data, mis), off_dev(off)
    out, po, lo = p.split_strings(values, offsets)
    assert lst(lo) == want[2], label
    assert lst(po) == want[1], label
    assert blob(out) == want[0], label
    rc, k, m, out2, po2, lo2 = raw(p, values, len(data), offsets, nrec, need, pieces, out_mis=out_mis)
    assert (rc, k, m) == (0, pieces, need), (label, rc, k, m, api.lib().trre_last_error())
    for t, w in zip((out2, po2, lo2), want):
        assert_prefix(t, w, label)
    return want


def test_golden_and_paired_patterns():
    """golden acceptor vectors (first 2 000 lines), the pairs and the three symbol layouts against the yardstick; no case skipped"""
    rng = random.Random(81)
    golden = span_lib.golden_acceptors()
    assert len(golden) >= 18, len(golden)
    cases = [(pat, pat, name, lines[:2000]) for pat, vs in golden.items() for name, lines in vs]
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
    for prog, acc in PAIRS + LAYOUTS:
        cases.append((prog, acc, "pair", soup(rng, b"abcdefgh ingxt059", 300) + extra))
    progs, layouts, n_pieces = {}, set(), 0
    for prog, acc, name, recs in cases:
        if prog not in progs:
            progs[prog] = (trre_amd.Program(prog, "nft", "spans"), Spanner(acc))
        p, spanner = progs[prog]
        want = check(p, split_lines(spanner, recs), recs, (prog, name), mis=rng.randrange(16), out_mis=rng.randrange(16))
        n_pieces += want[2][-1]
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and n_pieces > 10000, (layouts, n_pieces)


def test_counts_and_joined_pieces_on_every_usable_golden_vector():
    """transducers included (first 2 000 lines): per string the number of pieces is the length of Finder(P)'s list + 1, the
    pieces joined are the bytes outside A..B of the oracle's output for the wrapped program plus whatever lies behind a NUL.
    Skipped: the vectors the reference does not survive — each gives TRRE_E_DIVERGES with both sizes 0 — and nothing else; a
    pattern beyond the guided tables is refused by the builder, as documented"""
    usable, dead, _, _ = find_lib.vectors()
    progs, compared, refused = {}, 0, 0
    for pat, name, data in usable:
        recs = lines_of(data)[:2000]
        if pat not in progs:
            try:
                progs[pat] = (trre_amd.Program(pat, "nft", "spans"), Finder(pat), Weak(pat))
            except trre_amd.TrreError as e:
                assert e.code == api.E_UNSUPPORTED and "guided tables" in e.message, (pat, e)
                assert trre_amd.Program(pat, "nft").info.guided_rev_states == 0, pat
                progs[pat] = None
        if progs[pat] is None:
            refused += 1
            continue
        p, finder, weak = progs[pat]
        data2, off = pack(recs)
        out, po, lo = p.split_strings(to_dev(data2), off_dev(off))
        got = split_lib.per_string(blob(out), lst(po), lst(lo))
        assert len(got) == len(recs) and lst(po)[-1] == out.numel(), (pat, name)
        counts = [len(w) for w in finder.lines(recs)]
        assert [len(w) - 1 for w in got] == counts, (pat, name)
        for l, pieces, (k, rest) in zip(recs, got, weak.lines(recs)):
            assert len(pieces) == k + 1 and b"".join(pieces) == rest + split_lib.nul_tail(l), (pat, name, l)
        compared += 1
    assert compared + refused == len(usable) and compared > 400 and refused < 10, (compared, refused)
    assert len(dead) == 13
    for pat, name, data in dead:
        recs = lines_of(data)
        data2, off = pack(recs)
        rc, k, m, _, _, _ = raw(trre_amd.Program(pat, "nft", "spans"), to_dev(data2), len(data2), off_dev(off), len(recs), 1 << 16, 1 << 16)
        assert rc == api.E_DIVERGES and (k, m) == (0, 0), (pat, name, rc, k, m)
        assert "stack max capacity" in api.lib().trre_last_error().decode(), (pat, name)


def test_edges():
    """nrec = 0; one empty string; 70 000 empty strings under 'x*' (140 000 empty pieces, nothing kept); 'x*' on one string of
    20 000 b (20 002 pieces); 'a+' on 40 000 a (framed tiles with no marker inside a match); 'b+' on 40 000 a (tiles with no marker
    outside any match, 40 000 bytes copied); a NUL at the first, a middle and the last byte; nrec of 63, 64, 65; d_in misaligned
    by 1 .. 15, d_out at odd addresses; ',' by hand"""
    import torch
    rng = random.Random(82)
    star, plus = trre_amd.Program("x*", "nft", "spans"), trre_amd.Program("a+", "nft", "spans")
    xs, ap = Spanner("x*"), Spanner("a+")
    # nrec == 0: entry 0 of both arrays and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    out, po, lo = star.split_strings(empty, zero)
    assert out.numel() == 0 and po.cpu().tolist() == [0] and lo.cpu().tolist() == [0]
    assert star.split_list([]) == []
    rc, k, m, out, po, lo = raw(star, empty, 0, zero, 0, 0, 0)
    assert (rc, k, m) == (0, 0, 0) and lo.cpu().tolist() == [0] + [FILL] * PAD and po.cpu().tolist() == [0] + [FILL] * PAD
    rc, k, m, _, _, lo = raw(star, empty, 0, zero, 0, 0, 0, null=True)
    assert (rc, k, m) == (0, 0, 0) and lo.cpu().tolist() == [0] + [FILL] * PAD
    # one empty string: one empty piece under a pattern that does not match it, two under one that does
    assert check(plus, split_lines(ap, [b""]), [b""], "one empty, no match") == (b"", [0, 0], [0, 1])
    assert check(star, split_lines(xs, [b""]), [b""], "one empty") == (b"", [0, 0, 0], [0, 2])
    # every framed byte a marker: A B newline, 210 000 of them
    want = check(star, [cut_pieces(b"", xs(b""))] * 70000, [b""] * 70000, "70 000 empty")
    assert want[0] == b"" and len(want[1]) == 140001 and want[2][-1] == 140000
    # A and B adjacent at every piece and tile edge
    want = check(star, split_lines(xs, [b"b" * 20000]), [b"b" * 20000], "20 000 b")
    assert want[2] == [0, 20002] and want[0] == b"b" * 20000 and want[1] == [0] + list(range(20001)) + [20000]
    # one span across three framed tiles: tiles with no marker inside a match
    long = [b"", b"a" * 40000, b"ba"]
    assert check(plus, split_lines(ap, long), long, "40 000 a") == (b"b", [0, 0, 0, 0, 1, 1], [0, 1, 3, 5])
    # no marker at all outside any match: 40 000 bytes copied
    want = check(trre_amd.Program("b+", "nft", "spans"), split_lines(Spanner("b+"), [b"a" * 40000]), [b"a" * 40000], "b+ on 40 000 a")
    assert want == (b"a" * 40000, [0, 40000], [0, 1])
    # a NUL ends the search: the last piece keeps it and everything behind it
    cats, spanner = trre_amd.Program("(cat|dog)", "nft", "spans"), Spanner("(cat|dog)")
    nuls = [b"\0cat dog", b"a cat\0dog", b"cat dog\0", b"\0", b"cat", b"dog\0\0cat"]
    per = split_lines(spanner, nuls)
    assert per[:3] == [[b"\0cat dog"], [b"a ", b"\0dog"], [b"", b" ", b"\0"]]
    check(cats, per, nuls, "nuls")
    assert cats.split_list(nuls) == per
    # nrec around a wave; d_in at every misalignment, d_out at odd addresses
    pool = [b"", b"cat", b"a cat and a dog", b"xyz", b"\0 cat", b"do\0g cat", b"catdogcat", b"c" * 40]
    for nrec in (63, 64, 65):
        recs = [rng.choice(pool) for _ in range(nrec)]
        check(cats, split_lines(spanner, recs), recs, ("nrec", nrec))
    recs = [rng.choice(pool) for _ in range(200)]
    per = split_lines(spanner, recs)
    for mis in range(1, 16):
        check(cats, per, recs, ("mis", mis), mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])
    # by hand
    comma = trre_amd.Program(",", "nft", "spans")
    assert comma.split_list([b"a,b,,c", b"", b","]) == [[b"a", b"b", b"", b"c"], [b""], [b"", b""]]
    check(comma, split_lines(Spanner(","), [b"a,b,,c", b"", b","]), [b"a,b,,c", b"", b","], "by hand")


def test_capacity_and_sizes():
    """cap = out_len - 1 with room for the pieces, piece_cap = n_pieces - 1 with room for the bytes: TRRE_E_CAPACITY, both sizes
    right, d_list_off right, d_out and d_piece_off all sentinel; the null-pointer size query; exact room succeeds"""
    rng = random.Random(83)
    for prog, acc, alpha in (("[0-9]+:N", "[0-9]+", b"0123456789xy "), ("(a|b)+", "(a|b)+", b"aabc"), ("x*", "x*", b"xxy")):
        p, spanner = trre_amd.Program(prog, "nft", "spans"), Spanner(acc)
        recs = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
        want = split_lib.expect(split_lines(spanner, recs))
        data, off = pack(recs)
        need, pieces, nrec = len(want[0]), len(want[1]) - 1, len(recs)
        assert need > 0 and pieces > nrec + nrec // 2, prog
        values, offsets = to_dev(data), off_dev(off)

        def refused(rc, k, m, out, po, lo):
            assert (rc, k, m) == (api.E_CAPACITY, pieces, need), (prog, rc, k, m)
            assert_untouched(out, prog)
            assert_untouched(po, prog)
            assert_prefix(lo, want[2], prog)

        refused(*raw(p, values, len(data), offsets, nrec, 0, 0, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, need - 1, pieces))
        refused(*raw(p, values, len(data), offsets, nrec, need, pieces - 1))
        refused(*raw(p, values, len(data), offsets, nrec, need + 100, 0))
        rc, k, m, out, po, lo = raw(p, values, len(data), offsets, nrec, need, pieces)
        assert (rc, k, m) == (0, pieces, need), (prog, rc, k, m)
        assert_prefix(out, want[0], prog)
        assert_prefix(po, want[1], prog)
    # nothing kept at all: d_out may be null with cap 0 while the piece offsets are filled
    p = trre_amd.Program("[0-9]+", "nft", "spans")
    values, offsets = to_dev(b"123456"), off_dev([0, 2, 2, 6])
    rc, k, m, _, _, lo = raw(p, values, 6, offsets, 3, 0, 0, null=True)
    assert (rc, k, m) == (api.E_CAPACITY, 5, 0) and lo[:4].cpu().tolist() == [0, 2, 3, 5]
    po = words(6 + PAD)
    k, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_split_device_strings(p._h, values.data_ptr(), 6, offsets.data_ptr(), 3, None, 0, po.data_ptr(), 5, lo.data_ptr(), ctypes.byref(k),
                                             ctypes.byref(m), None)
    assert (rc, k.value, m.value) == (0, 5, 0) and po.cpu().tolist() == [0] * 6 + [FILL] * PAD


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, pcap=64, **kw):
        rc, k, m, out, po, lo = raw(p, vals, len(data), offs, 4, cap, pcap, **kw)
        assert rc == rc_want and (k, m) == (0, 0), (rc, k, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("poff", po), ("loff", lo)):
            if name not in kw:
                assert_untouched(t, name)
        assert offsets.cpu().tolist() == off and blob(values) == data

    for mode in ("scan", "match", "find"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        untouched(api.E_ARG, p, offs=off_dev(bad))                                               # bad offsets: nothing written
    # every pairwise overlap of the five arrays
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, out=values[601:], cap=1)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, poff=as_words(values[:520]))                                         # d_in / d_piece_off
    untouched(api.E_ARG, p, loff=as_words(values[560:600]))                                      # d_in / d_list_off
    untouched(api.E_ARG, p, out=offsets.view(torch.uint8), cap=40)                               # d_off / d_out
    untouched(api.E_ARG, p, poff=offsets, pcap=4)                                                # d_off / d_piece_off
    untouched(api.E_ARG, p, loff=offsets)                                                        # d_off / d_list_off
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, poff=shared[64:], pcap=8)     # d_out / d_piece_off
    untouched(api.E_ARG, p, out=shared.view(torch.uint8)[512:], cap=64, loff=shared[60:])        # d_out / d_list_off
    untouched(api.E_ARG, p, poff=shared, loff=shared[64:])                                       # d_piece_off / d_list_off
    assert bool((shared == FILL).all())
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, k, m, out, po, lo = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, 700, 64)
        assert rc == api.E_ARG and (k, m) == (0, 0) and "newline" in api.lib().trre_last_error().decode()
        for t in (out, po, lo):
            assert_untouched(t, at)
    # ... and the same strings go through
    rc, k, m, out, po, lo = raw(p, values, len(data), offsets, 4, 700, 64)
    assert (rc, k, m) == (0, 6, 2) and lo[:5].cpu().tolist() == [0, 2, 3, 5, 6] and po[:7].cpu().tolist() == [0, 0, 0, 0, 0, 0, 2]
    assert blob(out[:2]) == b"ab" and bool((out[2:] == BFILL).all()) and bool((po[7:] == FILL).all()) and bool((lo[5:] == FILL).all())


def test_interleaved_with_the_span_calls_on_one_program():
    """span_strings, split_strings, count_strings, split_strings back to back on ONE program: a large input, a tiny one, none,
    staged texts of exactly one framed-text tile and of one tile and a byte.  The buffers the calls share only grow and every
    pass carves them anew: every result stays right"""
    seq = sequence(84, b"a1b", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)))
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    for label in ("large", "tiny", "none", "one tile", "one tile and a byte", "large again"):
        recs = seq[label]
        spans = spanner.lines(recs)
        per = [cut_pieces(l, sp) for l, sp in zip(recs, spans)]
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        want_spans, want = span_lib.expect(spans, off), split_lib.expect(per)
        for step in range(2):
            st, en, lo = p.span_strings(values, offsets)
            assert (lst(st), lst(en), lst(lo)) == want_spans, (label, step)
            out, po, lo = p.split_strings(values, offsets)
            assert (blob(out), lst(po), lst(lo)) == want, (label, step)
            assert lst(p.count_strings(values, offsets)) == [len(w) for w in spans], (label, step)
            out, po, lo = p.split_strings(values, offsets)
            assert (blob(out), lst(po), lst(lo)) == want, (label, step)
            # the kept bytes are the input minus the matched ones (checked here, not in the call)
            assert out.numel() == len(data) - sum(e - s for w in spans for s, e in w), (label, step)
