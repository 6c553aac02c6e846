"""Match spans on the GPU (include/trre_mi355x.h: trre_span_device_strings; Program.span_strings / span_list / count_strings)
against the oracle: where every match of every string starts and ends.  Every expectation is the oracle's under the wrapped
acceptor (tests/span_lib.py), in the run.  Each case goes once through Program.span_strings and once through the C ABI with
sentinel-filled arrays of exactly the size asked for: the words behind d_start[n_matches], d_end[n_matches] and
d_list_off[nrec] stay as they were."""
import ctypes
import random

import pytest

import find_lib
import span_lib
import trre_amd
from find_lib import Finder, lines_of
from gpu_column_lib import FILL, PAD, assert_prefix, assert_untouched, blob, dev, lst, off_dev, pack, soup, to_dev, words
from span_lib import LAYOUTS, PAIRS, Spanner, Weak
from trre_amd import api

pytestmark = pytest.mark.gpu

def raw(p, values, n, offsets, nrec, span_cap, null_spans=False, starts=None, ends=None, loff=None):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_matches, d_start, d_end, d_list_off)"""
    if starts is None:
        starts = words(span_cap + PAD)
    if ends is None:
        ends = words(span_cap + PAD)
    if loff is None:
        loff = words(nrec + 1 + PAD)
    k = ctypes.c_size_t(77)
    rc = api.lib().trre_span_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec,
                                            None if null_spans else starts.data_ptr(), None if null_spans else ends.data_ptr(), span_cap,
                                            loff.data_ptr(), ctypes.byref(k), None)
    return rc, k.value, starts, ends, loff


def check(p, per, recs, label, mis=0):
    """one call through Program.span_strings and one through the C ABI with exact room, against the per-string spans `per`"""
    data, off = pack(recs)
    want = span_lib.expect(per, off)
    found, nrec = len(want[0]), len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    st, en, lo = p.span_strings(values, offsets)
    assert lst(st) == want[0], label
    assert lst(en) == want[1], label
    assert lst(lo) == want[2], label
    rc, k, st2, en2, lo2 = raw(p, values, len(data), offsets, nrec, found)
    assert (rc, k) == (0, found), (label, rc, k, api.lib().trre_last_error())
    for t, w in zip((st2, en2, lo2), want):
        assert_prefix(t, w, label)
    return want


def test_golden_and_paired_patterns():
    """golden acceptor vectors (first 2 000 lines), the pairs and the three symbol layouts against the yardstick; no case skipped"""
    rng = random.Random(71)
    golden = span_lib.golden_acceptors()
    assert len(golden) >= 18, len(golden)
    cases = [(pat, pat, name, lines[:2000]) for pat, vs in golden.items() for name, lines in vs]
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
    for prog, acc in PAIRS + LAYOUTS:
        cases.append((prog, acc, "pair", soup(rng, b"abcdefgh ingxt059", 300) + extra))
    progs, layouts, n_matches = {}, set(), 0
    for prog, acc, name, recs in cases:
        if prog not in progs:
            progs[prog] = (trre_amd.Program(prog, "nft", "spans"), Spanner(acc))
        p, spanner = progs[prog]
        assert p.info.kernel == trre_amd.KERNEL_GUIDED_GEN
        want = check(p, spanner.lines(recs), recs, (prog, name), mis=rng.randrange(16))
        n_matches += len(want[0])
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and n_matches > 10000, (layouts, n_matches)


def test_counts_and_gaps_on_every_usable_golden_vector():
    """transducers included (first 2 000 lines): per string the number of spans is the length of Finder(P)'s list (count_strings
    too), the bytes outside the spans are the bytes outside A..B of the oracle's output for the wrapped program.  Skipped: the
    vectors the reference does not survive — each gives TRRE_E_DIVERGES with n_matches = 0 — and nothing else; a pattern beyond
    the guided tables is refused by the builder, as documented"""
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
        text, off = pack(recs)
        values, offsets = to_dev(text), off_dev(off)
        st, en, lo = p.span_strings(values, offsets)
        got = span_lib.relative(lst(st), lst(en), lst(lo), off)
        counts = [len(w) for w in finder.lines(recs)]
        assert [len(w) for w in got] == counts, (pat, name)
        assert lst(p.count_strings(values, offsets)) == counts, (pat, name)
        for l, sp, (k, rest) in zip(recs, got, weak.lines(recs)):
            assert len(sp) == k and span_lib.gaps(l, sp) == rest, (pat, name, l)
            assert all(0 <= s <= e <= len(l) for s, e in sp), (pat, name, l, sp)
        compared += 1
    assert compared + refused == len(usable) and compared > 400 and refused < 10, (compared, refused)
    assert len(dead) == 13
    for pat, name, data in dead:
        recs = lines_of(data)
        text, off = pack(recs)
        rc, k, _, _, _ = raw(trre_amd.Program(pat, "nft", "spans"), to_dev(text), len(text), off_dev(off), len(recs), 1 << 16)
        assert rc == api.E_DIVERGES and k == 0, (pat, name, rc, k)
        assert "stack max capacity" in api.lib().trre_last_error().decode(), (pat, name)


def test_edges():
    """nrec = 0; one empty string; 70 000 empty strings under 'x*' (framed A B newline across tiles); 'x*' on one string of
    20 000 b (A and B adjacent at every piece and tile edge); 'a+' on 40 000 a (one span across tiles); a NUL at the first, a
    middle and the last byte; nrec of 63, 64, 65; d_in misaligned by 1 .. 15"""
    import torch
    rng = random.Random(72)
    star, plus = trre_amd.Program("x*", "nft", "spans"), trre_amd.Program("a+", "nft", "spans")
    # nrec == 0: d_list_off[0] = 0 and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    st, en, lo = star.span_strings(empty, zero)
    assert st.numel() == 0 and en.numel() == 0 and lo.cpu().tolist() == [0]
    assert star.span_list([]) == [] and star.count_strings(empty, zero).numel() == 0
    rc, k, st, en, lo = raw(star, empty, 0, zero, 0, 0, null_spans=True)
    assert (rc, k) == (0, 0) and lo.cpu().tolist() == [0] + [FILL] * PAD
    # one empty string
    xs, ap = Spanner("x*"), Spanner("a+")
    assert check(star, xs.lines([b""]), [b""], "one empty") == ([0], [0], [0, 1])
    # every framed byte a marker: A B newline, 210 000 of them
    want = check(star, xs.lines([b""] * 70000), [b""] * 70000, "70 000 empty")
    assert want[2][-1] == 70000 and set(want[0]) == {0}
    # A and B adjacent at every piece and tile edge: 20 001 empty matches, framed 60 003 bytes
    want = check(star, xs.lines([b"b" * 20000]), [b"b" * 20000], "20 000 b")
    assert want[2] == [0, 20001] and want[0] == want[1] == list(range(20001))
    # one span across three framed tiles
    long = [b"", b"a" * 40000, b"ba"]
    assert check(plus, ap.lines(long), long, "40 000 a") == ([0, 40001], [40000, 40002], [0, 0, 1, 2])
    # a NUL ends the search: at the first, a middle and the last byte
    cats, spanner = trre_amd.Program("(cat|dog)", "nft", "spans"), Spanner("(cat|dog)")
    nuls = [b"\0cat dog", b"a cat\0dog", b"cat dog\0", b"\0", b"cat", b"dog\0\0cat"]
    assert spanner(b"a cat\0dog") == [(2, 5)] and spanner(b"\0cat dog") == [] and spanner(b"cat dog\0") == [(0, 3), (4, 7)]
    check(cats, spanner.lines(nuls), nuls, "nuls")
    assert cats.span_list(nuls) == spanner.lines(nuls)
    # nrec around a wave; d_in at every misalignment
    pool = [b"", b"cat", b"a cat and a dog", b"xyz", b"\0 cat", b"do\0g cat", b"catdogcat", b"c" * 40]
    for nrec in (63, 64, 65):
        recs = [rng.choice(pool) for _ in range(nrec)]
        check(cats, spanner.lines(recs), recs, ("nrec", nrec))
    recs = [rng.choice(pool) for _ in range(200)]
    per = spanner.lines(recs)
    for mis in range(1, 16):
        check(cats, per, recs, ("mis", mis), mis=mis)


def test_capacity_and_sizes():
    """span_cap = n_matches - 1: TRRE_E_CAPACITY, *n_matches right, d_list_off right, d_start and d_end all sentinel; the
    null-pointer size query; count_strings is the oracle's counts; exact room succeeds"""
    rng = random.Random(73)
    for prog, acc, alpha in (("[0-9]+:N", "[0-9]+", b"0123456789xy "), ("(a|b)+", "(a|b)+", b"aabc"), ("x*", "x*", b"xxy")):
        p, spanner = trre_amd.Program(prog, "nft", "spans"), Spanner(acc)
        recs = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
        per = spanner.lines(recs)
        data, off = pack(recs)
        want = span_lib.expect(per, off)
        found, nrec = len(want[0]), len(recs)
        assert found > nrec // 2, prog
        values, offsets = to_dev(data), off_dev(off)
        rc, k, _, _, lo = raw(p, values, len(data), offsets, nrec, 0, null_spans=True)
        assert (rc, k) == (api.E_CAPACITY, found), (prog, rc, k)
        assert_prefix(lo, want[2], prog)
        rc, k, st, en, lo = raw(p, values, len(data), offsets, nrec, found - 1)
        assert (rc, k) == (api.E_CAPACITY, found), (prog, rc, k)
        assert_untouched(st, prog)
        assert_untouched(en, prog)
        assert_prefix(lo, want[2], prog)
        assert lst(p.count_strings(values, offsets)) == [len(w) for w in per], prog
        rc, k, st, en, lo = raw(p, values, len(data), offsets, nrec, found)
        assert (rc, k) == (0, found), (prog, rc, k)
        assert_prefix(st, want[0], prog)
        assert_prefix(en, want[1], prog)
    # no match at all: the size query itself succeeds
    p = trre_amd.Program("[0-9]+", "nft", "spans")
    values, offsets = to_dev(b"abcdef"), off_dev([0, 2, 2, 6])
    rc, k, _, _, lo = raw(p, values, 6, offsets, 3, 0, null_spans=True)
    assert (rc, k) == (0, 0) and lo[:4].cpu().tolist() == [0, 0, 0, 0]


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, **kw):
        rc, k, st, en, lo = raw(p, vals, len(data), offs, 4, 64, **kw)
        assert rc == rc_want and k == 0, (rc, k, api.lib().trre_last_error())
        for name, t in (("starts", st), ("ends", en), ("loff", lo)):
            if name not in kw:
                assert_untouched(t, name)

    for mode in ("scan", "match", "find"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    with pytest.raises(trre_amd.TrreError) as e:
        trre_amd.Program("[0-9]+:N", "dft", "spans")                                             # the DFT engine: refused at compile
    assert e.value.code == api.E_UNSUPPORTED
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        untouched(api.E_ARG, p, offs=off_dev(bad))                                               # bad offsets: nothing written
    shared = words(64 + PAD)
    untouched(api.E_ARG, p, starts=shared, ends=shared[8:])                                      # the span arrays overlap
    assert_untouched(shared)
    untouched(api.E_ARG, p, starts=offsets)                                                      # d_start on the offsets
    untouched(api.E_ARG, p, loff=offsets)                                                        # d_list_off on the offsets
    untouched(api.E_ARG, p, ends=values[:520].view(torch.int64))                                 # d_end inside d_in
    assert offsets.cpu().tolist() == off and blob(values) == data
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        untouched(api.E_ARG, p, vals=to_dev(bytes(holed)))
        assert "newline" in api.lib().trre_last_error().decode()
    # a spans program given to the other calls
    for call in (p.scan_strings, p.match_strings, p.find_strings):
        with pytest.raises(trre_amd.TrreError) as e:
            call(values, offsets)
        assert e.value.code == api.E_ARG
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev())
    m = ctypes.c_size_t(5)
    assert api.lib().trre_scan_device(p._h, values.data_ptr(), len(data), out.data_ptr(), out.numel(), ctypes.byref(m), None) == api.E_ARG and m.value == 0
    assert bool((out == 0xA5).all())
    # ... and the same strings go through
    rc, k, st, en, lo = raw(p, values, len(data), offsets, 4, 64)
    assert (rc, k) == (0, 2) and lo[:5].cpu().tolist() == [0, 1, 1, 2, 2]
    assert st[:2].cpu().tolist() == [0, 100] and en[:2].cpu().tolist() == [100, 600] and bool((st[2:] == FILL).all())


def test_span_list_and_find_strings_still_agree():
    """span_list is m.span() per string; the spans of a program are where find_strings' outputs came from"""
    recs = [b"2024", b"", b"cat", b"catcat 7", b"dog", b"12a3", b"cat\0dog 5", b"x"]
    p, spanner = trre_amd.Program("[0-9]+|cat", "nft", "spans"), Spanner("[0-9]+|cat")
    want = spanner.lines(recs)
    assert [] in want and [(0, 3), (3, 6), (7, 8)] in want, want
    assert p.span_list(recs) == want
    assert trre_amd.Program("x*", "nft", "spans").span_list([b"bb", b""]) == [[(0, 0), (1, 1), (2, 2)], [(0, 0)]]
    found = trre_amd.Program("[0-9]+|cat", "nft", "find").find_list(recs)
    assert found == [[r[s:e] for s, e in w] for r, w in zip(recs, want)]
