"""Field k of every string on the GPU (include/trre_mi355x.h: trre_field_device_strings; Program.field_strings / field_list)
against the oracle: every string split at every match and one piece of it taken, from either end, with a validity bitmap.  Every
expectation is the oracle's spans under the wrapped acceptor (tests/span_lib.py), cut and indexed in Python (tests/field_lib.py).
Each case goes once through Program.field_strings and once through the C ABI with sentinel-filled arrays of exactly the size
asked for — the bytes behind d_out[out_len], the words behind d_out_off[nrec] and behind the bitmap's last word stay as they
were.  On top of the oracle, never instead of it: field k of string i is piece list_off[i] + k of the device's own split."""
import ctypes
import random

import pytest

import field_lib
import filter_lib
import span_lib
import split_lib
import trre_amd
from gpu_column_lib import (BFILL, FILL, PAD, assert_prefix, assert_untouched, bitmap_of, blob, carve, dev, lst, off_dev, pack, sequence,
                            soup, to_dev, words)
from span_lib import LAYOUTS, PAIRS, Spanner
from test_gpu_filter_strings import POOL          # the filter tests' pool, NULs and empties in it
from trre_amd import api

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, -1, -2, 5, -(1 << 63))


def raw(p, values, n, offsets, nrec, k, cap, null=False, out=None, ooff=None, valid=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_valid, *out_len, d_out, d_out_off, d_valid as words); d_out lies
    `out_mis` past a 16-byte boundary; null: the size query, without d_out and d_out_off"""
    if out is None:
        out = carve(cap, out_mis)
    if ooff is None:
        ooff = words(nrec + 1 + PAD)
    if valid is None:
        valid = words((nrec + 63) // 64 + PAD)
    v, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_field_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, None if null else out.data_ptr(),
                                             cap, None if null else ooff.data_ptr(), valid.data_ptr(), ctypes.byref(v), ctypes.byref(m), None)
    return rc, v.value, m.value, out, ooff, valid


def check(p, spans, recs, label, ks=KS, mis=0, out_mis=0, pieces=None):
    """for every k: one call through Program.field_strings (plain and packed) and one through the C ABI with exact room, against
    the strings' spans; with `pieces` (the device's split as (out, piece_off, list_off)) the cross-check on top"""
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    got = {}
    for k in ks:
        want = field_lib.expect(recs, spans, k)
        need, n_valid = len(want[0]), sum(want[2])
        out, oo, valid = p.field_strings(values, offsets, k)
        assert lst(valid) == want[2], (label, k)
        assert lst(oo) == want[1], (label, k)
        assert blob(out) == want[0], (label, k)
        _, _, packed = p.field_strings(values, offsets, k, packed=True)
        assert blob(packed) == field_lib.bitmap(want[2]), (label, k)
        rc, v, m, out2, oo2, valid2 = raw(p, values, len(data), offsets, nrec, k, need, out_mis=out_mis)
        assert (rc, v, m) == (0, n_valid, need), (label, k, rc, v, m, api.lib().trre_last_error())
        assert_prefix(out2, want[0], (label, k))
        assert_prefix(oo2, want[1], (label, k))
        assert bitmap_of(valid2, nrec) == (field_lib.bitmap(want[2]), [FILL] * PAD), (label, k)
        assert sum(bin(b).count("1") for b in bitmap_of(valid2, nrec)[0]) == v, (label, k)      # *n_valid is the bitmap's population
        if pieces is not None and k > -(1 << 62):
            pout, po, lo = pieces
            for i in range(nrec):
                j = lo[i] + k if k >= 0 else lo[i + 1] + k
                if want[2][i]:
                    assert lo[i] <= j < lo[i + 1] and want[0][want[1][i]:want[1][i + 1]] == pout[po[j]:po[j + 1]], (label, k, i)
                else:
                    assert not lo[i] <= j < lo[i + 1], (label, k, i)
        got[k] = want
    return got


def device_split(p, recs, mis=0):
    data, off = pack(recs)
    out, po, lo = p.split_strings(to_dev(data, mis), off_dev(off))
    return blob(out), lst(po), lst(lo)


def test_paired_patterns_and_layouts():
    """the pairs and the three symbol layouts on a few hundred random short strings and the pool with NULs and empties, every k,
    against the yardstick and against the device's own split"""
    rng = random.Random(191)
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
    layouts, n_valid, n_absent = set(), 0, 0
    for prog, acc in PAIRS + LAYOUTS:
        recs = soup(rng, b"abcdefgh ingxt059", 300) + extra + POOL
        p, spanner = trre_amd.Program(prog, "nft", "spans"), Spanner(acc)
        mis = rng.randrange(16)
        got = check(p, spanner.lines(recs), recs, prog, mis=mis, out_mis=rng.randrange(16), pieces=device_split(p, recs, mis))
        for k, want in got.items():
            n_valid += sum(want[2])
            n_absent += len(recs) - sum(want[2])
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and n_valid > 2000 and n_absent > 2000, (layouts, n_valid, n_absent)


def test_edges():
    """nrec = 0; one empty string; 70 000 empty strings under 'x*' and 'a+'; one string longer than two tiles with its field
    inside it; a NUL ends the search and the last piece keeps it; nrec of 63, 64, 65; d_in misaligned by 1 .. 15 with d_out at odd
    addresses; ',' and 'x*' by hand"""
    import torch
    rng = random.Random(192)
    star, plus, comma = (trre_amd.Program(q, "nft", "spans") for q in ("x*", "a+", ","))
    xs, ap, cs = Spanner("x*"), Spanner("a+"), Spanner(",")
    # nrec == 0: d_out_off[0] and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for k in KS:
        out, oo, valid = star.field_strings(empty, zero, k)
        assert out.numel() == 0 and lst(oo) == [0] and lst(valid) == []
        assert star.field_list([], k) == []
        rc, v, m, out, oo, valid = raw(star, empty, 0, zero, 0, k, 0)
        assert (rc, v, m) == (0, 0, 0) and lst(oo) == [0] + [FILL] * PAD and lst(valid) == [FILL] * PAD and bool((out == BFILL).all())
        rc, v, m, _, _, valid = raw(star, empty, 0, zero, 0, k, 0, null=True)
        assert (rc, v, m) == (0, 0, 0) and lst(valid) == [FILL] * PAD
    # one empty string: one empty piece under 'a+'; '' and '' around the empty match under 'x*'
    got = check(plus, [ap(b"")], [b""], "one empty, a+")
    assert got[0] == got[-1] == (b"", [0, 0], [True]) and got[1] == got[-2] == (b"", [0, 0], [False])
    got = check(star, [xs(b"")], [b""], "one empty, x*")
    assert got[1] == got[-2] == (b"", [0, 0], [True]) and got[2] == (b"", [0, 0], [False])
    # no field has bytes with nrec > 0 and the null size query: TRRE_OK, the bitmap written
    rc, v, m, _, _, valid = raw(plus, empty, 0, off_dev([0, 0]), 1, 0, 0, null=True)
    assert (rc, v, m) == (0, 1, 0) and lst(valid) == [1] + [FILL] * PAD
    # 70 000 empty strings: one tile of the input, the bitmap's 1 094 words and its tail
    many = [b""] * 70000
    got = check(star, [xs(b"")] * 70000, many, "70 000 empty, x*", ks=(1, 2, -1))
    assert got[1] == (b"", [0] * 70001, [True] * 70000) and got[2] == (b"", [0] * 70001, [False] * 70000)
    got = check(plus, [ap(b"")] * 70000, many, "70 000 empty, a+", ks=(0, 1))
    assert got[0][2] == [True] * 70000 and got[1][2] == [False] * 70000
    # one string longer than two tiles with its field inside it, across the tile edges
    long = [b"b", b"a" + b"b" * 40000 + b"a" + b"b" * 7, b"ba"]
    got = check(plus, ap.lines(long), long, "40 000 b", pieces=device_split(plus, long))
    assert got[1] == (b"b" * 40000, [0, 0, 40000, 40000], [False, True, True]) and got[-1][0] == b"b" + b"b" * 7
    assert got[0] == (b"b" + b"b", [0, 1, 1, 2], [True] * 3)
    inner = [b"b" * 20000 + b"a" + b"b" * 3 + b"a" + b"b" * 20000]                      # the field of 3 bytes, its string over three tiles
    got = check(plus, ap.lines(inner), inner, "3 of 40 005", mis=5, out_mis=3)
    assert got[1] == (b"bbb", [0, 3], [True]) and got[2][1] == [0, 20000]
    # a NUL ends the search; the last piece keeps it and everything behind it
    nuls = [b"a,b\0c,d", b"\0,", b",\0", b"", b"a,b,,c"]
    got = check(comma, cs.lines(nuls), nuls, "nuls", pieces=device_split(comma, nuls))
    assert field_lib.per_string(*got[1]) == [b"b\0c,d", None, b"\0", None, b"b"]
    assert field_lib.per_string(*got[-1]) == [b"b\0c,d", b"\0,", b"\0", b"", b"c"]
    assert comma.field_list(nuls, 1) == [b"b\0c,d", None, b"\0", None, b"b"] and comma.field_list(nuls, 2) == [None, None, None, None, b""]
    # x* on bb: empty matches split
    assert [star.field_list([b"bb"], k) for k in range(5)] == [[b""], [b"b"], [b"b"], [b""], [None]]
    # nrec around a wave; d_in at every misalignment, d_out at odd addresses
    cats, spanner = trre_amd.Program("(cat|dog)", "nft", "spans"), Spanner("(cat|dog)")
    for nrec in (63, 64, 65):
        recs = [rng.choice(POOL) for _ in range(nrec)]
        check(cats, spanner.lines(recs), recs, ("nrec", nrec))
    recs = [rng.choice(POOL) for _ in range(200)]
    spans = spanner.lines(recs)
    for mis in range(1, 16):
        check(cats, spans, recs, ("mis", mis), ks=((0, 1), (-1, 2), (-2,))[mis % 3], mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])


def test_capacity_and_sizes():
    """the null size query and cap = out_len - 1: TRRE_E_CAPACITY, both sizes and the bitmap right, d_out and d_out_off all
    sentinel; exact room succeeds"""
    rng = random.Random(193)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    recs = [bytes(rng.choice(b"0123456789xy ") for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
    spans = spanner.lines(recs)
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data), off_dev(off)
    for k in (0, 1, -1, -2):
        want = field_lib.expect(recs, spans, k)
        need, n_valid = len(want[0]), sum(want[2])
        assert need > 0 and (k in (0, -1) or (n_valid >= 300 and nrec - n_valid >= 300)), (k, n_valid)

        def refused(rc, v, m, out, oo, valid):
            assert (rc, v, m) == (api.E_CAPACITY, n_valid, need), (k, rc, v, m)
            assert_untouched(out, k)
            assert_untouched(oo, k)
            assert bitmap_of(valid, nrec) == (field_lib.bitmap(want[2]), [FILL] * PAD), k

        refused(*raw(p, values, len(data), offsets, nrec, k, 0, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, k, 0))
        refused(*raw(p, values, len(data), offsets, nrec, k, need - 1))
        rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, nrec, k, need)
        assert (rc, v, m) == (0, n_valid, need), (k, rc, v, m)
        assert_prefix(out, want[0], k)
        assert_prefix(oo, want[1], k)
        assert bitmap_of(valid, nrec) == (field_lib.bitmap(want[2]), [FILL] * PAD), k


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, k=1, **kw):
        rc, v, m, out, oo, valid = raw(p, vals, len(data), offs, 4, k, cap, **kw)
        assert rc == rc_want and (v, m) == (0, 0), (rc, v, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("ooff", oo), ("valid", valid)):
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
        for k in (0, -1):
            untouched(api.E_ARG, p, offs=off_dev(bad), k=k)                                      # bad offsets: nothing written
    # every pairwise overlap of the five arrays
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, out=values[601:], cap=1)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, ooff=as_words(values[:40]))                                          # d_in / d_out_off
    untouched(api.E_ARG, p, valid=as_words(values[592:600]))                                     # d_in / d_valid
    untouched(api.E_ARG, p, out=offsets.view(torch.uint8), cap=40)                               # d_off / d_out
    untouched(api.E_ARG, p, ooff=offsets)                                                        # d_off / d_out_off
    untouched(api.E_ARG, p, valid=offsets[4:])                                                   # d_off / d_valid
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, ooff=shared[64:])             # d_out / d_out_off
    untouched(api.E_ARG, p, out=shared.view(torch.uint8)[512:], cap=64, valid=shared[71:])       # d_out / d_valid
    untouched(api.E_ARG, p, ooff=shared, valid=shared[4:])                                       # d_out_off / d_valid
    assert bool((shared == FILL).all())
    untouched(api.E_ARG, p, valid=words(2 + PAD).view(torch.uint8)[4:].view(torch.int32))        # a bitmap that is not 8-byte aligned
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, v, m, out, oo, valid = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, 0, 700)
        assert rc == api.E_ARG and (v, m) == (0, 0) and "newline" in api.lib().trre_last_error().decode()
        for t in (out, oo, valid):
            assert_untouched(t, at)
    # ... and the same strings go through: [12 x 50], [], [12 x 250], [ab]: every digit is inside a match
    rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, 4, 0, 700)
    assert (rc, v, m) == (0, 4, 2) and lst(oo[:5]) == [0, 0, 0, 0, 2] and blob(out[:2]) == b"ab" and lst(valid[:1]) == [15]
    assert bool((out[2:] == BFILL).all()) and bool((oo[5:] == FILL).all()) and bool((valid[1:] == FILL).all())
    rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, 4, 1, 700)
    assert (rc, v, m) == (0, 2, 0) and lst(oo[:5]) == [0] * 5 and lst(valid[:1]) == [5]
    assert bool((out == BFILL).all()) and bool((oo[5:] == FILL).all()) and bool((valid[1:] == FILL).all())


def test_interleaved_with_the_other_span_calls_on_one_program():
    """field_strings, filter_strings, split_strings, span_strings and field_strings again, back to back on ONE program: a small
    input, a 330 KiB one, none, an input of exactly one tile and of one tile and a byte, the large one again.  The buffers the
    calls share only grow and every pass carves them anew: every result stays right"""
    seq = sequence(195, b"a1b", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)), framed=False)
    p, spanner = trre_amd.Program("[0-9]+", "nft", "spans"), Spanner("[0-9]+")
    for label in ("tiny", "large", "none", "one tile", "one tile and a byte", "large again"):
        recs = seq[label]
        spans = spanner.lines(recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        want_spans = span_lib.expect(spans, off)
        want_split = split_lib.expect([split_lib.cut_pieces(l, sp) for l, sp in zip(recs, spans)])
        want_filter = filter_lib.expect(recs, spans)
        for k, k2 in ((1, -1), (0, -2)):
            out, oo, valid = p.field_strings(values, offsets, k)
            assert (blob(out), lst(oo), lst(valid)) == field_lib.expect(recs, spans, k), (label, k)
            out, oo, rows = p.filter_strings(values, offsets)
            assert (blob(out), lst(oo), lst(rows)) == want_filter, (label, k)
            out, po, lo = p.split_strings(values, offsets)
            assert (blob(out), lst(po), lst(lo)) == want_split, (label, k)
            st, en, lo = p.span_strings(values, offsets)
            assert (lst(st), lst(en), lst(lo)) == want_spans, (label, k)
            out, oo, valid = p.field_strings(values, offsets, k2)
            assert (blob(out), lst(oo), lst(valid)) == field_lib.expect(recs, spans, k2), (label, k2)
