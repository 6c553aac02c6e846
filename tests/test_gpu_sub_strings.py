"""Replaced strings on the GPU (include/trre_mi355x.h: trre_sub_device_strings; Program.sub_strings / sub_list) against the
oracle: some of every string's matches replaced by what they print, the rest of the string kept.  Every expectation is composed in
Python from the oracle's spans and the oracle's find outputs (tests/sub_lib.py).  Each case goes once through
Program.sub_strings and once through the C ABI with sentinel-filled arrays of exactly the room asked for — the bytes behind
d_out[out_len] and the words behind d_out_off[nrec] stay as they were."""
import ctypes
import random

import pytest

import sub_lib
import trre_amd
from find_lib import Finder
from gpu_column_lib import (BFILL, FILL, PAD, STR_TILE, assert_prefix, assert_untouched, blob, carve, dev, lst, off_dev, pack, sequence,
                            to_dev, words)
from span_lib import Spanner
from trre_amd import api

pytestmark = pytest.mark.gpu

E63 = (1 << 63) - 1


def raw(p, values, n, offsets, nrec, first, count, cap, null=False, out=None, ooff=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_replaced, *out_len, d_out, d_out_off); d_out lies `out_mis` past a
    16-byte boundary; null: the size query, without d_out and d_out_off"""
    if out is None:
        out = carve(cap, out_mis)
    if ooff is None:
        ooff = words(nrec + 1 + PAD)
    r, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_sub_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, first, count,
                                           None if null else out.data_ptr(), cap, None if null else ooff.data_ptr(), ctypes.byref(r),
                                           ctypes.byref(m), None)
    return rc, r.value, m.value, out, ooff


def check(p, want_of, recs, label, sels=sub_lib.SELECTIONS, mis=0, out_mis=0):
    """for every (first, count): one call through Program.sub_strings and one through the C ABI with exact room, against
    want_of(first, count) = (bytes, offsets, selected matches); returns {selection: want}"""
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    got = {}
    for first, count in sels:
        want = want_of(first, count)
        out, oo = p.sub_strings(values, offsets, count=count, first=first)
        assert lst(oo) == want[1], (label, first, count)
        assert blob(out) == want[0], (label, first, count)
        rc, r, m, out2, oo2 = raw(p, values, len(data), offsets, nrec, first, count, len(want[0]), out_mis=out_mis)
        assert (rc, r, m) == (0, want[2], len(want[0])), (label, first, count, rc, r, m, api.lib().trre_last_error())
        assert_prefix(out2, want[0], (label, first, count))
        assert_prefix(oo2, want[1], (label, first, count))
        got[(first, count)] = want
    return got


def fixed(per, n_sel):
    """want_of for one selection written out by hand"""
    out = b"".join(per)
    off = [0]
    for x in per:
        off.append(off[-1] + len(x))
    return lambda first, count: (out, off, n_sel)


def test_programs_and_layouts():
    """the corpus under every program, the eight selections, a random misalignment of d_in and of d_out each; the corpus must
    tell the selections apart, and the programs cover the three symbol layouts; (0, -1) on the NUL-free strings is also what the
    scan-mode program of the same pattern returns on the device"""
    rng = random.Random(292)
    recs = sub_lib.corpus()
    free = [r for r in recs if b"\0" not in r]
    layouts, first_kind, second_kind = set(), 0, 0
    for program, acceptor in sub_lib.PROGRAMS:
        y = sub_lib.Yardstick(program, acceptor, recs)
        a, b = sub_lib.corpus_figures(y)
        if (program, acceptor) in sub_lib.ADDED:
            assert a >= 1, program
        elif program != sub_lib.ONCE:
            first_kind, second_kind = first_kind + a, second_kind + b
        p = trre_amd.Program(program, "nft", "sub")
        check(p, y.expect, recs, program, mis=rng.randrange(16), out_mis=rng.randrange(16))
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
        data, off = pack(free)
        values, offsets = to_dev(data, rng.randrange(16)), off_dev(off)
        out, oo = p.sub_strings(values, offsets)
        scan = trre_amd.Program(program, "nft", "scan")
        sout, soo = scan.scan_strings(values, offsets)
        assert lst(oo) == lst(soo) and blob(out) == blob(sout), program
    assert layouts == {4, 8, 16} and first_kind >= 400 and second_kind >= 400, (layouts, first_kind, second_kind)


def test_edges():
    """nrec = 0; one empty string; 70 000 empty strings; 40 000 matches in a row, deleted, kept and grown; one string over three
    tiles whose only selected match sits at output positions T - 1, T, T + 1; the NUL cases by hand; nrec of 63, 64, 65; d_in at
    every misalignment with d_out at odd addresses"""
    import torch
    rng = random.Random(293)
    T = STR_TILE
    # nrec == 0: d_out_off[0] and nothing else
    star = trre_amd.Program("x*:y", "nft", "sub")
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for first, count in sub_lib.SELECTIONS:
        out, oo = star.sub_strings(empty, zero, count=count, first=first)
        assert out.numel() == 0 and lst(oo) == [0] and star.sub_list([], count=count, first=first) == []
        rc, r, m, out, oo = raw(star, empty, 0, zero, 0, first, count, 0)
        assert (rc, r, m) == (0, 0, 0) and lst(oo) == [0] + [FILL] * PAD and bool((out == BFILL).all())
        assert raw(star, empty, 0, zero, 0, first, count, 0, null=True)[:3] == (0, 0, 0)
    # one empty string: ':x' and 'x*:y' match it once, 'a+:x' not at all
    for program, acceptor, hit in ((":x", "", b"x"), ("x*:y", "x*", b"y"), ("a+:x", "a+", b"")):
        p = trre_amd.Program(program, "nft", "sub")
        outs = Finder(program).lines([b""])
        assert outs == [[hit] if hit else []]
        y = lambda first, count, hit=hit: sub_lib.expect([b""], [[(0, 0)] if hit else []], [[hit] if hit else []], first, count)
        got = check(p, y, [b""], program)
        assert got[(0, -1)] == (hit, [0, len(hit)], len(hit)) and got[(1, 1)] == (b"", [0, 0], 0)
    # 70 000 empty strings under x*:y: a byte each, or nothing
    many = [b""] * 70000
    got = check(star, lambda first, count: sub_lib.expect(many, [[(0, 0)]] * 70000, [[b"y"]] * 70000, first, count), many, "70 000 empty",
                sels=((0, 1), (1, 1)))
    assert got[(0, 1)] == (b"y" * 70000, list(range(70001)), 70000) and got[(1, 1)] == (b"", [0] * 70001, 0)
    # 40 000 matches in a row
    run = [b"a" * 40000]
    dele, grow = trre_amd.Program("[aie]:", "nft", "sub"), trre_amd.Program("a:xyz", "nft", "sub")
    spans = [[(k, k + 1) for k in range(40000)]]
    assert Spanner("[aie]").lines([b"a" * 50]) == [[(k, k + 1) for k in range(50)]]
    got = check(dele, lambda first, count: sub_lib.expect(run, spans, [[b""] * 40000], first, count), run, "deleted", sels=((0, -1), (20000, -1)), out_mis=3)
    assert got[(0, -1)] == (b"", [0, 0], 40000) and got[(20000, -1)] == (b"a" * 20000, [0, 20000], 20000)
    got = check(grow, lambda first, count: sub_lib.expect(run, spans, [[b"xyz"] * 40000], first, count), run, "grown", sels=((0, -1), (39999, 1)), mis=7,
                out_mis=9)
    assert got[(0, -1)] == (b"xyz" * 40000, [0, 120000], 40000) and got[(39999, 1)] == (b"a" * 39999 + b"xyz", [0, 40002], 1)
    # one string over three tiles: its only selected match at output positions T - 1, T, T + 1 (d_out aligned: the tile edge is T)
    digits = trre_amd.Program("[0-9]+:N", "nft", "sub")
    for at in (T - 1, T, T + 1):
        rec = b"7" + b"b" * (at - 1) + b"123" + b"b" * (2 * T) + b"9"
        want = b"7" + b"b" * (at - 1) + b"N" + b"b" * (2 * T) + b"9"
        got = check(digits, fixed([want], 1), [rec], ("edge", at), sels=((1, 1),))
        assert got[(1, 1)][1] == [0, 2 * T + at + 2] and got[(1, 1)][0][at:at + 1] == b"N"
    # the NUL cases by hand
    assert dele.sub_list([b"a\0ie", b"aie", b"\0", b""]) == [b"\0ie", b"", b"\0", b""]
    comma = trre_amd.Program(",:;", "nft", "sub")
    nuls = [b"a,b\0c,d", b"\0,", b",\0", b"", b"a,b,,c"]
    assert comma.sub_list(nuls) == [b"a;b\0c,d", b"\0,", b";\0", b"", b"a;b;;c"]
    assert comma.sub_list(nuls, count=1, first=1) == [b"a,b\0c,d", b"\0,", b",\0", b"", b"a,b;,c"]
    y = sub_lib.Yardstick(",:;", ",", nuls)
    check(comma, y.expect, nuls, "nuls")
    # the examples of the definition
    cd = trre_amd.Program("(cat:dog|dog:cat)", "nft", "sub")
    assert [cd.sub_list([b"cat dog cat"], count=c, first=f)[0] for f, c in ((0, 1), (1, 1), (1, -1), (0, -1))] == \
        [b"dog dog cat", b"cat cat cat", b"cat cat dog", b"dog cat dog"]
    assert [star.sub_list([b"bb"], count=c, first=f)[0] for f, c in ((0, -1), (0, 1), (2, 1), (3, 1))] == [b"ybyby", b"ybb", b"bby", b"bb"]
    # nrec around a wave; d_in at every misalignment, d_out at odd addresses
    pool = sub_lib.corpus()
    for nrec in (63, 64, 65):
        recs = [rng.choice(pool) for _ in range(nrec)]
        check(cd, sub_lib.Yardstick("(cat:dog|dog:cat)", "(cat|dog)", recs).expect, recs, ("nrec", nrec), sels=((0, -1), (1, 1)))
    recs = [rng.choice(pool) for _ in range(200)]
    y = sub_lib.Yardstick("(cat:dog|dog:cat)", "(cat|dog)", recs)
    for mis in range(1, 16):
        check(cd, y.expect, recs, ("mis", mis), sels=(((0, -1),), ((0, 1), (1, 1)), ((2, -1),))[mis % 3], mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])


@pytest.mark.parametrize("program,acceptor", [("a:xyz", "a"), ("[0-9]+:N", "[0-9]+")])
def test_capacity_and_sizes(program, acceptor):
    """the null size query, cap = 0 and cap = out_len - 1: TRRE_E_CAPACITY, both sizes right, d_out and d_out_off all sentinel;
    exact room succeeds — for a program that grows its input and one that shrinks it"""
    rng = random.Random(294)
    p = trre_amd.Program(program, "nft", "sub")
    recs = [bytes(rng.choice(b"0123456789aab ") for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
    y = sub_lib.Yardstick(program, acceptor, recs)
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data), off_dev(off)
    for first, count in ((0, -1), (0, 1), (1, 2)):
        want = y.expect(first, count)
        need = len(want[0])
        assert need != len(data) and want[2] >= 300, (first, count, need)

        def refused(rc, r, m, out, oo):
            assert (rc, r, m) == (api.E_CAPACITY, want[2], need), (first, count, rc, r, m)
            assert_untouched(out, (first, count))
            assert_untouched(oo, (first, count))

        refused(*raw(p, values, len(data), offsets, nrec, first, count, 0, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, first, count, 0))
        refused(*raw(p, values, len(data), offsets, nrec, first, count, need - 1))
        rc, r, m, out, oo = raw(p, values, len(data), offsets, nrec, first, count, need)
        assert (rc, r, m) == (0, want[2], need), (first, count, rc, r, m)
        assert_prefix(out, want[0], (first, count))
        assert_prefix(oo, want[1], (first, count))


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, first=0, count=-1, **kw):
        rc, r, m, out, oo = raw(p, vals, len(data), offs, 4, first, count, cap, **kw)
        assert rc == rc_want and (r, m) == (0, 0), (rc, r, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("ooff", oo)):
            if name not in kw:
                assert_untouched(t, name)
        assert lst(offsets) == off and blob(values) == data

    for mode in ("scan", "match", "find", "spans"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    p = trre_amd.Program("[0-9]+:N", "nft", "sub")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)                                                              # forced backtracking
    p.set_kernel(trre_amd.KERNEL_AUTO)
    untouched(api.E_UNSUPPORTED, trre_amd.Program("x:\n", "nft", "sub"))                         # a newline-printing program
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        untouched(api.E_ARG, p, offs=off_dev(bad))                                               # bad offsets: nothing written
    untouched(api.E_ARG, p, first=-1)
    untouched(api.E_ARG, p, first=-(1 << 63), count=1)
    # every pairwise overlap of the four arrays
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, out=values[601:], cap=1)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, ooff=as_words(values[:40]))                                          # d_in / d_out_off
    untouched(api.E_ARG, p, out=offsets.view(torch.uint8), cap=40)                               # d_off / d_out
    untouched(api.E_ARG, p, ooff=offsets)                                                        # d_off / d_out_off
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, ooff=shared[64:])             # d_out / d_out_off
    assert bool((shared == FILL).all())
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, r, m, out, oo = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, 0, -1, 700)
        assert rc == api.E_ARG and (r, m) == (0, 0) and "newline" in api.lib().trre_last_error().decode()
        assert_untouched(out, at)
        assert_untouched(oo, at)
    # ... and the same strings go through: [12 x 50], [], [12 x 250], [ab]
    rc, r, m, out, oo = raw(p, values, len(data), offsets, 4, 0, -1, 700)
    assert (rc, r, m) == (0, 2, 4)
    assert_prefix(out, b"NNab")
    assert_prefix(oo, [0, 1, 1, 2, 4])


def test_interleaved_on_one_program():
    """a small input, a 330 KiB one, none, an input of exactly one tile and of one tile and a byte, the large one again, on ONE sub
    program with alternating selections, a spans program and a find program of the same pattern called in between on the same
    device: the buffers only grow and every result stays right"""
    import find_lib  # noqa: F401
    import span_lib
    seq = sequence(295, b"a1b", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)), framed=False)
    p, spans_p, find_p = (trre_amd.Program("[0-9]+:N", "nft", m) for m in ("sub", "spans", "find"))
    for turn, label in enumerate(("tiny", "large", "none", "one tile", "one tile and a byte", "large again")):
        recs = seq[label]
        y = sub_lib.Yardstick("[0-9]+:N", "[0-9]+", recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        sels = ((0, -1), (1, 1)) if turn % 2 else ((0, 1), (2, -1))
        for k, (first, count) in enumerate(sels):
            want = y.expect(first, count)
            out, oo = p.sub_strings(values, offsets, count=count, first=first)
            assert (blob(out), lst(oo)) == want[:2], (label, first, count)
            if k == 0:
                st, en, lo = spans_p.span_strings(values, offsets)
                assert (lst(st), lst(en), lst(lo)) == span_lib.expect(y.spans, off), label
                fout, fo, flo = find_p.find_strings(values, offsets)
                assert blob(fout) == b"".join(o for per in y.outs for o in per) and lst(flo) == lst(lo), label
