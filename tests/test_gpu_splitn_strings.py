"""Split strings at the first or last matches only, and field k of that split, on the GPU (include/trre_mi355x.h:
trre_splitn_device_strings, trre_fieldn_device_strings; Program.split_strings / field_strings with limit= and from_end=) against
the oracle: every expectation is the oracle's spans under the wrapped acceptor (tests/span_lib.py) with the cut rule applied in
Python and the pieces cut from the uncut string (tests/splitn_lib.py).  Each case goes once through the Python method and once
through the C ABI with sentinel-filled arrays of exactly the size asked for: what lies behind the used part stays as it was.
Then the identities against the device's own split and field calls, the placed edges of the kernels, and the capacity rules."""
import ctypes
import random

import pytest

import field_lib
import find_lib
import span_lib
import split_lib
import splitn_lib
import trre_amd
from find_lib import lines_of
from gpu_column_lib import FILL, PAD, assert_prefix, assert_untouched, blob, carve, dev, lst, off_dev, pack, soup, to_dev, words
from span_lib import LAYOUTS, PAIRS, Spanner
from splitn_lib import INT64_MAX, INT64_MIN
from trre_amd import api

pytestmark = pytest.mark.gpu

ENDS = (False, True)
_progs = {}


def program(pat):
    if pat not in _progs:
        _progs[pat] = trre_amd.Program(pat, "nft", "spans")
    return _progs[pat]


def raw_split(p, values, n, offsets, nrec, limit, from_end, cap, pcap, null=False, out_mis=0):
    """trre_splitn_device_strings itself, with sentinel-filled arrays: (rc, *n_pieces, *out_len, d_out, d_piece_off, d_list_off)"""
    out, poff, loff = carve(cap, out_mis), words(pcap + 1 + PAD), words(nrec + 1 + PAD)
    k, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_splitn_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, limit, int(from_end),
                                              None if null else out.data_ptr(), cap, None if null else poff.data_ptr(), pcap, loff.data_ptr(),
                                              ctypes.byref(k), ctypes.byref(m), None)
    return rc, k.value, m.value, out, poff, loff


def raw_field(p, values, n, offsets, nrec, k, limit, from_end, cap, null=False, out_mis=0):
    """trre_fieldn_device_strings itself: (rc, *n_valid, *out_len, d_out, d_out_off, d_valid as words)"""
    out, ooff, valid = carve(cap, out_mis), words(nrec + 1 + PAD), words((nrec + 63) // 64 + PAD)
    v, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_fieldn_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, limit, int(from_end),
                                              None if null else out.data_ptr(), cap, None if null else ooff.data_ptr(), valid.data_ptr(),
                                              ctypes.byref(v), ctypes.byref(m), None)
    return rc, v.value, m.value, out, ooff, valid


def check_split(p, spans, recs, limit, from_end, label, mis=0, out_mis=0, column=None):
    """one call through Program.split_strings and one through the C ABI with exact room; returns the expectation"""
    data, off = pack(recs)
    want = splitn_lib.expect(recs, spans, limit, from_end)
    need, pieces, nrec = len(want[0]), len(want[1]) - 1, len(recs)
    values, offsets = column or (to_dev(data, mis), off_dev(off))
    label = (label, limit, from_end)
    out, po, lo = p.split_strings(values, offsets, limit=limit, from_end=from_end)
    assert lst(lo) == want[2], label
    assert lst(po) == want[1], label
    assert blob(out) == want[0], label
    rc, k, m, out2, po2, lo2 = raw_split(p, values, len(data), offsets, nrec, limit, from_end, need, pieces, out_mis=out_mis)
    assert (rc, k, m) == (0, pieces, need), (label, rc, k, m, api.lib().trre_last_error())
    for t, w in zip((out2, po2, lo2), want):
        assert_prefix(t, w, label)
    return want


def check_field(p, spans, recs, k, limit, from_end, label, mis=0, out_mis=0, column=None):
    data, off = pack(recs)
    want = splitn_lib.expect_field(recs, spans, k, limit, from_end)
    need, n_valid, nrec = len(want[0]), sum(want[2]), len(recs)
    values, offsets = column or (to_dev(data, mis), off_dev(off))
    label = (label, k, limit, from_end)
    out, oo, valid = p.field_strings(values, offsets, k, limit=limit, from_end=from_end)
    assert lst(valid) == want[2], label
    assert lst(oo) == want[1], label
    assert blob(out) == want[0], label
    rc, v, m, out2, oo2, valid2 = raw_field(p, values, len(data), offsets, nrec, k, limit, from_end, need, out_mis=out_mis)
    assert (rc, v, m) == (0, n_valid, need), (label, rc, v, m, api.lib().trre_last_error())
    assert_prefix(out2, want[0], label)
    assert_prefix(oo2, want[1], label)
    nw = (nrec + 63) // 64
    assert blob(valid2[:nw]) == field_lib.bitmap(want[2]) and bool((valid2[nw:] == FILL).all()), label
    return want


def fields_of(limit):
    return sorted({0, 1, -1, -2, limit, limit + 1, -(limit + 1), -(limit + 2)})


_cases = None


def oracle_cases():
    """the PAIRS + LAYOUTS soups of 300 strings and the golden acceptors' first 2 000 lines, each with its spans from the oracle:
    computed once, shared by the parametrised cases and left unchanged"""
    global _cases
    if _cases is None:
        rng = random.Random(301)
        extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
        golden = span_lib.golden_acceptors()
        assert len(golden) >= 18, len(golden)
        found = [(pat, pat, name, lines[:2000]) for pat, vs in golden.items() for name, lines in vs]
        found += [(prog, acc, "pair", soup(rng, b"abcdefgh ingxt059", 300) + extra) for prog, acc in PAIRS + LAYOUTS]
        spanners = {}
        _cases = []
        for prog, acc, name, recs in found:
            spanner = spanners.setdefault(acc, Spanner(acc))
            _cases.append((prog, name, recs, spanner.lines(recs), rng.randrange(16), rng.randrange(16)))
    return _cases


@pytest.mark.parametrize("from_end", ENDS)
@pytest.mark.parametrize("limit", (0, 1, 3))
def test_against_the_oracle_yardstick(limit, from_end):
    """no case skipped; all three symbol layouts hit; one column on the device per case, shared by the split and its fields"""
    layouts, n_pieces, n_valid = set(), 0, 0
    for prog, name, recs, spans, mis, out_mis in oracle_cases():
        p = program(prog)
        data, off = pack(recs)
        column = (to_dev(data, mis), off_dev(off))
        want = check_split(p, spans, recs, limit, from_end, (prog, name), out_mis=out_mis, column=column)
        n_pieces += want[2][-1]
        for k in fields_of(limit):
            n_valid += sum(check_field(p, spans, recs, k, limit, from_end, (prog, name), out_mis=out_mis, column=column)[2])
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16} and n_pieces > 10000 and n_valid > 10000, (layouts, n_pieces, n_valid)


def test_the_vectors_the_reference_does_not_survive_diverge():
    _, dead, _, _ = find_lib.vectors()
    assert len(dead) == 13
    for pat, name, data in dead:
        recs = lines_of(data)
        data2, off = pack(recs)
        p, values, offsets = program(pat), to_dev(data2), off_dev(off)
        rc, k, m, _, _, _ = raw_split(p, values, len(data2), offsets, len(recs), 1, True, 1 << 16, 1 << 16)
        assert rc == api.E_DIVERGES and (k, m) == (0, 0), (pat, name, rc, k, m)
        assert "stack max capacity" in api.lib().trre_last_error().decode(), (pat, name)
        rc, v, m, _, _, _ = raw_field(p, values, len(data2), offsets, len(recs), 0, 1, False, 1 << 16)
        assert rc == api.E_DIVERGES and (v, m) == (0, 0), (pat, name, rc, v, m)


def test_identities_against_the_devices_own_calls():
    """limit = -1 and limit = 2^63 - 1 give the split and field calls' arrays byte for byte, with either flag value; limit = 0
    gives d_in back; fieldn(k) is piece k of splitn, for every string"""
    rng = random.Random(302)
    for prog, alpha in (("[0-9]+:N", b"0123456789xy "), ("x*", b"xxy"), (",", b"ab,,")):
        p = program(prog)
        recs = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30, 200]))) for _ in range(1500)] + [b"1,\0,2", b"\0"]
        data, off = pack(recs)
        values, offsets = to_dev(data, 5), off_dev(off)
        whole = tuple(map(lst, p.split_strings(values, offsets)))
        for limit in (-1, INT64_MAX, INT64_MIN, 1 << 40):
            for from_end in ENDS:
                assert tuple(map(lst, p.split_strings(values, offsets, limit=limit, from_end=from_end))) == whole, (prog, limit, from_end)
                for k in (0, 1, -1, -2, 3):
                    a = p.field_strings(values, offsets, k, packed=True)
                    b = p.field_strings(values, offsets, k, packed=True, limit=limit, from_end=from_end)
                    assert all(lst(x) == lst(y) for x, y in zip(a, b)), (prog, k, limit, from_end)
        for from_end in ENDS:
            out, po, lo = p.split_strings(values, offsets, limit=0, from_end=from_end)
            assert blob(out) == data and lst(po) == off and lst(lo) == list(range(len(recs) + 1)), (prog, from_end)
        for limit in (0, 1, 2, 5):
            for from_end in ENDS:
                out, po, lo = p.split_strings(values, offsets, limit=limit, from_end=from_end)
                per = split_lib.per_string(blob(out), lst(po), lst(lo))
                for k in fields_of(limit):
                    fo, foo, fv = p.field_strings(values, offsets, k, limit=limit, from_end=from_end)
                    got = field_lib.per_string(blob(fo), lst(foo), lst(fv))
                    assert got == [field_lib.pick(w, k) for w in per], (prog, k, limit, from_end)


def test_tiles_wholly_inside_one_match():
    """'a+' on 40 000 a with limit 0 (every byte kept) and limit 1 (nothing kept); 'b+' on 40 000 a"""
    plus, ap = program("a+"), Spanner("a+")
    long = [b"", b"a" * 40000, b"ba"]
    spans = ap.lines(long)
    for from_end in ENDS:
        assert check_split(plus, spans, long, 0, from_end, "40 000 a") == (b"".join(long), [0, 0, 40000, 40002], [0, 1, 2, 3])
        assert check_split(plus, spans, long, 1, from_end, "40 000 a") == (b"b", [0, 0, 0, 0, 1, 1], [0, 1, 3, 5])
        for k in (0, 1, -1):
            check_field(plus, spans, long, k, 0, from_end, "40 000 a")
            check_field(plus, spans, long, k, 1, from_end, "40 000 a")
    recs = [b"a" * 40000]
    for limit in (0, 1):
        for from_end in ENDS:
            assert check_split(program("b+"), Spanner("b+").lines(recs), recs, limit, from_end, "b+") == (recs[0], [0, 40000], [0, 1])


def test_commas_at_the_tile_and_piece_edges():
    """',' on one string of about 33 000 bytes.  Comma j at input position p has its 0x01 at framed position p + 2 j, its position
    byte behind it and its 0x02 behind that: comma 1 puts them at 16 382 .. 16 384, 16 383 .. 16 385 and 16 384 .. 16 386 in
    turn, comma 3 ends a 64-byte piece the same three ways; the limits make the last (the first) cutting match the one before an
    edge, the one on it and the one after it, from both ends"""
    comma, cs = program(","), Spanner(",")
    for shift in (0, 1, 2):
        at = [100, 16380 + shift, 16421 + shift, 20471 + shift, 30000, 32990]
        body = bytearray(b"z" * 33000)
        for q in at:
            body[q] = ord(",")
        recs = [bytes(body)]
        spans = cs.lines(recs)
        assert spans == [[(q, q + 1) for q in at]]
        assert at[1] + 2 == 16382 + shift and (at[3] + 6) % 64 == 61 + shift
        for limit in (1, 2, 3, 4, 5, 6):
            for from_end in ENDS:
                check_split(comma, spans, recs, limit, from_end, ("commas", shift), out_mis=shift + 1)
                for k in (1, -2, limit):
                    check_field(comma, spans, recs, k, limit, from_end, ("commas", shift))


def test_empty_matches_and_a_newline_two_tiles_behind_the_first_marker():
    """'x*' on 20 000 b with limits 0, 1 and 10 000; 70 000 empty strings under 'x*' with limit 1; from the end, a string whose
    closing newline lies two tiles behind its first marker: c comes from the list offsets, not from the tile"""
    star, xs = program("x*"), Spanner("x*")
    recs = [b"b" * 20000]
    spans = xs.lines(recs)
    assert len(spans[0]) == 20001
    for limit in (0, 1, 10000):
        for from_end in ENDS:
            want = check_split(star, spans, recs, limit, from_end, "20 000 b")
            assert want[0] == recs[0] and want[2] == [0, min(limit, 20001) + 1]
            for k in (0, 1, -1, limit):
                check_field(star, spans, recs, k, limit, from_end, "20 000 b")
    empties = [b""] * 70000
    spans = [xs(b"")] * 70000
    for from_end in ENDS:
        want = check_split(star, spans, empties, 1, from_end, "70 000 empty")
        assert want[0] == b"" and len(want[1]) == 140001 and want[2][-1] == 140000
        assert sum(check_field(star, spans, empties, 1, 1, from_end, "70 000 empty")[2]) == 70000
    comma, cs = program(","), Spanner(",")
    recs = [b"k", b"a,b" + b"z" * 40000 + b",c,d", b",", b""]
    spans = cs.lines(recs)
    for limit in (1, 2, 3):
        for from_end in ENDS:
            check_split(comma, spans, recs, limit, from_end, "far newline", mis=3)
            for k in (0, 1, -1):
                check_field(comma, spans, recs, k, limit, from_end, "far newline", mis=3)


def test_nrec_around_a_wave_nuls_and_misalignment():
    import torch
    rng = random.Random(303)
    cats, spanner = program("(cat|dog)"), Spanner("(cat|dog)")
    # nrec == 0: entry 0 of the arrays and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for from_end in ENDS:
        out, po, lo = cats.split_strings(empty, zero, limit=1, from_end=from_end)
        assert out.numel() == 0 and lst(po) == [0] and lst(lo) == [0]
        rc, k, m, out, po, lo = raw_split(cats, empty, 0, zero, 0, 1, from_end, 0, 0)
        assert (rc, k, m) == (0, 0, 0) and lst(lo) == [0] + [FILL] * PAD and lst(po) == [0] + [FILL] * PAD
        rc, v, m, out, oo, valid = raw_field(cats, empty, 0, zero, 0, 0, 1, from_end, 0)
        assert (rc, v, m) == (0, 0, 0) and lst(oo) == [0] + [FILL] * PAD
        assert cats.split_list([], limit=1, from_end=from_end) == [] and cats.field_list([], 0, limit=1, from_end=from_end) == []
    # a NUL at the first, a middle and the last byte
    nuls = [b"\0cat dog", b"a cat\0dog", b"cat dog\0", b"\0", b"cat", b"dog\0\0cat", b"cat dog cat\0 dog"]
    spans = spanner.lines(nuls)
    assert splitn_lib.split_lines(spanner, nuls, 1, False)[:3] == [[b"\0cat dog"], [b"a ", b"\0dog"], [b"", b" dog\0"]]
    assert cats.split_list(nuls, limit=1) == splitn_lib.split_lines(spanner, nuls, 1, False)
    assert cats.split_list(nuls, limit=1, from_end=True)[2] == [b"cat ", b"\0"]
    assert cats.field_list([b"a=b=c"], 1, limit=1) == [None] and program("=").field_list([b"a=b=c", b"k"], 1, limit=1) == [b"b=c", None]
    assert program("\\.").field_list([b"x.tar.gz", b"noext"], 0, limit=1, from_end=True) == [b"x.tar", b"noext"]
    pool = [b"", b"cat", b"a cat and a dog", b"xyz", b"\0 cat", b"do\0g cat", b"catdogcat", b"c" * 40, b"dog cat dog cat"]
    for limit in (0, 1, 2):
        for from_end in ENDS:
            check_split(cats, spans, nuls, limit, from_end, "nuls")
            for nrec in (63, 64, 65):
                recs = [rng.choice(pool) for _ in range(nrec)]
                w = spanner.lines(recs)
                check_split(cats, w, recs, limit, from_end, ("nrec", nrec))
                for k in (0, 1, -1):
                    check_field(cats, w, recs, k, limit, from_end, ("nrec", nrec))
    recs = [rng.choice(pool) for _ in range(200)]
    w = spanner.lines(recs)
    for mis in range(1, 16):
        check_split(cats, w, recs, 1, bool(mis & 1), ("mis", mis), mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])
        check_field(cats, w, recs, -1, 1, bool(mis & 1), ("mis", mis), mis=mis, out_mis=(1, 3, 7, 9, 15)[mis % 5])


def test_capacity_and_sizes():
    """the size query with nulls, cap one short and piece_cap one short: TRRE_E_CAPACITY, both sizes right, d_list_off (d_valid)
    valid, d_out and the offsets all sentinel; a retry with exact room succeeds"""
    rng = random.Random(304)
    for prog, acc, alpha in (("[0-9]+:N", "[0-9]+", b"0123456789xy "), ("x*", "x*", b"xxy")):
        p, spanner = program(prog), Spanner(acc)
        recs = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
        spans = spanner.lines(recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        nrec = len(recs)
        for limit, from_end in ((1, False), (2, True)):
            want = splitn_lib.expect(recs, spans, limit, from_end)
            need, pieces = len(want[0]), len(want[1]) - 1
            assert 0 < need < len(data) and pieces > nrec + nrec // 4, prog

            def refused(rc, k, m, out, po, lo):
                assert (rc, k, m) == (api.E_CAPACITY, pieces, need), (prog, rc, k, m)
                assert_untouched(out, prog)
                assert_untouched(po, prog)
                assert_prefix(lo, want[2], prog)

            refused(*raw_split(p, values, len(data), offsets, nrec, limit, from_end, 0, 0, null=True))
            refused(*raw_split(p, values, len(data), offsets, nrec, limit, from_end, need - 1, pieces))
            refused(*raw_split(p, values, len(data), offsets, nrec, limit, from_end, need, pieces - 1))
            rc, k, m, out, po, lo = raw_split(p, values, len(data), offsets, nrec, limit, from_end, need, pieces)
            assert (rc, k, m) == (0, pieces, need), (prog, rc, k, m)
            assert_prefix(out, want[0], prog)
            assert_prefix(po, want[1], prog)
            assert_prefix(lo, want[2], prog)
            fw = splitn_lib.expect_field(recs, spans, 1, limit, from_end)
            fneed, n_valid, nw = len(fw[0]), sum(fw[2]), (nrec + 63) // 64
            assert fneed > 0
            for cap, null in ((0, True), (fneed - 1, False)):
                rc, v, m, out, oo, valid = raw_field(p, values, len(data), offsets, nrec, 1, limit, from_end, cap, null=null)
                assert (rc, v, m) == (api.E_CAPACITY, n_valid, fneed), (prog, rc, v, m)
                assert_untouched(out, prog)
                assert_untouched(oo, prog)
                assert blob(valid[:nw]) == field_lib.bitmap(fw[2]) and bool((valid[nw:] == FILL).all())
            rc, v, m, out, oo, valid = raw_field(p, values, len(data), offsets, nrec, 1, limit, from_end, fneed)
            assert (rc, v, m) == (0, n_valid, fneed)
            assert_prefix(out, fw[0], prog)
            assert_prefix(oo, fw[1], prog)
