"""The per-thread bodies of k_field_init, k_field_pick, k_field_count and k_field_emit (trre_amd/csrc/records_block.hpp:
field_init, field_pick_markers, field_count_strings, field_mark, field_emit_offsets, and the span and filter bodies they reuse)
run on the host by tests/field_shim.cpp against numpy.  A column is strings of given lengths with ordered, disjoint spans drawn
here; the span call's list offsets and framed text are written out from them, so the range [lo_i, hi_i) of field k is known
before the shim runs.  Checked: lo and hi of every string, each stored exactly once by the init pass or by one marker lane; the
bitmap's words and tail bits; the fields' bytes in input order; out_off, entry 0 by tile 0 alone and every other byte and word
once; nothing behind out_len, nrec + 1 and the bitmap's last word."""
import ctypes
import random

import numpy as np

import column_shim_lib

GEOS = (0, 1, 2, 3)
UNSTORED = np.int64(-0x1111111111111112)          # 0xEEEE... as a signed word
KS = (0, 1, 2, -1, -2, 5, -(1 << 63))

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("field")
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.shim_field_tile.argtypes = [i32]
        L.shim_field_tile.restype = i64
        L.shim_field.argtypes = [i32, vp, i64, vp, vp, i64, i64, vp, i64, i32, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_field_tile(geo)


def far(T):
    """as if 5 * 2^32 input bytes with 2^23 T matches and 2^34 + 11 field bytes came before"""
    return dict(pos0=((5 << 32) // T + 3) * T, ra0=T << 23, rk0=(1 << 34) + 11)


def frame(lens, spans):
    """the span call's framed text of the column: per string its position bytes, A in front of every match and B behind it, '\\n'"""
    parts = []
    for l, w in zip(lens, spans):
        at = 0
        for s, e in w:
            assert at <= s <= e <= l, (l, w)
            parts.append(b"." * (s - at) + b"\x01" + b"." * (e - s) + b"\x02")
            at = e
        parts.append(b"." * (l - at) + b"\n")
    return b"".join(parts)


def bounds(l, w, k):
    """(has, lo, hi) of field k of a string of l bytes with the spans w, relative to the string: the pieces' definition"""
    c = len(w)
    kk = k if k >= 0 else c + 1 + k
    if not 0 <= kk <= c:
        return False, l, l
    return True, (0 if kk == 0 else w[kk - 1][1]), (l if kk == c else w[kk][0])


def check(geo, lens, spans, k, src_mis=0, dst_mis=0, pos0=0, ra0=0, rk0=0, seed=1):
    """the shim against numpy on one column.  Returns (n_valid, out_len)"""
    nrec, n = len(lens), int(sum(lens))
    assert nrec >= 1 and len(spans) == nrec and not (pos0 and lens[0] == 0)
    off = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    loff = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(w) for w in spans], dtype=np.int64), out=loff[1:])
    src = np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8)
    framed = np.frombuffer(frame(lens, spans), dtype=np.uint8)
    bd = [bounds(l, w, k) for l, w in zip(lens, spans)]
    has = np.asarray([b[0] for b in bd], dtype=bool)
    lo = off[:-1] + np.asarray([b[1] for b in bd], dtype=np.int64)
    hi = off[:-1] + np.asarray([b[2] for b in bd], dtype=np.int64)
    want_off = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(hi - lo, out=want_off[1:])
    out_len, n_valid = int(want_off[-1]), int(has.sum())
    keep = np.zeros(n + 1, dtype=np.int64)
    np.add.at(keep, lo, 1)
    np.add.at(keep, hi, -1)
    want_out = src[np.cumsum(keep)[:n] > 0]
    assert len(want_out) == out_len
    words = (nrec + 63) // 64
    want_bits = np.zeros(words * 64, dtype=np.uint8)
    want_bits[:nrec] = has
    want_valid = np.packbits(want_bits, bitorder="little").view(np.uint64)
    out = np.full(out_len + 1, 0x11, dtype=np.uint8)
    oo = np.full(nrec + 2, -5, dtype=np.int64)
    valid = np.full(words + 1, 0x1111, dtype=np.uint64)
    glo, ghi = np.full(nrec + 1, -5, dtype=np.int64), np.full(nrec + 1, -5, dtype=np.int64)
    totals, stores = np.zeros(2, dtype=np.int64), np.zeros(5, dtype=np.int64)
    so, sl = off + pos0, loff + ra0
    rc = lib().shim_field(geo, src.ctypes.data if n else None, n, so.ctypes.data, sl.ctypes.data, nrec, k, framed.ctypes.data, len(framed), src_mis,
                          dst_mis, pos0, ra0, rk0, n_valid, out_len, out.ctypes.data, oo.ctypes.data, valid.ctypes.data, glo.ctypes.data,
                          ghi.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, n, nrec, k, n_valid, out_len, src_mis, dst_mis, pos0)
    assert rc == 0, (rc,) + label
    assert np.array_equal(glo[:nrec], lo + pos0) and np.array_equal(ghi[:nrec], hi + pos0), label
    assert np.array_equal(valid[:words], want_valid), label                                      # words and tail bits
    assert totals.tolist() == [n_valid, out_len], (label, totals)
    assert np.array_equal(out[:out_len], want_out), label
    assert np.array_equal(oo[1:nrec + 1], want_off[1:] + rk0), label
    assert oo[0] == (UNSTORED if pos0 else 0), label
    assert out[out_len] == 0x11 and oo[nrec + 1] == -5 and valid[words] == 0x1111 and glo[nrec] == -5 and ghi[nrec] == -5, label
    assert stores.tolist() == [out_len, nrec + (0 if pos0 else 1), words, nrec, nrec], (label, stores)      # every byte and word once
    if k in (0, -1) and not any(spans) and not pos0 and not rk0:
        assert np.array_equal(out[:out_len], src) and np.array_equal(oo[:nrec + 1], off), label  # every field its whole string
    return n_valid, out_len


def chop(rng, n, longest):
    """string lengths that add up to n, empty ones among them"""
    lens = []
    while sum(lens) < n:
        lens.append(min(rng.choice((0, 0, 1, 2, 3, 7, 16, longest)), n - sum(lens)))
    return lens or [0]


def draw(rng, l, density=4):
    """ordered, disjoint spans in a string of l bytes, empty ones among them, never two at one place"""
    w, x = [], 0
    while x <= l:
        if rng.randrange(density) == 0:
            e = min(x + rng.choice((0, 0, 1, 1, 2, 5)), l)
            w.append((x, e))
            x = e + 1
        else:
            x += 1
    return w


def around(lo, hi):
    """the spans that make [lo, hi) field 1 (and field -2) of a string: a 1-byte match in front of lo, one behind hi"""
    return [(lo - 1, lo), (hi, hi + 1)]


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_by_hand():
    """a,b,,c as [1, 1, 0, 1] bytes around three 1-byte matches; an empty string; a string without a match"""
    lens, spans = [6, 0, 3], [[(1, 2), (3, 4), (4, 5)], [], []]
    assert check(0, lens, spans, 0) == (3, 4)               # a, '', xyz
    assert check(0, lens, spans, 1) == (1, 1)               # b
    assert check(0, lens, spans, 2) == (1, 0)               # ''
    assert check(0, lens, spans, 3) == (1, 1)               # c
    assert check(0, lens, spans, 4) == (0, 0)
    assert check(0, lens, spans, -1) == (3, 4)              # c, '', xyz
    assert check(0, lens, spans, -4) == (1, 1)              # a
    assert check(0, lens, spans, -5) == (0, 0)
    assert check(0, lens, spans, -(1 << 63)) == (0, 0) and check(0, lens, spans, (1 << 63) - 1) == (0, 0)
    # x* on bb: empty matches split
    assert [check(0, [2], [[(0, 0), (1, 1), (2, 2)]], k) for k in range(5)] == [(1, 0), (1, 1), (1, 1), (1, 0), (0, 0)]


def test_lengths_around_the_tile_edges():
    """input lengths 0, 1, 15, 16, 17, T - 1, T, T + 1 and 3 T: one string, random strings; no match (every field the whole
    string for k = 0 and -1: out == in, out_off == off; every field absent for the others), random matches"""
    rng = random.Random(191)
    for geo in GEOS:
        T = tile(geo)
        for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T):
            for lens in ([n], chop(rng, n, 40), chop(rng, n, T // 2 + 3)):
                for spans in ([[] for _ in lens], [draw(rng, l) for l in lens]):
                    for k in KS:
                        check(geo, lens, spans, k, src_mis=rng.randrange(16), dst_mis=rng.randrange(16), seed=n + 1)


def test_every_field_empty():
    """k out of range everywhere; and every byte matched, so that every piece is empty and present"""
    for geo in GEOS:
        T = tile(geo)
        lens = [5] * ((2 * T + 10) // 5)
        assert check(geo, lens, [[(1, 2)] for _ in lens], 2, src_mis=geo) == (0, 0)
        assert check(geo, lens, [[(0, 5)] for _ in lens], 0, dst_mis=3) == (len(lens), 0)
        assert check(geo, lens, [[(0, 5)] for _ in lens], -1, dst_mis=3) == (len(lens), 0)


def test_range_inside_a_string_over_three_tiles():
    """the field strictly inside a string that spans three tiles, lo and hi at T - 1, T, T + 1 of the v-space and around 2 T"""
    for geo in GEOS:
        T = tile(geo)
        for mis in (0, 1, 15):
            first = 7
            for lo in (T - 1, T, T + 1):
                for hi in (lo, lo + 1, 2 * T - 1, 2 * T, 2 * T + 1):
                    a, b = lo - mis - first, hi - mis - first                       # relative to the long string
                    for k in (1, -2):
                        assert check(geo, [first, 3 * T, 9], [[], around(a, b), []], k, src_mis=mis, dst_mis=(mis * 7 + hi) % 16) == (1, hi - lo)


def test_string_ends_in_a_tile_its_field_lies_before():
    """a string that ends in tile b with its range wholly in tile b - 1: tile b clips it to nothing, tile b - 1 has it as the
    string that covers its end; and the reverse, the range wholly in the string's last tile"""
    for geo in GEOS:
        T = tile(geo)
        for mis in (0, 9):
            for end in (T + 1, T + 40, 2 * T - 1):
                l = end - mis - 3
                for vlo, vhi in ((T // 2, T // 2 + 20), (T - 30, T - 2), (mis + 8, mis + 8)):      # (in the v-space; the string starts at mis + 3)
                    lo, hi = vlo - mis - 3, vhi - mis - 3
                    assert check(geo, [3, l, 6], [[], around(lo, hi), []], 1, src_mis=mis, dst_mis=5) == (1, hi - lo)
                lo = T - mis - 3
                assert check(geo, [3, l, 6], [[], around(lo, l - 1), []], 1, src_mis=mis, dst_mis=11) == (1, l - 1 - lo)


def test_one_byte_strings_present_and_absent_in_turn():
    """over 2 T bytes: every destination vector has 16 sources.  k = 1 with a match in every other string: the others have no
    field 1; the matched ones have an empty one — and k = 0 keeps the unmatched bytes and the empty pieces in front of a match"""
    for geo in GEOS:
        T = tile(geo)
        for first in (0, 1):
            spans = [[(0, 1)] if (i + first) & 1 else [] for i in range(2 * T)]
            assert check(geo, [1] * (2 * T), spans, 1, src_mis=3 * geo, dst_mis=5 + geo) == (T, 0)
            assert check(geo, [1] * (2 * T), spans, 0, src_mis=1, dst_mis=0) == (2 * T, T)
            spans = [[(1, 1)] if (i + first) & 1 else [] for i in range(2 * T)]             # an empty match at the string's end
            assert check(geo, [1] * (2 * T), spans, -2, src_mis=2, dst_mis=13) == (T, T)


def test_all_strings_empty():
    """n = 0, nrec = 1, 63, 64, 65 and 70 000: one tile, no byte; the bitmap's words and tail bits"""
    for geo in GEOS:
        for nrec in (1, 63, 64, 65, 70000):
            none = [[] for _ in range(nrec)]
            assert check(geo, [0] * nrec, none, 0) == (nrec, 0)
            assert check(geo, [0] * nrec, none, -1, src_mis=geo + 1) == (nrec, 0)
            assert check(geo, [0] * nrec, none, 1) == (0, 0)
            some = [[(0, 0)] if (i * 7) % 3 == 0 else [] for i in range(nrec)]              # x* on '': one empty match
            assert check(geo, [0] * nrec, some, 1, dst_mis=geo)[0] == sum(1 for w in some if w)
            assert check(geo, [0] * nrec, some, -2)[0] == sum(1 for w in some if w)


def test_picked_markers_on_either_side_of_a_tile_edge():
    """an A on the last framed byte of a tile with its B on the first of the next, both being the picked markers: the empty
    match is match 1 of its string, k = 1 ends at its A and k = 2 starts at its B"""
    for geo in GEOS:
        T = tile(geo)
        for tiles in (1, 2):
            # framed: 3 bytes and '\n' of string 0; then string 1: p position bytes, A . B, then q bytes, A B — the last A at tiles * T - 1
            p = 10
            q = tiles * T - 1 - (4 + p + 3)
            l = p + 1 + q + 20
            spans = [[], [(p, p + 1), (p + 1 + q, p + 1 + q)]]
            assert frame([3, l], spans)[tiles * T - 1:tiles * T + 1] == b"\x01\x02"
            assert check(geo, [3, l], spans, 1, src_mis=4) == (2 - 1, q)
            assert check(geo, [3, l], spans, 2, dst_mis=7) == (1, 20)
            assert check(geo, [3, l], spans, -1) == (2, 23)
            assert check(geo, [3, l], spans, -2, src_mis=15, dst_mis=15) == (1, q)


def test_who_stores_which_bound():
    """kk = 0 (lo by the init pass), kk = c (hi by the init pass), both, neither, and absent: between them the two passes store
    every lo and hi exactly once (the shim counts the stores and refuses a second one)"""
    rng = random.Random(192)
    for geo in GEOS:
        T = tile(geo)
        lens = [rng.choice((0, 1, 4, 30, T // 3)) for _ in range(40)]
        spans = [draw(rng, l, 3) for l in lens]
        for k in (0, 1, 2, 3, -1, -2, -3, 7, -7):
            check(geo, lens, spans, k, src_mis=rng.randrange(16), dst_mis=rng.randrange(16))


def test_every_source_and_destination_misalignment():
    rng = random.Random(193)
    for geo in (0, 2):
        T = tile(geo)
        lens = chop(rng, T + 200, 50)
        spans = [draw(rng, l) for l in lens]
        for src_mis in range(16):
            for dst_mis in range(16):
                check(geo, lens, spans, (0, 1, -1, -2)[(src_mis + dst_mis) % 4], src_mis=src_mis, dst_mis=dst_mis)
    T = tile(3)
    lens = chop(rng, 2 * T + 200, 300)
    spans = [draw(rng, l, 9) for l in lens]
    for mis in range(16):
        check(3, lens, spans, 1, src_mis=mis, dst_mis=(mis * 11 + 5) % 16)
        check(3, lens, spans, -1, src_mis=(mis * 3) % 16, dst_mis=mis)


def test_output_lengths():
    """0, 1, 15, 16, 17 and 33 bytes out of two tiles, at every destination misalignment: one field, and m 1-byte fields"""
    for geo in (0, 3):
        T = tile(geo)
        for m in (0, 1, 15, 16, 17, 33):
            for dst_mis in range(16):
                assert check(geo, [T - 5, m + 40, T], [[], around(20, 20 + m), []], 1, dst_mis=dst_mis, src_mis=dst_mis ^ 5) == (1, m)
                if m:
                    lens = [T - 5] + [3] * m + [T]
                    spans = [[]] + [around(1, 2)] * m + [[]]
                    assert check(geo, lens, spans, 1, dst_mis=dst_mis) == (m, m)


def test_bases_and_ranks_beyond_32_bits():
    """positions, match ranks and output offsets as if a long column came before"""
    rng = random.Random(194)
    for geo in GEOS:
        T = tile(geo)
        for n in (T + 1, 2 * T + 5):
            lens = [3] + chop(rng, n - 3, 70)
            spans = [draw(rng, l) for l in lens]
            for k in (0, 1, -1, -2, 5):
                check(geo, lens, spans, k, src_mis=rng.randrange(16), dst_mis=rng.randrange(16), **far(T))
        check(geo, [4, 3 * T, 1], [[], around(T - 1, 2 * T + 1), []], 1, **far(T))
        check(geo, [4, 3 * T, 1], [[(1, 2)], [], [(0, 1)]], -1, src_mis=9, dst_mis=3, **far(T))


def test_stand_alone_program_under_sanitizers():
    """field_shim.cpp with its own main, built with -fsanitize=address,undefined, over generated lengths, columns, k from both
    ends and out of range, misalignments and the shift beyond 2^32: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("field")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
