"""The per-thread bodies of k_filter_part, k_filter_count and k_filter_emit (trre_amd/csrc/records_block.hpp: filter_part,
filter_count_strings, filter_mark, filter_seg_kept, filter_emit_rows, filter_emit_vecs) run on the host by tests/filter_shim.cpp
against numpy.  String i is kept exactly when (list_off[i + 1] > list_off[i]) != invert; the kept strings' bytes leave in input
order, kept string r starts at out_off[r] and was row rows[r]; out_off[0] is stored by tile 0 alone, every other byte and word
once, and nothing behind out_len, n_kept + 1 and n_kept."""
import ctypes
import random

import numpy as np

import column_shim_lib

GEOS = (0, 1, 2, 3)
UNSTORED = np.int64(-0x1111111111111112)          # 0xEEEE... as a signed word
FAR = dict(rr0=(1 << 33) + 7, rk0=(1 << 34) + 11)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("filter")
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.shim_filter_tile.argtypes = [i32]
        L.shim_filter_tile.restype = i64
        L.shim_filter.argtypes = [i32, vp, i64, vp, vp, i64, i32, i32, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_filter_tile(geo)


def far_pos(T):
    return ((5 << 32) // T + 3) * T


def check(geo, lens, hits, invert=False, src_mis=0, dst_mis=0, pos0=0, rr0=0, rk0=0, seed=1):
    """the shim against numpy on one column: string i has lens[i] random letters and is a hit (has a match) when hits[i].
    Returns (n_kept, out_len)"""
    lens, hits = np.asarray(lens, dtype=np.int64), np.asarray(hits, dtype=bool)
    nrec, n = len(lens), int(lens.sum())
    assert nrec >= 1 and len(hits) == nrec and not (pos0 and lens[0] == 0)
    off = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    rs = np.random.RandomState(seed)
    src = rs.randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8)
    loff = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.where(hits, rs.randint(1, 4, size=nrec), 0), out=loff[1:])
    kept = hits != bool(invert)
    want_rows = np.flatnonzero(kept).astype(np.int64)
    n_kept = len(want_rows)
    want_off = np.zeros(n_kept + 1, dtype=np.int64)
    np.cumsum(lens[kept], out=want_off[1:])
    out_len = int(want_off[-1])
    want_out = src[np.repeat(kept, lens)]
    assert len(want_out) == out_len
    out = np.full(out_len + 1, 0x11, dtype=np.uint8)
    oo = np.full(n_kept + 2, -5, dtype=np.int64)
    rows = np.full(n_kept + 1, -5, dtype=np.int64)
    totals, stores = np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.int64)
    shifted = off + pos0
    rc = lib().shim_filter(geo, src.ctypes.data if n else None, n, shifted.ctypes.data, loff.ctypes.data, nrec, int(invert), src_mis, dst_mis, pos0, rr0,
                           rk0, n_kept, out_len, out.ctypes.data, oo.ctypes.data, rows.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, n, nrec, n_kept, out_len, invert, src_mis, dst_mis, pos0)
    assert rc == 0, (rc,) + label
    assert totals.tolist() == [n_kept, out_len], (label, totals)
    assert np.array_equal(out[:out_len], want_out), label
    assert np.array_equal(oo[1:n_kept + 1], want_off[1:] + rk0), label
    assert oo[0] == (UNSTORED if pos0 else 0), label
    assert np.array_equal(rows[:n_kept], want_rows), label
    assert out[out_len] == 0x11 and oo[n_kept + 1] == -5 and rows[n_kept] == -5, label          # nothing behind the ends
    assert stores.tolist() == [out_len, n_kept + (0 if pos0 else 1), n_kept], (label, stores)   # every byte and word once
    if n_kept == nrec and not pos0 and not rk0:
        assert np.array_equal(out[:out_len], src) and np.array_equal(oo[:nrec + 1], off), label  # everything kept: out == in
    return n_kept, out_len


def chop(rng, n, longest):
    """string lengths that add up to n, empty ones among them"""
    lens = []
    while sum(lens) < n:
        lens.append(min(rng.choice((0, 0, 1, 2, 3, 7, 16, longest)), n - sum(lens)))
    return lens or [0]


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_by_hand():
    """[ab] kept, [] dropped, [cde] dropped, [f] kept"""
    assert check(0, [2, 0, 3, 1], [1, 0, 0, 1]) == (2, 3)
    assert check(0, [2, 0, 3, 1], [1, 0, 0, 1], invert=True) == (2, 3)
    assert check(0, [0], [1]) == (1, 0) and check(0, [0], [0]) == (0, 0)


def test_lengths_around_the_tile_edges():
    """input lengths 0, 1, 15, 16, 17, T - 1, T, T + 1 and 3 T: one string, random strings; nothing kept, everything kept (out ==
    in, out_off == off), a random half"""
    rng = random.Random(91)
    for geo in GEOS:
        T = tile(geo)
        for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T):
            for lens in ([n], chop(rng, n, 40), chop(rng, n, T // 2 + 3)):
                k = len(lens)
                for hits in ([0] * k, [1] * k, [rng.randrange(2) for _ in range(k)]):
                    for invert in (False, True):
                        check(geo, lens, hits, invert, src_mis=rng.randrange(16), dst_mis=rng.randrange(16), seed=n + 1)


def test_one_byte_strings_kept_and_dropped_in_turn():
    """over 2 T bytes: every destination vector has 16 sources"""
    for geo in GEOS:
        T = tile(geo)
        for first in (0, 1):
            hits = [(i + first) & 1 for i in range(2 * T)]
            assert check(geo, [1] * (2 * T), hits, src_mis=3 * geo, dst_mis=5 + geo) == (T, T)
            assert check(geo, [1] * (2 * T), hits, invert=True, src_mis=1, dst_mis=0) == (T, T)


def test_empty_strings_between_non_empty_ones():
    """empty kept strings between dropped non-empty ones (two toggles in one place), and the reverse"""
    for geo in GEOS:
        T = tile(geo)
        k = (2 * T + 9) // 3
        lens = [0, 3] * k + [0]
        hits = [1, 0] * k + [1]
        assert check(geo, lens, hits, src_mis=7) == (k + 1, 0)
        assert check(geo, lens, hits, invert=True, dst_mis=9) == (k, 3 * k)
        lens = [0, 0, 5, 0] * (k // 2)
        hits = [1, 0, 1, 1] * (k // 2)
        check(geo, lens, hits, src_mis=15, dst_mis=15)
        check(geo, lens, hits, invert=True, src_mis=15, dst_mis=1)


def test_strings_over_three_tiles():
    """a kept string over three tiles between dropped neighbours; a dropped one between two kept 1-byte strings: its tiles
    store nothing, and the two bytes are all that is stored"""
    for geo in GEOS:
        T = tile(geo)
        for long in (3 * T, 3 * T + 5, 4 * T - 1):
            for mis in (0, 1, 15):
                assert check(geo, [7, long, 9], [0, 1, 0], src_mis=mis, dst_mis=(mis * 7) % 16) == (1, long)
                assert check(geo, [1, long, 1], [1, 0, 1], src_mis=mis, dst_mis=(mis * 5) % 16) == (2, 2)
                assert check(geo, [T // 2, long, 1], [1, 0, 1], invert=True, src_mis=mis) == (1, long)


def test_string_ends_at_the_tile_edges():
    """ends at T - 1, T and T + 1 of the v-space, at every source misalignment: kept then dropped, dropped then kept, and an
    empty string on the edge"""
    for geo in (0, 1, 2):
        T = tile(geo)
        for mis in range(16):
            for end in (T - 1, T, T + 1):
                first = end - mis
                for hits in ([1, 0, 1], [0, 1, 0], [1, 1, 0]):
                    check(geo, [first, T, 3], hits, src_mis=mis, dst_mis=(mis + end) % 16)
                    check(geo, [first, 0, T], hits, src_mis=mis, dst_mis=(mis + 3) % 16)


def test_all_strings_empty():
    """n = 0, nrec = 1, 64, 65 and 70 000: one tile, no byte, every row in order"""
    for geo in GEOS:
        for nrec in (1, 64, 65, 70000):
            assert check(geo, [0] * nrec, [1] * nrec) == (nrec, 0)
            assert check(geo, [0] * nrec, [1] * nrec, invert=True) == (0, 0)
            hits = [(i * 7) % 3 == 0 for i in range(nrec)]
            assert check(geo, [0] * nrec, hits, src_mis=geo + 1)[0] == sum(hits)


def test_every_source_and_destination_misalignment():
    rng = random.Random(92)
    for geo in (0, 2):
        T = tile(geo)
        lens = chop(rng, T + 200, 50)
        hits = [rng.randrange(3) > 0 for _ in lens]
        for src_mis in range(16):
            for dst_mis in range(16):
                check(geo, lens, hits, src_mis=src_mis, dst_mis=dst_mis)
    T = tile(3)
    lens = chop(rng, 2 * T + 200, 300)
    hits = [rng.randrange(3) > 0 for _ in lens]
    for mis in range(16):
        check(3, lens, hits, src_mis=mis, dst_mis=(mis * 11 + 5) % 16)
        check(3, lens, hits, invert=True, src_mis=(mis * 3) % 16, dst_mis=mis)


def test_output_lengths():
    """0, 1, 15, 16, 17 and 33 bytes kept out of two tiles, at every destination misalignment"""
    for geo in (0, 3):
        T = tile(geo)
        for m in (0, 1, 15, 16, 17, 33):
            for dst_mis in range(16):
                lens = [T - 5, m, T]
                assert check(geo, lens, [0, 1, 0], dst_mis=dst_mis, src_mis=dst_mis ^ 5) == (1, m)
                if m:
                    assert check(geo, [T - 5] + [1] * m + [T], [0] + [1] * m + [0], dst_mis=dst_mis) == (m, m)


def test_bases_and_ranks_beyond_32_bits():
    """positions and ranks as if 5 * 2^32 input bytes holding 2^33 + 7 kept strings and 2^34 + 11 kept bytes came before"""
    rng = random.Random(93)
    for geo in GEOS:
        T = tile(geo)
        for n in (T + 1, 2 * T + 5):
            lens = [3] + chop(rng, n - 3, 70)
            hits = [rng.randrange(2) for _ in lens]
            for invert in (False, True):
                check(geo, lens, hits, invert, src_mis=rng.randrange(16), dst_mis=rng.randrange(16), pos0=far_pos(T), **FAR)
        check(geo, [1, 3 * T, 1], [1, 0, 1], pos0=far_pos(T), **FAR)
        check(geo, [1, 3 * T, 1], [0, 1, 0], src_mis=9, dst_mis=3, pos0=far_pos(T), **FAR)


def test_stand_alone_program_under_sanitizers():
    """filter_shim.cpp with its own main, built with -fsanitize=address,undefined, over the same lengths, columns, misalignments,
    both senses and the shift beyond 2^32: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("filter")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
