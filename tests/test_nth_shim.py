"""The per-thread bodies of k_nth_plan, k_nth_offsets and k_nth_emit (trre_amd/csrc/records_block.hpp: nth_plan,
nth_offsets_sum, nth_offsets_thread, nth_emit_window, nth_keep_window, nth_emit_vecs) run on the host by tests/nth_shim.cpp
against tests/nth_lib.py's expect() on lists made by hand, so every edge can be placed: what the find call's two scans and
k_find_unframe would leave (the list offsets, the texts and their offsets) is written out from the lists.  Checked: the two
totals of the plan pass; the output's bytes, offsets and bitmap; every byte of out, every word of out_off, of the bitmap and of
the parked sources stored exactly once, nothing behind out_len, nrec + 1 and the bitmap's last word."""
import ctypes
import random

import numpy as np

import column_shim_lib
import nth_lib

GEOS = (0, 1, 2, 3)
KS = (0, 1, 2, -1, -2, 5, -(1 << 63), (1 << 63) - 1)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("nth")
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        for f in (L.shim_nth_tile, L.shim_nth_chunk):
            f.argtypes = [i32]
            f.restype = i64
        L.shim_nth_window.restype = i64
        L.shim_nth.argtypes = [i32, vp, i64, vp, vp, i64, i64, i32, i32, i64, i64, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_nth_tile(geo)


def chunk(geo):
    return lib().shim_nth_chunk(geo)


def check(geo, lists, k, x_mis=0, dst_mis=0):
    """the shim against nth_lib.expect() on one column's lists.  Returns (n_valid, out_len)"""
    nrec = len(lists)
    assert nrec >= 1
    loff = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(l) for l in lists], dtype=np.int64), out=loff[1:])
    flat = [t for l in lists for t in l]
    found = len(flat)
    xoff = np.zeros(found + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(t) for t in flat], dtype=np.int64), out=xoff[1:])
    x = np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8)
    assert 0xEE not in x
    want, want_off, want_valid = nth_lib.expect(lists, k)
    out_len, n_valid, nw = len(want), sum(want_valid), (nrec + 63) // 64
    out = np.full(out_len + 1, 0x11, dtype=np.uint8)
    oo = np.full(nrec + 2, -5, dtype=np.int64)
    valid = np.full(nw + 1, 0x33, dtype=np.uint64)
    totals, stores = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64)
    rc = lib().shim_nth(geo, loff.ctypes.data, nrec, xoff.ctypes.data, x.ctypes.data, found, k, x_mis, dst_mis, n_valid, out_len, out.ctypes.data,
                        oo.ctypes.data, valid.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, nrec, found, k, n_valid, out_len, x_mis, dst_mis)
    assert rc == 0, (rc,) + label
    assert totals.tolist() == [n_valid, out_len], (label, totals)
    assert out[:out_len].tobytes() == want, label
    assert oo[:nrec + 1].tolist() == want_off, label
    assert valid[:nw].tobytes() == nth_lib.bitmap(want_valid), label
    assert out[out_len] == 0x11 and oo[nrec + 1] == -5 and valid[nw] == 0x33, label
    assert stores.tolist() == [out_len, nw, nrec, nrec + 1], (label, stores)             # every byte and word once
    return n_valid, out_len


def text(rng, n):
    return bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))


def random_lists(rng, nrec, longest=20, most=5):
    return [[text(rng, 0 if rng.randrange(3) == 0 else rng.randrange(longest)) for _ in range(rng.randrange(most))] for _ in range(nrec)]


def test_every_misalignment_of_output_and_source():
    """the output at every address mod 16 and the texts at every address mod 16, and — through preceding texts of 0 .. 15 bytes —
    the selected sources at every offset mod 16 whatever the buffer's own; every k"""
    rng = random.Random(401)
    for geo in GEOS:
        T = tile(geo)
        lists = random_lists(rng, 300, longest=60)
        for mis in range(16):
            for k in KS[:4] if mis else KS:
                check(geo, lists, k, x_mis=mis, dst_mis=(5 * mis + 3) % 16)
            check(geo, lists, 0, x_mis=0, dst_mis=mis)
            check(geo, lists, -1, x_mis=mis, dst_mis=0)
        # entries of 40 bytes whose sources start 0 .. 15 bytes behind an aligned one: the unselected text in front has that length
        for dst_mis in range(16):
            lists = [[text(rng, lead), text(rng, 40)] for lead in range(16)] * 3
            assert check(geo, lists, 1, dst_mis=dst_mis)[0] == 48
            assert check(geo, lists, -1, x_mis=dst_mis, dst_mis=(dst_mis * 7) % 16)[0] == 48
        assert T >= 1024


def test_string_counts_around_the_waves_and_the_chunks():
    """nrec of 1, 63, 64, 65 and of the plan chunk's size - 1, + 0, + 1, two chunks and 77: the bitmap's words and its tail, the
    offsets across the chunks' bases"""
    rng = random.Random(402)
    for geo in GEOS:
        C = chunk(geo)
        for nrec in (1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 77):
            lists = random_lists(rng, nrec)
            for k in KS:
                check(geo, lists, k, x_mis=rng.randrange(16), dst_mis=rng.randrange(16))
            assert check(geo, [[]] * nrec, 0) == (0, 0) and check(geo, [[]] * nrec, -1) == (0, 0)
            assert check(geo, [[b""]] * nrec, 0) == (nrec, 0)                            # valid and empty: no byte, every bit
            assert check(geo, [[b"y"]] * nrec, 0, dst_mis=5) == (nrec, nrec)
            assert check(geo, [[b"y"]] * nrec, 1) == (0, 0)


def test_output_tile_edges():
    """an entry of exactly one tile and of one tile and a byte between short neighbours; one entry over more than two tiles;
    entries that straddle the edge by 1 and by 15 bytes — with d_out aligned and misaligned (the edge lies at T - dst_mis then)"""
    rng = random.Random(403)
    for geo in GEOS:
        T = tile(geo)
        for dst_mis in (0, 1, 15):
            for n in (T, T + 1):
                lists = [[b"ab"], [text(rng, 3), text(rng, n)], [b"cd", b"e"], [], [text(rng, 5)]]
                assert check(geo, lists, -1, dst_mis=dst_mis, x_mis=3) == (4, 2 + n + 1 + 5)
                assert check(geo, lists, 1, dst_mis=dst_mis) == (2, n + 1)
            big = [[b"q"], [text(rng, 2 * T + T // 2 + 7)], [b"r"]]
            assert check(geo, big, 0, dst_mis=dst_mis, x_mis=9) == (3, 2 * T + T // 2 + 9)
            edge = T - dst_mis
            for over in (1, 15):
                lists = [[text(rng, edge - (20 - over))], [text(rng, 20)], [text(rng, 40)]]
                assert check(geo, lists, 0, dst_mis=dst_mis, x_mis=over)[1] == edge + over + 40
            # an empty entry exactly at the edge, valid and absent
            lists = [[text(rng, edge)], [b""], [], [text(rng, 33)]]
            assert check(geo, lists, 0, dst_mis=dst_mis) == (3, edge + 33)


def test_runs_of_empty_entries_at_one_position():
    """40 000 strings whose selected match is empty, then one with a 100-byte entry: 40 000 empty entries at output position 0,
    which cost one search and overflow the tile's image of offsets; the same run between two entries; all of them absent"""
    rng = random.Random(404)
    for geo in (0, 3):
        run = [[b"", b"zz"]] * 40000
        assert check(geo, run + [[text(rng, 100)]], 0) == (40001, 100)
        assert check(geo, [[text(rng, 30)]] + run + [[text(rng, 100)]], 0, dst_mis=11) == (40002, 130)
        assert check(geo, [[text(rng, 30)]] + run + [[text(rng, 100)]], 2, dst_mis=3) == (0, 0)
        assert check(geo, run + [[text(rng, 100), b"k"]], 1, x_mis=7) == (40001, 80001)
    assert 40000 > lib().shim_nth_window()


def test_a_window_larger_than_the_image():
    """one-byte entries: a tile of the device's geometry touches more entries than its image of offsets holds (the search goes
    to memory), a tile of the small ones does not; three-byte entries next to absent ones"""
    rng = random.Random(405)
    for geo in GEOS:
        T = tile(geo)
        n = 2 * T + 11
        assert check(geo, [[text(rng, 1)] for _ in range(n)], 0, dst_mis=geo) == (n, n)
        assert check(geo, [[text(rng, 3)] if i & 1 else [] for i in range(n)], -1, x_mis=5) == (n // 2, 3 * (n // 2))
    assert tile(3) > lib().shim_nth_window() > tile(0)                                   # both sides of the image's size ran


def test_k_from_either_end():
    """k = -1 on strings with 0, 1 and many matches; k beyond either end; INT64_MIN and INT64_MAX select nothing"""
    lists = [[], [b"one"], [b"a", b"bb", b"ccc", b"dddd", b"eeeee", b"ffffff"], [b"", b""], []]
    for geo in GEOS:
        assert check(geo, lists, -1) == (3, 3 + 6)
        assert check(geo, lists, -2) == (2, 5)
        assert check(geo, lists, -6) == (1, 1) and check(geo, lists, -7) == (0, 0)
        assert check(geo, lists, 5) == (1, 6) and check(geo, lists, 6) == (0, 0)
        assert check(geo, lists, -(1 << 63)) == (0, 0) and check(geo, lists, (1 << 63) - 1) == (0, 0)


def test_sanitized_program():
    """the same entry point over generated shapes as a stand-alone program under -fsanitize=address,undefined: a process of its
    own on the CPU"""
    done = column_shim_lib.sanitized("nth")
    assert done.returncode == 0 and b"shapes ok" in done.stdout, (done.stdout[-400:], done.stderr[-2000:])
