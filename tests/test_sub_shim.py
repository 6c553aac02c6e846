"""The per-thread bodies of k_sub_plan, k_sub_place, k_sub_offsets and k_sub_emit (trre_amd/csrc/records_block.hpp:
sub_plan_thread, sub_place_sums, sub_place_thread, sub_offset, sub_emit_window, sub_keep_window, sub_emit_vecs) run on the host
by tests/sub_shim.cpp against a composition written here.  A column is strings of given lengths with ordered, disjoint spans and
texts drawn in the test, so every edge can be placed: what k_span_emit and k_find_unframe would leave (starts, ends, list
offsets, the texts and their offsets) is written out from them.  Checked: the three totals of the plan pass; the output's bytes
and offsets; every byte of out and every word of out_off stored exactly once, nothing behind out_len and nrec + 1."""
import ctypes
import random

import numpy as np

import column_shim_lib

GEOS = (0, 1, 2, 3)
SELECTIONS = [(0, -1), (0, 1), (1, 1), (2, -1), (0, 0), (5, 2), ((1 << 63) - 1, 1), (0, -(1 << 63))]

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("sub")
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.shim_sub_tile.argtypes = [i32]
        L.shim_sub_tile.restype = i64
        L.shim_sub_window.restype = i64
        L.shim_sub.argtypes = [i32, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_sub_tile(geo)


def selected(r, first, count):
    return first <= r and (count < 0 or r - first < count)


def compose(src, lens, spans, texts, first, count):
    """(the outputs concatenated, their offsets, the selected matches): spans relative to their string, texts per match"""
    out, off, at, n_sel = [], [0], 0, 0
    total = 0
    for l, w, x in zip(lens, spans, texts):
        s0, p = at, at
        for r, ((s, e), t) in enumerate(zip(w, x)):
            assert p - s0 <= s <= e <= l, (l, w)
            if selected(r, first, count):
                out.append(src[p:s0 + s])
                out.append(t)
                total += s0 + s - p + len(t)
                p = s0 + e
                n_sel += 1
        out.append(src[p:s0 + l])
        total += s0 + l - p
        at += l
        off.append(total)
    return b"".join(out), off, n_sel


FAR = dict(pos0=(5 << 32) + 3, ra0=1024 << 23, rk0=(1 << 34) + 11)      # as if so many bytes, matches and output bytes came before


def check(geo, lens, spans, texts, first, count, src_mis=0, x_mis=0, dst_mis=0, seed=1, pos0=0, ra0=0, rk0=0):
    """the shim against compose() on one column.  Returns (n_sel, out_len)"""
    nrec, n = len(lens), int(sum(lens))
    assert nrec >= 1 and len(spans) == nrec == len(texts)
    off = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    loff = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(w) for w in spans], dtype=np.int64), out=loff[1:])
    found = int(loff[-1])
    src = np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8).tobytes()
    start = np.asarray([off[i] + s for i, w in enumerate(spans) for s, _ in w] + [0], dtype=np.int64)
    end = np.asarray([off[i] + e for i, w in enumerate(spans) for _, e in w] + [0], dtype=np.int64)
    flat = [t for x in texts for t in x]
    assert len(flat) == found
    xoff = np.zeros(found + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(t) for t in flat], dtype=np.int64), out=xoff[1:])
    x = np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8)
    want, want_off, n_sel = compose(src, lens, spans, texts, first, count)
    out_len = len(want)
    out = np.full(out_len + 1, 0x11, dtype=np.uint8)
    oo = np.full(nrec + 2, -5, dtype=np.int64)
    totals, stores = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int64)
    sbuf = np.frombuffer(src + b"\0", dtype=np.uint8)
    so, sl, ss, se = off + pos0, loff + ra0, start + pos0, end + pos0
    rc = lib().shim_sub(geo, sbuf.ctypes.data, n, so.ctypes.data, sl.ctypes.data, nrec, ss.ctypes.data, se.ctypes.data, xoff.ctypes.data,
                        x.ctypes.data, found, first, count, src_mis, x_mis, dst_mis, pos0, ra0, rk0, n_sel, out_len, out.ctypes.data, oo.ctypes.data,
                        totals.ctypes.data, stores.ctypes.data)
    label = (geo, n, nrec, found, first, count, n_sel, out_len, src_mis, x_mis, dst_mis, pos0)
    assert rc == 0, (rc,) + label
    assert totals[0] == n_sel and n - totals[2] + totals[1] == out_len, (label, totals)
    assert out[:out_len].tobytes() == want, label
    assert oo[:nrec + 1].tolist() == [w + rk0 for w in want_off], label
    assert out[out_len] == 0x11 and oo[nrec + 1] == -5, label
    assert stores.tolist() == [out_len, nrec + 1], (label, stores)                       # every byte and word once
    return n_sel, out_len


def text(rng, k):
    return bytes(rng.choice(b"ABCDEFGHIJ") for _ in range(k))


def one_string(n, spans, texts):
    return [n], [spans], [texts]


def random_column(rng, n, dense=True):
    """strings that add up to n bytes, with matches of 0 .. 3 bytes and texts of 0 .. 19 drawn among them"""
    lens, spans, texts, left = [], [], [], n
    while True:
        l = min(left, 0 if rng.randrange(4) == 0 else rng.randrange(60))
        w, x, p = [], [], 0
        while rng.randrange(8 if dense else 2):
            s = p + rng.randrange(3 if dense else 40)
            if s > l:
                break
            e = min(l, s + rng.randrange(4))
            w.append((s, e))
            x.append(text(rng, 0 if rng.randrange(3) == 0 else rng.randrange(20)))
            p = e
        lens.append(l); spans.append(w); texts.append(x)
        left -= l
        if left == 0 and rng.randrange(3):
            return lens, spans, texts


def test_output_lengths_and_every_misalignment():
    """output lengths 0, 1, 15, 16, 17, T - 1, T, T + 1, 3 T: one string whose one selected match makes up the difference to the
    input; then random columns at every source, text and destination misalignment under every selection"""
    rng = random.Random(301)
    for geo in GEOS:
        T = tile(geo)
        for want_len in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T):
            for n, t in ((want_len + 5, 0), (max(want_len - 3, 0), want_len - max(want_len - 3, 0)), (0, want_len)):
                s = min(2, n, want_len - t)
                e = n - (want_len - t - s)                                              # in[:s] + text + in[e:]
                assert 0 <= s <= e <= n and s + t + n - e == want_len, (want_len, n, t)
                got = check(geo, *one_string(n, [(s, e)], [text(rng, t)]), 0, -1, src_mis=rng.randrange(16), x_mis=rng.randrange(16),
                            dst_mis=rng.randrange(16))
                assert got == (1, want_len)
    for geo in GEOS:
        T = tile(geo)
        for mis in range(16):
            col = random_column(rng, 2 * T + 37 + mis, dense=bool(mis & 1))
            for k, (first, count) in enumerate(SELECTIONS):
                check(geo, *col, first, count, src_mis=mis, x_mis=(3 * mis + k) % 16, dst_mis=(mis + 5 * k) % 16, seed=mis)
            check(geo, *col, 0, -1, src_mis=0, x_mis=0, dst_mis=mis)
            check(geo, *col, 0, -1, src_mis=mis, x_mis=mis, dst_mis=0)


def test_tile_edges():
    """a text that straddles an output tile edge by 1 and by 15 bytes; a gap that does; a selected empty text exactly at the edge;
    an unselected match across the edge — with d_out aligned and misaligned (the edge lies at T - dst_mis then)"""
    rng = random.Random(302)
    for geo in GEOS:
        T = tile(geo)
        for dst_mis in (0, 1, 15):
            edge = T - dst_mis
            for over in (1, 15):
                # the text [edge - (20 - over) .. edge + over): 20 bytes, `over` of them behind the edge
                s = edge - (20 - over)
                check(geo, *one_string(2 * T, [(s, s + 3)], [text(rng, 20)]), 0, -1, dst_mis=dst_mis, src_mis=over)
                # a gap of 20 between two deleted matches, `over` of its bytes behind the edge
                check(geo, *one_string(2 * T, [(0, 5), (5 + s, 5 + s + 4), (5 + s + 24, 5 + s + 30)], [b"", b"", b""]), 0, -1, dst_mis=dst_mis)
            # an empty selected text exactly at the edge: between two gaps, and between two texts
            check(geo, *one_string(2 * T, [(edge, edge + 2)], [b""]), 0, -1, dst_mis=dst_mis)
            check(geo, *one_string(2 * T, [(edge - 4, edge - 4), (edge - 4, edge - 4), (edge - 4, edge - 2)], [b"WXYZ", b"", b"Q"]), 0, -1,
                  dst_mis=dst_mis)
            # unselected matches between selected ones, one of them across the edge
            w = [(edge - 40, edge - 30), (edge - 5, edge + 5), (edge + 20, edge + 22), (edge + 30, edge + 31)]
            for first, count in ((0, 1), (2, 1), (1, 1), (3, -1), (0, -1), (1, 2)):
                check(geo, *one_string(2 * T, w, [b"one", b"", b"three33", b"4"]), first, count, dst_mis=dst_mis)


def test_runs_of_matches_at_one_position():
    """40 000 adjacent one-byte matches, all selected with empty texts: 40 000 empty segments at output position 0 and an empty
    output; none selected: out == in; the second half selected; the same run between two gaps; 40 000 empty matches at one input
    position with empty texts, and with one text among them"""
    for geo in (0, 3):
        run = [(k, k + 1) for k in range(40000)]
        none = [b""] * 40000
        assert check(geo, *one_string(40000, run, none), 0, -1) == (40000, 0)
        assert check(geo, *one_string(40000, run, none), 0, 0) == (0, 40000)
        assert check(geo, *one_string(40000, run, none), 20000, -1, dst_mis=3) == (20000, 20000)
        assert check(geo, *one_string(40100, [(s + 50, e + 50) for s, e in run], none), 0, -1, dst_mis=9) == (40000, 100)
        same = [(7, 7)] * 40000
        assert check(geo, *one_string(20, same, none), 0, -1) == (40000, 20)
        assert check(geo, *one_string(20, same, [b""] * 39999 + [b"mark"]), 0, -1, dst_mis=14) == (40000, 24)
        assert check(geo, *one_string(20, same, [b"mark"] + [b""] * 39999), 0, -1) == (40000, 24)


def test_growth_and_a_window_larger_than_the_image():
    """every byte a match with a three-byte text: the output is three times the input over several tiles, and a tile of the device's
    geometry touches more segments than its image of places holds (the search goes to memory); every other byte deleted"""
    rng = random.Random(303)
    for geo in GEOS:
        T = tile(geo)
        n = 2 * T + 11
        run = [(k, k + 1) for k in range(n)]
        assert check(geo, *one_string(n, run, [text(rng, 3) for _ in range(n)]), 0, -1, dst_mis=geo) == (n, 3 * n)
        assert check(geo, *one_string(n, run, [text(rng, k & 1) for k in range(n)]), 0, -1, src_mis=5) == (n, n // 2)
        assert check(geo, *one_string(n, run, [text(rng, 1) for _ in range(n)]), 7, -1, dst_mis=11) == (n - 7, n)
    assert tile(3) > lib().shim_sub_window() and 3 * lib().shim_sub_window() > tile(0)       # both sides of the image's size ran


def test_strings_without_matches_and_empty_strings():
    """strings without matches before, between and behind strings with matches; all strings empty, nrec 1, 63, 64, 65 and
    70 000, with a match each (a text each: nrec bytes) and without"""
    rng = random.Random(304)
    for geo in GEOS:
        lens = [5, 0, 9, 0, 0, 30, 4, 0, 12, 0, 0]
        spans = [[], [], [(2, 4)], [], [], [(0, 0), (3, 9), (30, 30)], [], [], [(1, 2), (2, 3), (3, 3)], [], []]
        texts = [[text(rng, 1 + len(w) + k) for k in range(len(w))] for w in spans]
        for first, count in SELECTIONS:
            check(geo, lens, spans, texts, first, count, src_mis=geo, dst_mis=2 * geo + 1)
    for nrec in (1, 63, 64, 65, 70000):
        for geo in ((0, 3) if nrec == 70000 else GEOS):
            assert check(geo, [0] * nrec, [[]] * nrec, [[]] * nrec, 0, -1) == (0, 0)
            assert check(geo, [0] * nrec, [[(0, 0)]] * nrec, [[b"y"]] * nrec, 0, 1, dst_mis=5) == (nrec, nrec)
            assert check(geo, [0] * nrec, [[(0, 0)]] * nrec, [[b"y"]] * nrec, 1, 1) == (0, 0)


def test_beyond_2_to_the_32():
    """positions, match ranks and output offsets beyond 2^32, through shifted pointers: random columns, the run of 40 000 matches
    and the growth over several tiles again, as if a long column came before"""
    rng = random.Random(305)
    for geo in GEOS:
        T = tile(geo)
        for k, (first, count) in enumerate(SELECTIONS):
            col = random_column(rng, 2 * T + 41 + k, dense=bool(k & 1))
            check(geo, *col, first, count, src_mis=k, x_mis=2 * k, dst_mis=15 - k, seed=k, **FAR)
        n = 2 * T + 11
        run = [(j, j + 1) for j in range(n)]
        assert check(geo, *one_string(n, run, [text(rng, 3) for _ in range(n)]), 0, -1, dst_mis=geo, **FAR) == (n, 3 * n)
        assert check(geo, *one_string(n, run, [b""] * n), 0, -1, **FAR) == (n, 0)
        assert check(geo, *one_string(n, run, [b""] * n), 5, -1, dst_mis=7, **FAR) == (n - 5, 5)
        assert check(geo, [0] * 65, [[(0, 0)]] * 65, [[b"y"]] * 65, 0, 1, **FAR) == (65, 65)


def test_sanitized_program():
    """the same entry point over generated shapes as a stand-alone program under -fsanitize=address,undefined: a process of its
    own on the CPU"""
    done = column_shim_lib.sanitized("sub")
    assert done.returncode == 0 and b"shapes ok" in done.stdout, (done.stdout[-400:], done.stderr[-2000:])
