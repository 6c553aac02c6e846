"""The per-thread bodies of k_trim_pick and k_trim_bounds (trre_amd/csrc/records_block.hpp: trim_pick_markers, trim_bounds, and
the span bodies they reuse), followed by the field call's count and emit bodies with k = 0, run on the host by tests/trim_shim.cpp
against tests/trim_lib.py.  A column is strings of given lengths with ordered, disjoint spans drawn here; the span call's list
offsets and framed text are written out from them (tests/test_field_shim.py's frame), so every string's range is known before the
shim runs.  Checked: each of the six parked words — where matches 0, c - 1 and c - 2 start and end — stored exactly once where the
match exists and its side is asked for, and not at all otherwise; lo, hi, begin and end of every string, each stored once; the
entries' bytes in input order; out_off, entry 0 by tile 0 alone and every other byte and word once; nothing behind out_len and
nrec + 1."""
import ctypes
import random

import numpy as np

import column_shim_lib
import trim_lib
from test_field_shim import UNSTORED, chop, far, frame
from trim_lib import BOTH, LEFT, RIGHT

GEOS = (0, 1, 2, 3)
SIDES = (LEFT, RIGHT, BOTH)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("trim")
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.shim_trim_tile.argtypes = [i32]
        L.shim_trim_tile.restype = i64
        L.shim_trim.argtypes = [i32, vp, i64, vp, vp, i64, ctypes.c_uint32, vp, i64, i32, i32, i64, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp,
                                vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_trim_tile(geo)


def parked(off, spans, flags):
    """the six parked words [6][nrec] the pick pass must leave (UNSTORED: nobody stores it), and how many of each"""
    nrec = len(spans)
    want = np.full((6, nrec), UNSTORED, dtype=np.int64)
    for i, w in enumerate(spans):
        for role, j, side in ((0, 0, LEFT), (1, len(w) - 1, RIGHT), (2, len(w) - 2, RIGHT)):
            if 0 <= j < len(w) and flags & side:
                want[2 * role, i], want[2 * role + 1, i] = off[i] + w[j][0], off[i] + w[j][1]
    return want, (want != UNSTORED).sum(axis=1).tolist()


def check(geo, lens, spans, flags, views=True, src_mis=0, dst_mis=0, pos0=0, ra0=0, rk0=0, seed=1, nul_at=()):
    """the shim against trim_lib on one column; nul_at: positions of the column that hold a NUL (the spans drawn must end at or
    before their string's first).  Returns out_len"""
    nrec, n = len(lens), int(sum(lens))
    assert nrec >= 1 and len(spans) == nrec and not (pos0 and lens[0] == 0)
    off = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    loff = np.zeros(nrec + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(w) for w in spans], dtype=np.int64), out=loff[1:])
    src = np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8)
    for at in nul_at:
        src[at] = 0
    data = src.tobytes()
    lines = [data[off[i]:off[i + 1]] for i in range(nrec)]
    for l, w in zip(lines, spans):
        assert all(e <= (l.find(b"\0") if b"\0" in l else len(l)) for _, e in w), (l, w)
    framed = np.frombuffer(frame(lens, spans), dtype=np.uint8)
    want_out, want_off, want_begin, want_end = trim_lib.expect(lines, spans, flags)
    want_off, want_begin, want_end = (np.asarray(x, dtype=np.int64) for x in (want_off, want_begin, want_end))
    out_len = len(want_out)
    want_marks, want_parked = parked(off + pos0, spans, flags)
    out = np.full(out_len + 1, 0x11, dtype=np.uint8)
    oo = np.full(nrec + 2, -5, dtype=np.int64)
    glo, ghi, gb, ge = (np.full(nrec + 1, -5, dtype=np.int64) for _ in range(4))
    marks = np.full(6 * nrec + 1, -5, dtype=np.int64)
    totals, stores = np.zeros(2, dtype=np.int64), np.zeros(12, dtype=np.int64)
    so, sl = off + pos0, loff + ra0
    rc = lib().shim_trim(geo, src.ctypes.data if n else None, n, so.ctypes.data, sl.ctypes.data, nrec, flags, framed.ctypes.data, len(framed),
                         src_mis, dst_mis, pos0, ra0, rk0, out_len, int(views), out.ctypes.data, oo.ctypes.data, glo.ctypes.data, ghi.ctypes.data,
                         gb.ctypes.data, ge.ctypes.data, marks.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, n, nrec, flags, out_len, src_mis, dst_mis, pos0)
    assert np.array_equal(marks[:6 * nrec].reshape(6, nrec), want_marks) or rc in (3, 6), (rc, label)
    assert rc == 0, (rc,) + label
    assert np.array_equal(glo[:nrec], want_begin + pos0) and np.array_equal(ghi[:nrec], want_end + pos0), label
    if views:
        assert np.array_equal(gb[:nrec], want_begin + pos0) and np.array_equal(ge[:nrec], want_end + pos0), label
    else:
        assert (gb[:nrec] == UNSTORED).all() and (ge[:nrec] == UNSTORED).all(), label
    assert totals.tolist() == [nrec, out_len], (label, totals)
    assert out[:out_len].tobytes() == want_out, label
    assert np.array_equal(oo[1:nrec + 1], want_off[1:] + rk0), label
    assert oo[0] == (UNSTORED if pos0 else 0), label
    assert out[out_len] == 0x11 and oo[nrec + 1] == -5 and marks[6 * nrec] == -5, label
    assert all(g[nrec] == -5 for g in (glo, ghi, gb, ge)), label
    v = nrec if views else 0
    assert stores.tolist() == [out_len, nrec + (0 if pos0 else 1), nrec, nrec, v, v] + want_parked, (label, stores)    # every byte and word once
    if not any(spans) and not pos0 and not rk0:
        assert out[:out_len].tobytes() == data and np.array_equal(oo[:nrec + 1], off), label   # nothing to trim: every entry its whole string
    return out_len


def draw(rng, l, density=4):
    """ordered, disjoint spans in a string of l bytes: empty ones among them, never two at one place but for the empty tail
    attempt behind a non-empty match that ends at the string's end"""
    w, x = [], 0
    while x <= l:
        if rng.randrange(density) == 0:
            e = min(x + rng.choice((0, 0, 1, 1, 2, 5)), l)
            w.append((x, e))
            if e == l and e > x and rng.randrange(2):
                w.append((l, l))
            x = e + 1
        else:
            x += 1
    return w


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_by_hand():
    """x* on xxbxx: (0,2) (2,2) (3,5) (5,5); a string that is one match; an empty string; a string without a match"""
    lens, spans = [5, 3, 0, 4], [[(0, 2), (2, 2), (3, 5), (5, 5)], [(0, 3)], [], []]
    assert check(0, lens, spans, BOTH) == 1 + 0 + 0 + 4
    assert check(0, lens, spans, LEFT) == 3 + 0 + 0 + 4
    assert check(0, lens, spans, RIGHT) == 3 + 0 + 0 + 4
    assert check(0, lens, spans, BOTH, views=False) == 5


def test_counts_and_anchors():
    """c = 0, 1, 2, 3 matches per string, each with the left side anchored or not and the right side anchored or not, for every
    side, with the views and without; the empty tail match behind a non-empty match that ends at len, and behind one that does not"""
    l = 12
    firsts, lasts = ((0, 2), (1, 2)), ((9, 12), (9, 11))
    for geo in GEOS:
        lens, spans = [], []
        for c in (0, 1, 2, 3):
            for first in firsts:
                for last in lasts:
                    w = [] if c == 0 else [first] if c == 1 and last == lasts[1] else [last] if c == 1 else \
                        [first, last] if c == 2 else [first, (5, 6), last]
                    lens.append(l)
                    spans.append(w)
        spans += [[(0, 12)], [(3, 12), (12, 12)], [(3, 11), (12, 12)], [(0, 12), (12, 12)], [(0, 0), (12, 12)], [(0, 0)], [(12, 12)],
                  [(0, 4), (4, 4), (8, 12), (12, 12)]]
        lens += [l] * 8
        want = {LEFT: 0, RIGHT: 0, BOTH: 0}
        for flags in SIDES:
            for views in (True, False):
                want[flags] = check(geo, lens, spans, flags, views=views, src_mis=geo, dst_mis=3 * geo + 1)
        assert want[BOTH] < want[LEFT] and want[BOTH] < want[RIGHT] < sum(lens)


def test_nrec_around_a_wave():
    rng = random.Random(291)
    for geo in GEOS:
        for nrec in (1, 63, 64, 65):
            lens = [rng.choice((0, 1, 4, 9)) for _ in range(nrec)]
            spans = [draw(rng, l, 2) for l in lens]
            for flags in SIDES:
                check(geo, lens, spans, flags, src_mis=rng.randrange(16), dst_mis=rng.randrange(16))


def test_a_string_that_holds_a_nul():
    """the spans end at or before the NUL: never trimmed on the right, trimmed on the left, the NUL and what follows kept"""
    for geo in GEOS:
        lens, spans = [6, 5, 3], [[(0, 2), (3, 3)], [(0, 1), (1, 1)], [(0, 0)]]                # NULs at 3 of string 0, 1 of string 1, 0 of string 2
        nul_at = (3, 6 + 1, 11)
        assert check(geo, lens, spans, BOTH, nul_at=nul_at) == 4 + 4 + 3
        assert check(geo, lens, spans, RIGHT, nul_at=nul_at) == 14
        assert check(geo, lens, spans, LEFT, nul_at=nul_at, views=False) == 11


def test_lengths_around_the_tile_edges():
    rng = random.Random(292)
    for geo in GEOS:
        T = tile(geo)
        for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T):
            for lens in ([n], chop(rng, n, 40), chop(rng, n, T // 2 + 3)):
                for spans in ([[] for _ in lens], [draw(rng, l) for l in lens]):
                    for flags in SIDES:
                        check(geo, lens, spans, flags, views=bool(n & 1), src_mis=rng.randrange(16), dst_mis=rng.randrange(16), seed=n + 1)


def test_markers_on_either_side_of_a_framed_tile_edge():
    """an A on the last framed byte of a tile with its B on the first byte of the next: the empty match is match 0 of its string
    (at its start), and match c - 1 (at its end)"""
    for geo in GEOS:
        T = tile(geo)
        for tiles in (1, 2):
            # match 0: framed = string 0 (q bytes and '\n'), then string 1 starts with A B
            q = tiles * T - 2
            spans = [[], [(0, 0), (3, 5)]]
            assert frame([q, 9], spans)[tiles * T - 1:tiles * T + 1] == b"\x01\x02"
            for flags in SIDES:
                assert check(geo, [q, 9], spans, flags, src_mis=4) == q + 9
            # match c - 1: string 1 ends with A B, the A at tiles * T - 1: 3 bytes and '\n', A . B, then p position bytes
            p = tiles * T - 1 - (4 + 3)
            l = 1 + p
            spans = [[], [(0, 1), (l, l)]]
            assert frame([3, l], spans)[tiles * T - 1:tiles * T + 1] == b"\x01\x02"
            assert check(geo, [3, l], spans, BOTH, dst_mis=7) == 3 + p
            assert check(geo, [3, l], spans, RIGHT, src_mis=15, dst_mis=15) == 3 + l
            # ... and a non-empty last match whose A is the tile's last byte
            spans = [[], [(0, 1), (l, l + 2)]]
            assert frame([3, l + 2], spans)[tiles * T - 1:tiles * T + 3] == b"\x01..\x02"
            assert check(geo, [3, l + 2], spans, BOTH) == 3 + p


def test_a_string_over_three_tiles_trimmed_by_a_byte_and_by_more_than_a_tile():
    for geo in GEOS:
        T = tile(geo)
        for mis in (0, 1, 15):
            for cut in (1, T + 1):
                l = 3 * T
                spans = [[], [(0, cut), (l - cut, l)], []]
                assert check(geo, [7, l, 9], spans, BOTH, src_mis=mis, dst_mis=(mis * 7 + cut) % 16) == 16 + l - 2 * cut
                assert check(geo, [7, l, 9], spans, LEFT, src_mis=mis, views=False) == 16 + l - cut
                assert check(geo, [7, l, 9], [[], spans[1] + [(l, l)], []], RIGHT, dst_mis=mis) == 16 + l - cut


def test_all_strings_empty():
    """n = 0, nrec = 1, 63, 64, 65 and 70 000: one tile of the input, no byte; with no match and with the one empty match of x*"""
    for geo in GEOS:
        for nrec in (1, 63, 64, 65, 70000):
            none = [[] for _ in range(nrec)]
            some = [[(0, 0)] if (i * 7) % 3 == 0 else [] for i in range(nrec)]
            for flags in SIDES if nrec < 70000 else (BOTH,):
                assert check(geo, [0] * nrec, none, flags) == 0
                assert check(geo, [0] * nrec, some, flags, src_mis=geo + 1, dst_mis=geo) == 0


def test_every_source_and_destination_misalignment():
    rng = random.Random(293)
    for geo in (0, 2):
        T = tile(geo)
        lens = chop(rng, T + 200, 50)
        spans = [draw(rng, l, 2) for l in lens]
        for src_mis in range(16):
            for dst_mis in range(16):
                check(geo, lens, spans, SIDES[(src_mis + dst_mis) % 3], src_mis=src_mis, dst_mis=dst_mis)
    T = tile(3)
    lens = chop(rng, 2 * T + 200, 300)
    spans = [draw(rng, l, 3) for l in lens]
    for mis in range(16):
        check(3, lens, spans, BOTH, src_mis=mis, dst_mis=(mis * 11 + 5) % 16)
        check(3, lens, spans, SIDES[mis % 3], src_mis=(mis * 3) % 16, dst_mis=mis)


def test_bases_and_ranks_beyond_32_bits():
    """positions, match ranks and output offsets as if a long column came before"""
    rng = random.Random(294)
    for geo in GEOS:
        T = tile(geo)
        for n in (T + 1, 2 * T + 5):
            lens = [3] + chop(rng, n - 3, 70)
            spans = [draw(rng, l, 2) for l in lens]
            for flags in SIDES:
                check(geo, lens, spans, flags, src_mis=rng.randrange(16), dst_mis=rng.randrange(16), **far(T))
        check(geo, [4, 3 * T, 1], [[(0, 1)], [(0, T + 1), (2 * T, 3 * T)], [(0, 1), (1, 1)]], BOTH, src_mis=9, dst_mis=3, **far(T))


def test_stand_alone_program_under_sanitizers():
    """trim_shim.cpp with its own main, built with -fsanitize=address,undefined, over generated lengths, columns, sides, with and
    without views, misalignments and the shift beyond 2^32: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("trim")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
