"""The per-thread bodies of k_split_count and k_split_emit (trre_amd/csrc/records_block.hpp: split_mark_vecs, split_seg_kept,
split_fill_pv, split_emit_pieces) run on the host by tests/split_shim.cpp — a wave as 64 sequential lanes — against numpy.  With
a, b, l the A (0x01), B (0x02) and newlines before framed position q, a position byte at q is kept exactly when a == b; with kp
the kept bytes before q: a kept byte gives out[kp] = in[q - a - b - l], B number j gives piece_off[j + 1 + l] = kp, newline
number i gives piece_off[a + i + 1] = kp and list_off[i + 1] = a + i + 1; entry 0 of both arrays is stored by tile 0 alone,
every other byte and word once, by the lane that owns its framed byte."""
import ctypes
import random

import numpy as np

import column_shim_lib

from test_span_shim import A, B, DOT, KINDS, NL, UNSTORED, texts

GEOS = (0, 1, 2, 3)
UNSTORED_BYTE = 0xEE
FAR = dict(ra0=(1 << 32) + 5, rl0=(1 << 33) + 7, rk0=(1 << 34) + 11)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("split")
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.shim_split_tile.argtypes = [ctypes.c_int]
        L.shim_split_tile.restype = i64
        L.shim_split.argtypes = [ctypes.c_int, vp, i64, vp, i64, i64, i64, i64, ctypes.c_int, i64, i64, i64, i64, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_split_tile(geo)


def far_pos(T):
    return ((5 << 32) // T + 3) * T


def check(geo, framed, lists_only=False, pos0=0, ra0=0, rl0=0, rk0=0, seed=1):
    """the shim against numpy on one framed text; the source bytes are random letters.  Returns (kept, pieces)"""
    f = np.frombuffer(bytes(framed), dtype=np.uint8)
    m = len(f)
    isa, isb, isl = f == A, f == B, f == NL
    ispos = ~(isa | isb | isl)
    before = lambda mask, r0: r0 + np.cumsum(mask, dtype=np.int64) - mask       # exclusive
    a, b, l = before(isa, ra0), before(isb, ra0), before(isl, rl0)
    assert ((a - b >= 0) & (a - b <= 1)).all() and (a[isl] == b[isl]).all()     # A and B alternate; a newline is outside every match
    keep = ispos & (a == b)
    kp = before(keep, rk0)
    n, kept, found, lines = int(ispos.sum()), int(keep.sum()), int(isa.sum()), int(isl.sum())
    assert int(isb.sum()) == found
    src = np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8)
    want_out = src[(np.arange(m, dtype=np.int64) - (a - ra0) - (b - ra0) - (l - rl0))[keep]]
    # the piece offsets in order of their framed bytes: a B and a newline each open a piece
    opens = isb | isl
    want_piece = kp[opens]
    assert np.array_equal((b + 1 + l)[isb], (np.cumsum(opens) + ra0 + rl0)[isb]) and np.array_equal((a + l + 1)[isl], (np.cumsum(opens) + ra0 + rl0)[isl])
    want_list = (a + l + 1)[isl]
    pieces = found + lines
    out = np.full(kept + 1, 0x11, dtype=np.uint8)
    po = np.full(pieces + 2, -5, dtype=np.int64)
    lo = np.full(lines + 2, -5, dtype=np.int64)
    totals = np.zeros(4, dtype=np.int64)
    stores = np.zeros(3, dtype=np.int64)
    rc = lib().shim_split(geo, f.ctypes.data if m else None, m, src.ctypes.data if n else None, n, found, lines, kept, int(lists_only), pos0, ra0, rl0,
                          rk0, out.ctypes.data, po.ctypes.data, lo.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, m, found, lines, kept, lists_only, pos0)
    assert rc == 0, (rc,) + label
    assert totals.tolist() == [found, found, lines, kept], (label, totals)
    tile0 = bool(m) and not pos0
    if lists_only:
        assert (out[:kept] == UNSTORED_BYTE).all() and (po[:pieces + 1] == UNSTORED).all(), label
    else:
        assert np.array_equal(out[:kept], want_out), label
        assert np.array_equal(po[1:pieces + 1], want_piece), label
        assert po[0] == (0 if tile0 else UNSTORED), label
        if m and f[-1] == NL:
            assert po[pieces] == rk0 + kept, label                                   # the last newline's word is the terminator, out_len
    assert out[kept] == 0x11 and po[pieces + 1] == -5 and lo[lines + 1] == -5, label   # nothing behind the ends
    assert np.array_equal(lo[1:lines + 1], want_list), label
    assert lo[0] == (0 if tile0 else UNSTORED), label
    # every byte and word once
    assert stores.tolist() == [0 if lists_only else kept, 0 if lists_only else pieces + tile0, lines + tile0], (label, stores)
    return kept, pieces


def covered(m):
    """one match over (nearly) the whole text: tiles and pieces with no marker at depth 1, nothing kept inside"""
    body = np.full(m, DOT, dtype=np.uint8)
    if m >= 8:
        body[2], body[m - 3] = A, B
    if m:
        body[m - 1] = NL
    return body.tobytes()


def all_texts(rng, m, T):
    return [texts(rng, m, kind, T) for kind in KINDS] + [covered(m)]


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_by_hand():
    """'x*' on "bb" and on "": A B . A B . A B \\n A B \\n gives '', 'b', 'b', '' and '', ''"""
    f = bytes([A, B, DOT, A, B, DOT, A, B, NL, A, B, NL])
    out = np.zeros(2, dtype=np.uint8)
    po = np.zeros(7, dtype=np.int64)
    lo = np.zeros(3, dtype=np.int64)
    totals = np.zeros(4, dtype=np.int64)
    stores = np.zeros(3, dtype=np.int64)
    buf, src = np.frombuffer(f, dtype=np.uint8), np.frombuffer(b"bc", dtype=np.uint8)
    assert lib().shim_split(0, buf.ctypes.data, len(f), src.ctypes.data, 2, 4, 2, 2, 0, 0, 0, 0, 0, out.ctypes.data, po.ctypes.data, lo.ctypes.data,
                            totals.ctypes.data, stores.ctypes.data) == 0
    assert out.tobytes() == b"bc" and po.tolist() == [0, 0, 1, 2, 2, 2, 2] and lo.tolist() == [0, 4, 6]
    # ',' on "a,b,,c", "", ",": [a, b, '', c], [''], ['', '']
    f = bytes([DOT, A, DOT, B, DOT, A, DOT, B, A, DOT, B, DOT, NL, NL, A, DOT, B, NL])
    check(0, f)


def test_lengths_around_the_tile_edges_every_pattern():
    rng = random.Random(41)
    for geo in (0, 1, 2):
        T = tile(geo)
        for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T):
            for text in all_texts(rng, m, T):
                check(geo, text, seed=m)


def test_device_geometry_lengths_and_patterns():
    """the device's 16 KiB tiles: 0, 1, 63, 64, 65, 16 383, 16 384, 16 385 bytes and three tiles"""
    rng = random.Random(42)
    T = tile(3)
    assert T == 16384
    seen = 0
    for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T):
        for text in all_texts(rng, m, T):
            kept, pieces = check(3, text, seed=m)
            seen += kept + pieces
    assert seen > 100000


def test_no_marker_keeps_everything_and_a_covering_match_keeps_nothing():
    for geo in GEOS:
        T = tile(geo)
        m = 3 * T
        assert check(geo, bytes([DOT]) * m) == (m, 0)                       # depth 0 throughout, no piece closed
        assert check(geo, covered(m)) == (3, 2)                             # tiles 1 and most pieces: no marker, depth 1
        assert check(geo, bytes([A, B, NL]) * (m // 3)) == (0, 2 * (m // 3))    # every byte a marker
        # a match that opens on the last byte of tile 0 and closes on the first byte of tile 2: tile 1 has no marker at depth 1
        body = bytearray([DOT]) * m
        body[T - 1], body[2 * T] = A, B
        assert check(geo, bytes(body)) == (m - 2 - T, 1)


def test_lists_only():
    """the capacity path: no byte of out and no word of piece_off is stored, the list offsets are the same"""
    rng = random.Random(43)
    for geo in GEOS:
        T = tile(geo)
        for text in all_texts(rng, 2 * T + 77, T):
            check(geo, text, lists_only=True)


def test_bases_and_ranks_beyond_32_bits():
    """positions and ranks as if 5 * 2^32 framed bytes holding 2^32 + 5 matches, 2^33 + 7 newlines and 2^34 + 11 kept bytes came
    before the text"""
    rng = random.Random(44)
    for geo in GEOS:
        T = tile(geo)
        for kind in ("abn", "random", "tile_edges", "none", "newline_edges"):
            check(geo, texts(rng, 2 * T + 5, kind, T), pos0=far_pos(T), **FAR)
            check(geo, texts(rng, T + 1, kind, T), lists_only=True, pos0=far_pos(T), **FAR)
        check(geo, covered(2 * T + 5), pos0=far_pos(T), **FAR)

