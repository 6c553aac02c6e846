"""The per-thread bodies of k_splitn_count, k_splitn_emit, k_fieldn_init, k_fieldn_pick and k_fieldn_count (trre_amd/csrc/
records_block.hpp) run on the host by tests/splitn_shim.cpp — a wave as 64 sequential lanes — against the yardstick of
tests/splitn_lib.py applied to framed texts: A (0x01) number j behind l newlines opens match r = j - L[l] of its string's
c = L[l + 1] - L[l]; the position bytes outside the CUTTING matches are kept; with kp the kept bytes and cb the cutting B before
framed position q, a kept byte gives out[kp] = in[q - a - b - l], a cutting B piece_off[cb + 1 + l] = kp, newline number i
piece_off[cb + i + 1] = kp and list_off[i + 1] = cb + i + 1; the markers of a match that does not cut store nothing; entry 0 of
both arrays is stored by tile 0 alone, every other byte and word once.  Sentinel-filled arrays stay untouched behind their ends.
The same file with its own main runs under -fsanitize=address,undefined as a process of its own, on the CPU."""
import ctypes
import random

import numpy as np

import column_shim_lib
import field_lib
import splitn_lib
from splitn_lib import INT64_MAX, INT64_MIN

from test_span_shim import A, B, DOT, KINDS, NL, UNSTORED, texts, well_formed

GEOS = (0, 1, 2, 3)
UNSTORED_BYTE = 0xEE
FAR = dict(ra0=(1 << 32) + 5, rl0=(1 << 33) + 7, rk0=(1 << 34) + 11, rc0=(1 << 31) + 3)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("splitn")
        vp, i64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32
        L.shim_splitn_tile.argtypes = [ctypes.c_int]
        L.shim_splitn_tile.restype = i64
        L.shim_splitn_cuts.argtypes = [i64, i64, i64, u32]
        L.shim_splitn.argtypes = [ctypes.c_int, vp, i64, vp, i64, i64, i64, i64, u32, i64, i64, ctypes.c_int, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp]
        L.shim_fieldn_bounds.argtypes = [ctypes.c_int, vp, i64, vp, i64, i64, i64, u32, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_splitn_tile(geo)


def far_pos(T):
    return ((5 << 32) // T + 3) * T


def closed(text):
    """a framed text whose last byte is a newline: every marker belongs to a string"""
    return well_formed(text[:-1] + bytes([NL])) if text else text


def strings_of(framed):
    """per string of a framed text (bytes of A, B, DOT, closed by NL) its spans, relative to the string's position bytes"""
    per, spans, at, start = [], [], 0, None
    for c in framed:
        if c == A:
            start = at
        elif c == B:
            spans.append((start, at))
        elif c == NL:
            per.append((at, spans))
            spans, at = [], 0
        else:
            at += 1
    return per


def check(geo, framed, limit, from_end, lists_only=False, pos0=0, ra0=0, rl0=0, rk0=0, rc0=0, seed=1):
    """the shim against the yardstick on one framed text; the source bytes are random letters.  Returns (kept, pieces)"""
    f = np.frombuffer(bytes(framed), dtype=np.uint8)
    m = len(f)
    per = strings_of(bytes(framed))
    n, found, lines = sum(length for length, _ in per), sum(len(w) for _, w in per), len(per)
    src = np.random.RandomState(seed).randint(ord("a"), ord("z") + 1, size=n).astype(np.uint8)
    text, strs, at = src.tobytes(), [], 0
    for length, _ in per:
        strs.append(text[at:at + length])
        at += length
    want_out, want_po, want_lo = splitn_lib.expect(strs, [w for _, w in per], limit, from_end)
    kept, pieces = len(want_out), want_lo[-1]
    cuts = pieces - lines
    out = np.full(kept + 1, 0x11, dtype=np.uint8)
    po = np.full(pieces + 2, -5, dtype=np.int64)
    lo = np.full(lines + 2, -5, dtype=np.int64)
    totals = np.zeros(5, dtype=np.int64)
    stores = np.zeros(3, dtype=np.int64)
    rc = lib().shim_splitn(geo, f.ctypes.data if m else None, m, src.ctypes.data if n else None, n, found, lines, limit, int(from_end), kept, cuts,
                           int(lists_only), pos0, ra0, rl0, rk0, rc0, out.ctypes.data, po.ctypes.data, lo.ctypes.data, totals.ctypes.data,
                           stores.ctypes.data)
    label = (geo, m, found, lines, limit, from_end, lists_only, pos0)
    assert rc == 0, (rc,) + label
    assert totals.tolist() == [found, found, lines, kept, cuts], (label, totals)
    tile0 = bool(m) and not pos0
    if lists_only:
        assert (out[:kept] == UNSTORED_BYTE).all() and (po[:pieces + 1] == UNSTORED).all(), label
    else:
        assert out[:kept].tobytes() == want_out, label
        assert po[1:pieces + 1].tolist() == [rk0 + x for x in want_po[1:]], label
        assert po[0] == (0 if tile0 else UNSTORED), label
    assert out[kept] == 0x11 and po[pieces + 1] == -5 and lo[lines + 1] == -5, label   # nothing behind the ends
    assert lo[1:lines + 1].tolist() == [rc0 + rl0 + x for x in want_lo[1:]], label
    assert lo[0] == (0 if tile0 else UNSTORED), label
    # every byte and word once
    assert stores.tolist() == [0 if lists_only else kept, 0 if lists_only else pieces + tile0, lines + tile0], (label, stores)
    return kept, pieces


def check_bounds(geo, framed, k, limit, from_end):
    """k_fieldn_init, k_fieldn_pick and k_fieldn_count against the yardstick's field by index"""
    f = np.frombuffer(bytes(framed), dtype=np.uint8)
    per = strings_of(bytes(framed))
    nrec = len(per)
    off = np.zeros(nrec + 1, dtype=np.int64)
    off[1:] = np.cumsum([length for length, _ in per])
    lo, hi = np.full(nrec + 1, -5, dtype=np.int64), np.full(nrec + 1, -5, dtype=np.int64)
    words = (nrec + 63) // 64
    valid = np.full(words + 1, -5, dtype=np.int64)
    totals, stores = np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.int64)
    rc = lib().shim_fieldn_bounds(geo, f.ctypes.data, len(f), off.ctypes.data, nrec, k, limit, int(from_end), lo.ctypes.data, hi.ctypes.data,
                                  valid.ctypes.data, totals.ctypes.data, stores.ctypes.data)
    label = (geo, len(f), nrec, k, limit, from_end)
    assert rc == 0, (rc,) + label
    assert lo[nrec] == -5 and hi[nrec] == -5 and valid[words] == -5, label
    assert stores.tolist() == [words, nrec, nrec], (label, stores)
    n_valid = n_bytes = 0
    for i, (length, spans) in enumerate(per):
        # pieces of a string of `length` distinct positions: cut a range, read the bounds off the pieces
        cutting = splitn_lib.cutting(spans, limit, from_end)
        bounds = [(0 if j == 0 else cutting[j - 1][1], length if j == len(cutting) else cutting[j][0]) for j in range(len(cutting) + 1)]
        want = field_lib.pick(bounds, k)
        has = bool((int(valid[i // 64]) >> (i % 64)) & 1)
        assert has == (want is not None), label + (i,)
        s, e = want if want is not None else (length, length)
        assert (lo[i] - off[i], hi[i] - off[i]) == (s, e), label + (i,)
        n_valid += has
        n_bytes += e - s
    if nrec % 64:
        assert int(valid.view(np.uint64)[words - 1]) >> (nrec % 64) == 0, label            # the bitmap's tail is zero
    assert totals.tolist() == [n_valid, n_bytes], (label, totals)


def covered(m):
    """one match over (nearly) the whole text: tiles and pieces with no marker inside one match"""
    body = np.full(m, DOT, dtype=np.uint8)
    if m >= 8:
        body[2], body[m - 3] = A, B
    if m:
        body[m - 1] = NL
    return body.tobytes()


def all_texts(rng, m, T):
    return [closed(texts(rng, m, kind, T)) for kind in KINDS] + [covered(m)]


def most_matches(framed):
    return max([len(w) for _, w in strings_of(framed)] or [0])


ENDS = (False, True)


def test_geometry_and_the_rule_as_the_kernels_have_it():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]
    for c in range(5):
        for r in range(c):
            for limit in (0, 1, 2, 4, 5, INT64_MAX, -1, INT64_MIN):
                for from_end in ENDS:
                    assert bool(lib().shim_splitn_cuts(r, c, limit, int(from_end))) == splitn_lib.cuts(r, c, limit, from_end), (r, c, limit, from_end)


def test_by_hand():
    """'x*' on "bb" and on "": A B . A B . A B \\n A B \\n; ',' on "a,b,,c", "", ","."""
    for f in (bytes([A, B, DOT, A, B, DOT, A, B, NL, A, B, NL]), bytes([DOT, A, DOT, B, DOT, A, DOT, B, A, DOT, B, DOT, NL, NL, A, DOT, B, NL])):
        for limit in (0, 1, 2, 3, 4, -1):
            for from_end in ENDS:
                check(0, f, limit, from_end)
                for k in (0, 1, -1, -2, 3, -4):
                    check_bounds(0, f, k, limit, from_end)
    assert check(0, bytes([DOT, A, DOT, B, DOT, A, DOT, B, DOT, NL]), 1, False) == (4, 2)       # a=b=c: "a", "b=c"


def test_random_soups_every_geometry_every_limit_both_ends():
    rng = random.Random(51)
    for geo in GEOS:
        T = tile(geo)
        for m in (T // 2 + 3, 2 * T + 77):
            f = closed(texts(rng, m, "random", T))
            c = most_matches(f)
            assert c >= 3
            for limit in splitn_lib.limits_of(c):
                for from_end in ENDS:
                    check(geo, f, limit, from_end, seed=m)
                    if geo != 3 or limit in (1, c - 1):
                        for k in (0, 1, -1, -2, limit if abs(limit) < 100 else 5, -3):
                            check_bounds(geo, f, k, limit, from_end)


def test_lengths_around_the_tile_edges_every_pattern():
    rng = random.Random(52)
    for geo in (0, 1, 2):
        T = tile(geo)
        for m in (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T):
            for text in all_texts(rng, m, T):
                for limit, from_end in ((0, False), (1, False), (1, True), (2, True), (3, False), (INT64_MAX, True), (INT64_MIN, False)):
                    check(geo, text, limit, from_end, seed=m + 1)


def test_device_geometry_lengths_and_patterns():
    rng = random.Random(53)
    T = tile(3)
    assert T == 16384
    for m in (1, 65, T - 1, T, T + 1, 3 * T):
        for text in all_texts(rng, m, T):
            for limit, from_end in ((0, True), (1, False), (1, True), (3, False)):
                check(3, text, limit, from_end, seed=m)
            if m > 1:
                check_bounds(3, text, 1, 1, True)
                check_bounds(3, text, -1, 3, False)


def test_tiles_and_pieces_wholly_inside_one_match():
    """a tile, a 64-byte piece or a thread segment with no marker of its own: kept when the match does not cut, dropped when it does"""
    for geo in GEOS:
        T = tile(geo)
        m = 3 * T
        for from_end in ENDS:
            assert check(geo, covered(m), 0, from_end) == (m - 3, 1)          # the one match does not cut: every position byte kept
            assert check(geo, covered(m), 1, from_end) == (3, 2)              # it cuts: nothing of it kept
        # two matches in one string, the first over tile 1: from the front with limit 1 it cuts, from the end it does not
        body = bytearray([DOT]) * m
        body[T - 1], body[2 * T], body[2 * T + 5], body[2 * T + 9], body[m - 1] = A, B, A, B, NL
        assert check(geo, bytes(body), 1, False) == (m - 5 - T, 2)
        assert check(geo, bytes(body), 1, True) == (m - 5 - 3, 2)
        assert check(geo, bytes(body), 2, True) == (m - 5 - T - 3, 3)
        # ... and the string's closing newline two tiles behind the first marker: c comes from L, not from the tile
        body = bytearray([DOT]) * (4 * T)
        body[5], body[9], body[4 * T - 20], body[4 * T - 10], body[4 * T - 1] = A, B, A, B, NL
        assert check(geo, bytes(body), 1, True) == (4 * T - 5 - 9, 2)
        assert check(geo, bytes(body), 1, False) == (4 * T - 5 - 3, 2)


def test_lists_only():
    rng = random.Random(54)
    for geo in GEOS:
        T = tile(geo)
        for text in all_texts(rng, 2 * T + 77, T):
            check(geo, text, 1, True, lists_only=True)
            check(geo, text, 2, False, lists_only=True)


def test_bases_and_ranks_beyond_32_bits():
    rng = random.Random(55)
    for geo in GEOS:
        T = tile(geo)
        for kind in ("abn", "random", "tile_edges", "none", "newline_edges"):
            for limit, from_end in ((1, False), (1, True), (0, False), (-1, True)):
                check(geo, closed(texts(rng, 2 * T + 5, kind, T)), limit, from_end, pos0=far_pos(T), **FAR)
            check(geo, closed(texts(rng, T + 1, kind, T)), 1, True, lists_only=True, pos0=far_pos(T), **FAR)
        check(geo, covered(2 * T + 5), 0, False, pos0=far_pos(T), **FAR)
        check(geo, covered(2 * T + 5), 1, True, pos0=far_pos(T), **FAR)


def test_the_bodies_under_the_sanitizers():
    """tests/splitn_shim.cpp with its own main, built with -fsanitize=address,undefined: a process of its own, on the CPU"""
    done = column_shim_lib.sanitized("splitn")
    assert done.returncode == 0, (done.stdout.decode()[-2000:], done.stderr.decode()[-4000:])
    assert b"shapes ok" in done.stdout
