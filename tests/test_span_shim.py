"""The per-thread bodies of k_span_count and k_span_emit (trre_amd/csrc/records_block.hpp: span_mark_vecs, span_seg_count,
span_fill_pv, span_emit_pieces) run on the host by tests/span_shim.cpp — a wave as 64 sequential lanes — against numpy.  With a,
b, l the A (0x01), B (0x02) and newlines before framed position q: A number j at q gives start[j] = q - a - b - l, B number j
gives end[j] by the same expression, newline number i gives list_off[i + 1] = a; list_off[0] = 0 is stored by tile 0 alone,
every other word once, by the lane that owns its marker."""
import ctypes
import random

import numpy as np

import column_shim_lib

GEOS = (0, 1, 2, 3)
UNSTORED = -0x1111111111111112          # 0xEE..EE as int64: a word nobody stored
A, B, NL, DOT = 1, 2, 10, ord(".")

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("span")
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.shim_span_tile.argtypes = [ctypes.c_int]
        L.shim_span_tile.restype = i64
        L.shim_span.argtypes = [ctypes.c_int, vp, i64, i64, i64, ctypes.c_int, i64, i64, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_span_tile(geo)


def check(geo, framed, lists_only=False, pos0=0, ra0=0, rl0=0):
    f = np.frombuffer(bytes(framed), dtype=np.uint8)
    m = len(f)
    isa, isb, isl = f == A, f == B, f == NL
    before = lambda mask, r0: r0 + np.cumsum(mask, dtype=np.int64) - mask       # exclusive
    a, b, l = before(isa, ra0), before(isb, ra0), before(isl, rl0)
    pos = pos0 + np.arange(m, dtype=np.int64) - a - b - l
    want_start, want_end, want_list = pos[isa], pos[isb], a[isl]
    found, lines = int(isa.sum()), int(isl.sum())
    assert int(isb.sum()) == found
    start = np.full(found + 1, -5, dtype=np.int64)
    end = np.full(found + 1, -5, dtype=np.int64)
    lo = np.full(lines + 2, -5, dtype=np.int64)
    totals = np.zeros(3, dtype=np.int64)
    stores = ctypes.c_int64()
    rc = lib().shim_span(geo, f.ctypes.data if m else None, m, found, lines, int(lists_only), pos0, ra0, rl0, start.ctypes.data, end.ctypes.data,
                         lo.ctypes.data, totals.ctypes.data, ctypes.byref(stores))
    assert rc == 0, (rc, geo, m, found, lines, lists_only, pos0)
    assert totals.tolist() == [found, found, lines], (geo, m, totals)
    if lists_only:
        assert (start[:found] == UNSTORED).all() and (end[:found] == UNSTORED).all(), (geo, m)
    else:
        assert np.array_equal(start[:found], want_start) and np.array_equal(end[:found], want_end), (geo, m, pos0)
    assert start[found] == -5 and end[found] == -5 and lo[lines + 1] == -5
    assert np.array_equal(lo[1:lines + 1], want_list), (geo, m, pos0)
    # entry 0 belongs to thread 0 of tile 0: stored when there is a tile 0, by nobody behind a shift
    assert lo[0] == (UNSTORED if (pos0 or not m) else 0), (geo, m, lo[0])
    assert stores.value == (0 if lists_only else 2 * found) + lines + (1 if m and not pos0 else 0), (geo, m, found, lines, stores.value)
    return found, lines


def well_formed(body):
    """drop an A without its B at the end of a cut text"""
    body = bytearray(body)
    last_a = body.rfind(bytes([A]))
    if last_a >= 0 and body.find(bytes([B]), last_a) < 0:
        body[last_a] = DOT
    return bytes(body)


def texts(rng, m, kind, T):
    x = np.arange(m)
    body = np.full(m, DOT, dtype=np.uint8)
    if kind == "none":
        pass
    elif kind == "abn":                         # every byte a marker: an empty match per empty line
        body[:] = np.array([A, B, NL], dtype=np.uint8)[x % 3]
    elif kind == "abab":                        # every byte a marker, no newline
        body[:] = np.array([A, B], dtype=np.uint8)[x % 2]
    elif kind == "piece_edges":                 # A on the last byte of every 64-byte piece, its B on the first of the next
        body[x % 64 == 63] = A
        body[(x % 64 == 0) & (x > 0)] = B
    elif kind == "tile_edges":                  # ... of every tile
        body[x % T == T - 1] = A
        body[(x % T == 0) & (x > 0)] = B
    elif kind == "newline_edges":               # a newline at the first and the last byte of every tile
        body[(x % T == 0) | (x % T == T - 1)] = NL
    else:
        out, is_open = [], False
        for k in range(m):
            r = rng.randrange(8)
            if not is_open and r == 0:
                out.append(A)
                is_open = True
            elif is_open and r < 3:
                out.append(B)
                is_open = False
            elif not is_open and r == 1:
                out.append(NL)
            else:
                out.append(DOT)
        body = np.array(out, dtype=np.uint8).reshape(m)
    return well_formed(body.tobytes())


KINDS = ("none", "abn", "abab", "piece_edges", "tile_edges", "newline_edges", "random")


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_by_hand():
    """'x*' on "bb" and on "": A B . A B . A B \\n A B \\n"""
    f = bytes([A, B, DOT, A, B, DOT, A, B, NL, A, B, NL])
    check(0, f)
    start = np.zeros(4, dtype=np.int64)
    end = np.zeros(4, dtype=np.int64)
    lo = np.zeros(3, dtype=np.int64)
    totals = np.zeros(3, dtype=np.int64)
    stores = ctypes.c_int64()
    buf = np.frombuffer(f, dtype=np.uint8)
    assert lib().shim_span(0, buf.ctypes.data, len(f), 4, 2, 0, 0, 0, 0, start.ctypes.data, end.ctypes.data, lo.ctypes.data, totals.ctypes.data,
                           ctypes.byref(stores)) == 0
    # positions in the caller's values "bb": string 0 is [0, 2), string 1 is [2, 2)
    assert start.tolist() == [0, 1, 2, 2] and end.tolist() == [0, 1, 2, 2] and lo.tolist() == [0, 3, 4]


def test_lengths_around_the_tile_edges_every_pattern():
    rng = random.Random(31)
    for geo in (0, 1, 2):
        T = tile(geo)
        for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T):
            for kind in KINDS:
                check(geo, texts(rng, m, kind, T))


def test_device_geometry_lengths_and_patterns():
    """the device's 16 KiB tiles: 0, 1, 63, 64, 65, 16 383, 16 384, 16 385 bytes and three tiles"""
    rng = random.Random(32)
    T = tile(3)
    assert T == 16384
    seen = 0
    for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T):
        for kind in KINDS:
            found, lines = check(3, texts(rng, m, kind, T))
            seen += found + lines
    assert seen > 100000


def test_list_offsets_only():
    """the capacity path: no start or end word is stored, the list offsets are the same"""
    rng = random.Random(33)
    for geo in GEOS:
        T = tile(geo)
        for kind in KINDS:
            check(geo, texts(rng, 2 * T + 77, kind, T), lists_only=True)


def test_bases_and_ranks_beyond_32_bits():
    """positions and ranks as if 5 * 2^32 framed bytes holding 2^32 + 5 matches and 2^33 + 7 newlines came before the text"""
    rng = random.Random(34)
    for geo in GEOS:
        T = tile(geo)
        pos0 = ((5 << 32) // T + 3) * T
        for kind in ("abn", "random", "tile_edges", "none", "newline_edges"):
            check(geo, texts(rng, 2 * T + 5, kind, T), pos0=pos0, ra0=(1 << 32) + 5, rl0=(1 << 33) + 7)
            check(geo, texts(rng, T + 1, kind, T), lists_only=True, pos0=pos0, ra0=(1 << 32) + 5, rl0=(1 << 33) + 7)


def test_stand_alone_program_under_sanitizers():
    """span_shim.cpp with its own main, built with -fsanitize=address,undefined, over the same lengths, patterns, the
    list-offsets-only flag and the shift beyond 2^32: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("span")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
