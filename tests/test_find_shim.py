"""The per-thread bodies of k_find_unframe (trre_amd/csrc/records_block.hpp: k_match_unframe's compaction and find_offset_vecs,
behind k_match_count and k_chunk_scan) run on the host by tests/find_shim.cpp — a wave as 64 sequential lanes — against numpy:
framed newline number j at framed position q closes match j, match_off[j + 1] = q - j, match_off[0] = 0 is stored by tile 0
alone, every other word once, and the output is the framed text without its newlines."""
import ctypes
import random

import numpy as np

import column_shim_lib

GEOS = (0, 1, 2, 3)
UNSTORED = -0x1111111111111112          # 0xEE..EE as int64: a word nobody stored

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("find")
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.shim_find_tile.argtypes = [ctypes.c_int]
        L.shim_find_tile.restype = i64
        L.shim_find_unframe.argtypes = [ctypes.c_int, vp, i64, i64, i64, i64, i64, vp, vp, ctypes.POINTER(i64)]
        _lib = L
    return _lib


def tile(geo):
    return lib().shim_find_tile(geo)


def check(geo, framed, dst_mis=0, pos0=0, rank0=0):
    f = np.frombuffer(bytes(framed), dtype=np.uint8)
    q = np.flatnonzero(f == 10).astype(np.int64)
    found, m = len(q), len(f)
    want_off = np.concatenate([[0], pos0 + q - (rank0 + np.arange(found, dtype=np.int64))]).astype(np.int64)
    want_out = f[f != 10]
    out = np.full(m - found + 1, 0x77, dtype=np.uint8)
    off = np.full(found + 1, -5, dtype=np.int64)
    stores = ctypes.c_int64()
    rc = lib().shim_find_unframe(geo, f.ctypes.data if m else None, m, found, dst_mis, pos0, rank0, out.ctypes.data, off.ctypes.data, ctypes.byref(stores))
    assert rc == 0, (rc, geo, m, found, dst_mis, pos0)
    assert np.array_equal(out[:m - found], want_out) and out[m - found] == 0x77, (geo, m, found, dst_mis)
    assert np.array_equal(off[1:], want_off[1:]), (geo, m, found, dst_mis, pos0)
    # entry 0 belongs to one thread of tile 0: stored when there is a tile 0, by nobody behind a shift
    assert off[0] == (UNSTORED if (pos0 or not m) else 0), (geo, m, off[0])
    assert stores.value == found + (1 if m and not pos0 else 0), (geo, m, found, stores.value)


def texts(rng, m, kind, T):
    x = np.arange(m)
    if kind == "none":
        nl = np.zeros(m, bool)
    elif kind == "one":
        nl = x == rng.randrange(max(m, 1))
    elif kind == "all":
        nl = np.ones(m, bool)
    elif kind == "piece_edges":                 # first and last byte of every 64-byte piece
        nl = (x % 64 == 0) | (x % 64 == 63)
    elif kind == "tile_edges":
        nl = (x % T == 0) | (x % T == T - 1)
    elif kind == "vector_edges":
        nl = (x % 16 == 0) | (x % 16 == 15)
    else:
        nl = np.array([rng.random() < 0.2 for _ in range(m)], bool)
    body = np.array([rng.choice(b"abcxyz ") for _ in range(m)], dtype=np.uint8)
    body[nl] = 10
    return body.tobytes()


KINDS = ("none", "one", "all", "piece_edges", "tile_edges", "vector_edges", "random")


def test_geometry():
    assert [tile(g) for g in GEOS] == [1 << 10, 2 << 10, 2 << 10, 16 << 10]


def test_lengths_around_the_tile_edges_every_pattern():
    rng = random.Random(21)
    for geo in (0, 1, 2):
        T = tile(geo)
        for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T):
            for kind in KINDS:
                check(geo, texts(rng, m, kind, T), rng.randrange(16))


def test_device_geometry_lengths_and_patterns():
    """the device's 16 KiB tiles: 0, 1, 16 383, 16 384, 16 385 bytes and three tiles; no newline, one, all newlines (16 384
    offsets from one tile), newlines at the first and last byte of pieces and tiles"""
    rng = random.Random(22)
    T = tile(3)
    assert T == 16384
    for m in (0, 1, T - 1, T, T + 1, 3 * T):
        for kind in KINDS:
            check(3, texts(rng, m, kind, T), rng.randrange(16))


def test_every_destination_misalignment():
    rng = random.Random(23)
    for geo in (0, 3):
        T = tile(geo)
        f = texts(rng, 2 * T + 77, "random", T)
        for mis in range(16):
            check(geo, f, mis)


def test_tile_base_beyond_32_bits():
    """positions and ranks as if 5 * 2^32 framed bytes holding 4 * 2^32 + 7 newlines came before the text"""
    rng = random.Random(24)
    for geo in GEOS:
        T = tile(geo)
        pos0 = ((5 << 32) // T + 3) * T
        for kind in ("all", "random", "tile_edges", "none"):
            check(geo, texts(rng, 2 * T + 5, kind, T), rng.randrange(16), pos0, (4 << 32) + 7)


def test_stand_alone_program_under_sanitizers():
    """find_shim.cpp with its own main, built with -fsanitize=address,undefined, over the same lengths, patterns, misalignments
    and the shift beyond 2^32: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("find")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
