"""The ragged-records passes' per-thread bodies (trre_amd/csrc/records_block.hpp) run on the host by tests/records_shim.cpp,
against numpy: the staged copy, the ranks R_i (number of '\\n' in staged[0, off[i+1])), the first record of every tile, the
newlines per tile, the output offsets (just past output newline R_i) and the in-place restore — over random buffers, record
sizes, misalignments and four tile geometries (64 B to the device's 64 KiB), with record ends on tile edges, runs of empty
records, NULs, ranks beyond 2^32 (a large base) and nrec = 0."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "records_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "trre_amd", "csrc", "records_block.hpp")
SO = os.path.join(HERE, "_shim", "librecords_shim.so")
GEOS = (0, 1, 2, 3)
MASK56 = (1 << 56) - 1

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, HDR, os.path.join(os.path.dirname(HDR), "scan_block.hpp")]
        if not (os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(d) for d in deps)):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", SRC, "-o", SO], check=True)
        L = ctypes.CDLL(SO)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.shim_rec_tile.argtypes = [ctypes.c_int]
        L.shim_rec_tile.restype = i64
        L.shim_rec_stage.argtypes = [ctypes.c_int, vp, i64, i64, vp, i64, ctypes.c_int, ctypes.c_uint64, vp, vp, vp, vp]
        L.shim_rec_locate.argtypes = [ctypes.c_int, vp, i64, i64, vp, i64, ctypes.c_uint64]
        L.shim_rec_restore.argtypes = [vp, vp, i64, vp]
        L.shim_rec_restore.restype = None
        _lib = L
    return _lib


def ptr(a):
    return a.ctypes.data if a.size else None


def stage(geo, data, off, mis, keep=0, base0=0):
    n, nrec = len(data), len(off) - 1
    tile = lib().shim_rec_tile(geo)
    tiles = (mis + n + tile - 1) // tile if n else 0
    src = np.frombuffer(data, dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
    staged = np.zeros(n, np.uint8)
    out_off = np.full(nrec + 1, -1, np.int64)
    part = np.zeros(tiles + 1, np.int64)
    cnt = np.zeros(max(tiles, 1), np.uint64)
    offa = np.ascontiguousarray(off, dtype=np.int64)
    assert lib().shim_rec_stage(geo, ptr(src), n, mis, offa.ctypes.data, nrec, keep, base0, ptr(staged), out_off.ctypes.data,
                                part.ctypes.data, cnt.ctypes.data) == 0
    return staged.tobytes(), out_off, part, cnt[:tiles]


def want_staged(data, off):
    b = bytearray(data)
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            b[off[i + 1] - 1] = 10
    return bytes(b)


def random_offsets(rng, n):
    """record boundaries anywhere, runs of empty records included"""
    k = rng.choice([0, 1, 2, 5, 40, max(1, n // 3)])
    cuts = sorted(rng.randrange(0, n + 1) for _ in range(k))
    if cuts and rng.random() < 0.5:
        cuts += [cuts[-1]] * rng.randrange(1, 5)           # empty records
    return np.array([0] + sorted(cuts) + [n], dtype=np.int64)


def random_data(rng, n):
    alphabet = b"ab\n\n\0xyz" if rng.random() < 0.5 else b"abcdefgh\n"
    return bytes(rng.choice(alphabet) for _ in range(n))


def check_stage(geo, data, off, mis, keep=0, base0=0):
    staged, out_off, part, cnt = stage(geo, data, off, mis, keep, base0)
    st = want_staged(data, off)
    assert staged == st
    tile = lib().shim_rec_tile(geo)
    nl = np.frombuffer(st, dtype=np.uint8) == 10 if st else np.zeros(0, bool)
    csum = np.concatenate([[0], np.cumsum(nl)]).astype(np.int64)
    for i in range(len(off) - 1):
        p = int(off[i + 1])
        got = int(out_off[i + 1])
        assert got & MASK56 == base0 + int(csum[p]), (geo, mis, i)
        if keep and p > off[i]:
            assert got >> 56 == data[p - 1], (geo, mis, i)
    # tile counts and the partition: v = position + mis, tile b holds v in [b * tile, (b + 1) * tile)
    if data:
        v = np.arange(len(st)) + mis
        assert [int(c) for c in cnt] == [int(nl[(v >= b * tile) & (v < (b + 1) * tile)].sum()) for b in range(len(cnt))]
        ends = off[1:]
        end_tile = np.where(ends == 0, 0, (ends - 1 + mis) // tile)
        for b in range(len(part)):
            assert part[b] == (0 if b == 0 else int(np.searchsorted(end_tile, b, side="left"))), (geo, b)
    return st, out_off


def test_stage_random():
    rng = random.Random(5150)
    for trial in range(300):
        geo = GEOS[trial % 3]                      # (the device's geometry below: 64 KiB tiles)
        n = rng.choice([1, 2, 15, 16, 17, 63, 64, 65, 200, 1000, 3000])
        data = random_data(rng, n)
        check_stage(geo, data, random_offsets(rng, n), rng.randrange(16), keep=trial & 1)


def test_stage_record_ends_on_tile_edges():
    """records that end on the last or first byte of a tile, and straddle several tiles"""
    for geo in (0, 1, 2):
        tile = lib().shim_rec_tile(geo)
        for mis in (0, 1, 15):
            n = 5 * tile + 7
            data = bytes((i * 7) % 26 + 97 for i in range(n))
            edges = sorted({max(0, min(n, b * tile - mis + d)) for b in range(1, 6) for d in (-1, 0, 1)})
            off = np.array([0] + edges + [n], dtype=np.int64)
            check_stage(geo, data, off, mis)
            check_stage(geo, data, np.array([0, 3 * tile + 1, n], dtype=np.int64), mis)


def test_stage_device_geometry():
    rng = random.Random(77)
    for mis in (0, 9):
        n = 3 * (64 << 10) + 123
        data = random_data(rng, n)
        lines = [i + 1 for i, c in enumerate(data) if c == 10]
        check_stage(3, data, np.array([0] + lines[::3] + [n], dtype=np.int64), mis, keep=1)
        check_stage(3, data, np.array([0] + sorted(rng.randrange(n + 1) for _ in range(500)) + [n], dtype=np.int64), mis)


def test_empty_cases():
    """nrec = 0 (n = 0); n = 0 with empty records; a lone empty record set around a non-empty one"""
    for geo in GEOS:
        check_stage(geo, b"", np.array([0], dtype=np.int64), 3)
        _, out_off = check_stage(geo, b"", np.array([0, 0, 0], dtype=np.int64), 0)
        check_stage(geo, b"abc", np.array([0, 0, 0, 3, 3], dtype=np.int64), 5)


def test_ranks_beyond_32_bits():
    rng = random.Random(3)
    base0 = (5 << 32) + 12345
    for geo in GEOS:
        data = random_data(rng, 2000)
        off = random_offsets(rng, 2000)
        st, out_off = check_stage(geo, data, off, 7, base0=base0)
        locate_check(geo, st, off, 4, base0)


def scan_like(staged, drop):
    """a stand-in for the scan: every line prints a framing '\\n' and some bytes of its own (never '\\n')"""
    out = bytearray()
    for line in staged.split(b"\n")[:-1] if staged.endswith(b"\n") else staged.split(b"\n"):
        out += bytes(c for c in line if c not in drop).replace(b"\0", b"") * 1 + b"\n"
    return bytes(out)


def locate_check(geo, staged, off, mis, base0=0, out=None):
    nl = np.frombuffer(staged, dtype=np.uint8) == 10 if staged else np.zeros(0, bool)
    csum = np.concatenate([[0], np.cumsum(nl)]).astype(np.int64)
    ranks = np.array([0] + [base0 + int(csum[p]) for p in off[1:]], dtype=np.int64)
    out = scan_like(staged, b"b") if out is None else out
    if not out:
        return
    onl = np.flatnonzero(np.frombuffer(out, dtype=np.uint8) == 10)
    src = np.frombuffer(out, dtype=np.uint8).copy()
    assert lib().shim_rec_locate(geo, src.ctypes.data, len(out), mis, ranks.ctypes.data, len(off) - 1, base0) == 0
    for i in range(len(off) - 1):
        r = int(csum[off[i + 1]])
        assert ranks[i + 1] == (0 if r == 0 else int(onl[r - 1]) + 1), (geo, mis, i)
    assert ranks[-1] == len(out)


def test_locate_random():
    rng = random.Random(99)
    for trial in range(300):
        geo = GEOS[trial % 3]
        n = rng.choice([1, 2, 17, 64, 65, 300, 2000])
        data = random_data(rng, n)
        off = random_offsets(rng, n)
        staged = want_staged(data, off)
        locate_check(geo, staged, off, rng.randrange(16))
        locate_check(geo, staged, off, rng.randrange(16), out=scan_like(staged, b"") .replace(b"a", b"aaa"))


def test_locate_device_geometry():
    rng = random.Random(1)
    n = 200000
    data = random_data(rng, n)
    off = np.array([0] + sorted(rng.randrange(n + 1) for _ in range(3000)) + [n], dtype=np.int64)
    staged = want_staged(data, off)
    for mis in (0, 11):
        locate_check(3, staged, off, mis)


def test_restore():
    rng = random.Random(8)
    for trial in range(50):
        n = rng.randrange(1, 500)
        data = random_data(rng, n)
        off = random_offsets(rng, n)
        staged, out_off, _, _ = stage(trial % 4, data, off, trial % 16, keep=1)
        dst = np.frombuffer(staged, dtype=np.uint8).copy()
        lib().shim_rec_restore(dst.ctypes.data, np.ascontiguousarray(off).ctypes.data, len(off) - 1, out_off.ctypes.data)
        assert dst.tobytes() == data
