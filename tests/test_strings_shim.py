"""The packed-strings passes' per-thread bodies (trre_amd/csrc/records_block.hpp: k_str_part, k_str_stage, k_str_rank,
k_str_unframe) run on the host by tests/strings_shim.cpp, against numpy: the staged text (every string with a '\\n' behind
it), the ranks R_i (number of '\\n' in the staged text up to and with string i's closing one), the first string of every tile,
the newlines per tile, the unframed bytes and the final offsets — over random buffers, string sizes, source and destination
misalignments 0-15 and four tile geometries (64 B to the device's 16 KiB), with string ends on tile edges, strings that span
tiles, runs of empty strings, all-empty input, 1-byte strings throughout, ranks beyond 2^32 (a large base) and nrec = 0.  The
passes are also composed end to end with the records passes' own count / locate bodies (tests/records_shim.cpp) around a
stand-in scan."""
import ctypes
import os
import random
import subprocess

import numpy as np

from test_records_shim import lib as rec_lib, random_data, random_offsets, scan_like

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "strings_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "trre_amd", "csrc", "records_block.hpp")
SO = os.path.join(HERE, "_shim", "libstrings_shim.so")
GEOS = (0, 1, 2, 3)
REC_TILE = {0: 64, 1: 128, 2: 1024, 3: 64 << 10}     # records_shim.cpp's geometries (the locate pass keeps its own tiles)

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
        L.shim_str_tile.argtypes = [ctypes.c_int]
        L.shim_str_tile.restype = i64
        L.shim_str_stage.argtypes = [ctypes.c_int, vp, i64, i64, vp, i64, ctypes.c_uint64, vp, vp, vp, vp]
        L.shim_str_unframe.argtypes = [ctypes.c_int, vp, i64, vp, i64, i64, vp]
        _lib = L
    return _lib


def ptr(a):
    return a.ctypes.data if a.size else None


def recs_of(data, off):
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_stage(geo, data, off, mis, base0=0):
    """the staged text, the ranks, the partition and the counts of one call; returns (staged, ranks)"""
    n, nrec = len(data), len(off) - 1
    total = n + nrec
    tile = lib().shim_str_tile(geo)
    tiles = (total + tile - 1) // tile
    src = np.frombuffer(data, dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
    staged = np.zeros(total, np.uint8)
    out_off = np.full(nrec + 1, -1, np.int64)
    part = np.zeros(tiles + 1, np.int64)
    cnt = np.zeros(max(tiles, 1), np.uint64)
    offa = np.ascontiguousarray(off, dtype=np.int64)
    rc = lib().shim_str_stage(geo, ptr(src), n, mis, offa.ctypes.data, nrec, base0, ptr(staged), out_off.ctypes.data, part.ctypes.data,
                              cnt.ctypes.data)
    assert rc == 0, (geo, mis, rc)
    want = b"".join(r + b"\n" for r in recs_of(data, off))
    assert staged.tobytes() == want, (geo, mis, list(off))
    nl = np.frombuffer(want, dtype=np.uint8) == 10 if want else np.zeros(0, bool)
    csum = np.concatenate([[0], np.cumsum(nl)]).astype(np.int64)
    keys = offa[1:] + np.arange(nrec)
    assert out_off[0] == -1                                     # (entry 0 is the locate pass's)
    assert [int(r) for r in out_off[1:]] == [base0 + int(csum[k + 1]) for k in keys], (geo, mis)
    assert [int(c) for c in cnt[:tiles]] == [int(nl[b * tile:(b + 1) * tile].sum()) for b in range(tiles)]
    assert [int(x) for x in part] == [int(np.searchsorted(keys, b * tile, side="left")) for b in range(tiles + 1)]
    return want, out_off


def check_unframe(geo, framed, located, dst_mis):
    """framed: the records' outputs, each closed by a '\\n' just before located[i + 1]"""
    m, nrec = len(framed), len(located) - 1
    src = np.frombuffer(framed, dtype=np.uint8).copy() if m else np.zeros(0, np.uint8)
    oo = np.array(located, dtype=np.int64)
    out = np.zeros(m - nrec, np.uint8)
    rc = lib().shim_str_unframe(geo, ptr(src), m, oo.ctypes.data, nrec, dst_mis, ptr(out))
    assert rc == 0, (geo, dst_mis, rc)
    want = b"".join(framed[located[i]:located[i + 1] - 1] for i in range(nrec))
    assert out.tobytes() == want, (geo, dst_mis, located)
    assert oo.tolist() == [located[i] - i for i in range(nrec + 1)], (geo, dst_mis)
    return want, oo.tolist()


def end_to_end(geo, data, off, mis, dst_mis, base0=0, drop=b"b", grow=False):
    """stage -> a stand-in scan -> the records passes' count / locate -> unframe, against the specification per string"""
    staged, ranks = check_stage(geo, data, off, mis, base0)
    nrec = len(off) - 1
    if nrec == 0:
        return
    framed = scan_like(staged, drop)
    if grow:
        framed = framed.replace(b"a", b"aaa")
    ranks[0] = 0
    src = np.frombuffer(framed, dtype=np.uint8).copy()
    assert rec_lib().shim_rec_locate(geo, src.ctypes.data, len(framed), 0, ranks.ctypes.data, nrec, base0) == 0
    assert ranks[-1] == len(framed)
    got, oo = check_unframe(geo, framed, ranks.tolist(), dst_mis)
    outs = []
    for r in recs_of(data, off):
        o = scan_like(r + b"\n", drop)
        outs.append((o.replace(b"a", b"aaa") if grow else o)[:-1])
    assert got == b"".join(outs), (geo, mis, dst_mis, list(off))
    assert oo == [0] + np.cumsum([len(x) for x in outs]).tolist()


def test_geometries():
    assert [lib().shim_str_tile(g) for g in GEOS] == [64, 128, 1024, 16 << 10]
    assert [rec_lib().shim_rec_tile(g) for g in GEOS] == [REC_TILE[g] for g in GEOS]


def test_random_end_to_end():
    rng = random.Random(4242)
    for trial in range(400):
        geo = GEOS[trial % 3]
        n = rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 200, 1000, 3000])
        data = random_data(rng, n)
        end_to_end(geo, data, random_offsets(rng, n), trial % 16, (trial // 16 + trial) % 16, grow=bool(trial & 1))


def test_every_misalignment_pair():
    rng = random.Random(16)
    data = random_data(rng, 700)
    off = random_offsets(rng, 700)
    for geo in (0, 2):
        for mis in range(16):
            for dst_mis in range(16):
                end_to_end(geo, data, off, mis, dst_mis)


def test_string_ends_on_tile_edges():
    """closing newlines on the first and the last byte of a staged tile; strings that span several tiles"""
    for geo in (0, 1, 2):
        tile = lib().shim_str_tile(geo)
        n = 6 * tile
        data = bytes((i * 7) % 26 + 97 for i in range(n))
        for mis in (0, 1, 15):
            # string i's closing newline sits at staged position off[i + 1] + i: aim at b * tile - 1, b * tile and b * tile + 1
            ends, i = [], 0
            for b in range(1, 5):
                for d in (-1, 0, 1):
                    ends.append(b * tile + d - i)
                    i += 1
            off = np.array([0] + ends + [n], dtype=np.int64)
            staged, _ = check_stage(geo, data, off, mis)
            for b in range(1, 5):
                assert staged[b * tile - 1:b * tile + 2] == b"\n\n\n"
            end_to_end(geo, data, off, mis, 16 - mis & 15, drop=b"")
            end_to_end(geo, data, np.array([0, 3 * tile + 1, n], dtype=np.int64), mis, 3, drop=b"")
            end_to_end(geo, data, np.array([0, n], dtype=np.int64), mis, 9)


def test_empty_strings():
    """runs of empty strings longer than a tile, all-empty input (the staged text is nrec newlines), nrec = 0"""
    for geo in GEOS:
        tile = lib().shim_str_tile(geo)
        run = min(3 * tile + 5, 40000)
        for mis in (0, 7):
            end_to_end(geo, b"", np.zeros(1, np.int64), mis, 1)                          # nrec = 0
            end_to_end(geo, b"", np.zeros(2, np.int64), mis, 1)
            end_to_end(geo, b"", np.zeros(run + 1, np.int64), mis, 5)                    # n = 0, nrec > 0
            off = np.array([0] * run + [3] * run + [10], dtype=np.int64)
            end_to_end(geo, b"abc\nab\0bca", off, mis, 12, drop=b"")


def test_one_byte_strings():
    rng = random.Random(1)
    for geo in GEOS:
        n = 5000 if geo < 3 else 70000
        data = random_data(rng, n)
        for mis, dst_mis in ((0, 0), (5, 11)):
            end_to_end(geo, data, np.arange(n + 1, dtype=np.int64), mis, dst_mis, drop=b"")
            end_to_end(geo, data, np.arange(n + 1, dtype=np.int64), mis, dst_mis, drop=b"ab")


def test_device_geometry():
    """the device's 16 KiB tiles: strings of ~90 bytes (most vectors hold no string end), and strings that span tiles"""
    rng = random.Random(77)
    n = 5 * (16 << 10) + 123
    data = random_data(rng, n)
    for mis, dst_mis in ((0, 0), (9, 3), (15, 8)):
        cuts = sorted(rng.randrange(n + 1) for _ in range(n // 90))
        end_to_end(3, data, np.array([0] + cuts + [n], dtype=np.int64), mis, dst_mis)
        end_to_end(3, data, np.array([0] + cuts + [n], dtype=np.int64), mis, dst_mis, drop=b"", grow=True)
        end_to_end(3, data, np.array([0, 40000, 40001, n], dtype=np.int64), mis, dst_mis, drop=b"")


def test_ranks_beyond_32_bits():
    rng = random.Random(3)
    base0 = (5 << 32) + 12345
    for geo in GEOS:
        data = random_data(rng, 2000)
        end_to_end(geo, data, random_offsets(rng, 2000), 7, 4, base0=base0)


def test_unframe_alone():
    """framed outputs that no scan of a staged text would give: empty outputs, long ones, ends anywhere"""
    rng = random.Random(8)
    for trial in range(200):
        geo = GEOS[trial % 3]
        outs = [bytes(rng.choice(b"xyz\n") for _ in range(rng.choice([0, 0, 1, 3, 20, 150]))) for _ in range(rng.choice([1, 2, 30, 300]))]
        framed = b"".join(o + b"\n" for o in outs)
        located = [0]
        for o in outs:
            located.append(located[-1] + len(o) + 1)
        check_unframe(geo, framed, located, trial % 16)
