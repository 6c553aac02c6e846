"""The matched-strings passes' per-thread bodies (trre_amd/csrc/records_block.hpp: k_match_verdict, k_match_rank, k_match_final,
k_match_count, k_match_unframe) run on the host by tests/match_shim.cpp — a wave as 64 sequential lanes, its ballot as a loop —
against numpy: the bitmap words, the ranks inside a group, the groups' counts, M_i through the scan of the counts (with a large
base: ranks beyond 2^32), the final offsets and the compaction, composed with the records passes' own count / locate bodies
(tests/records_shim.cpp) around a stand-in scan that prints accepted lines only.  Symbols are given as arrays in the three
layouts the backward pass has (two per byte, one per byte, 16 bits each)."""
import ctypes
import random

import numpy as np

import column_shim_lib
from test_records_shim import lib as rec_lib

GEOS = (0, 1, 2, 3)
N_REV = {4: 16, 8: 200, 16: 700}

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = column_shim_lib.load("match")
        vp, i64, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64
        L.shim_match_group.restype = i64
        L.shim_match_tile.argtypes = [ctypes.c_int]
        L.shim_match_tile.restype = i64
        L.shim_match_verdict.argtypes = [ctypes.c_int, vp, i64, vp, i64, vp, ctypes.c_uint32, u64, vp, vp, vp, vp, vp]
        L.shim_match_final.argtypes = [vp, vp, vp, i64]
        L.shim_match_unframe.argtypes = [ctypes.c_int, vp, i64, i64, i64, vp]
        _lib = L
    return _lib


def T():
    return lib().shim_match_group()


def ptr(a):
    return a.ctypes.data if a.size else None


def lay_out(syms, bits):
    """one symbol per position -> the backward pass's layout"""
    s = np.asarray(syms, dtype=np.uint16)
    if bits == 16:
        return s.view(np.uint8).copy()
    if bits == 8:
        return s.astype(np.uint8)
    s = np.concatenate([s, np.zeros(len(s) & 1, np.uint16)]).astype(np.uint8)
    return (s[0::2] | (s[1::2] << 4)).astype(np.uint8)


def verdicts_of(kind, nrec, rng):
    i = np.arange(nrec)
    if kind == "all":
        return np.ones(nrec, bool)
    if kind == "none":
        return np.zeros(nrec, bool)
    if kind == "alternating":
        return (i & 1) == 1
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == nrec - 1
    if kind == "runs64":                      # rejected runs of 64, aligned to a word
        return (i // 64) % 2 == 1
    if kind == "runs65":                      # ... of 65: every alignment in turn
        return (i // 65) % 2 == 1
    if kind == "runs64_unaligned":
        return ((i + 13) // 64) % 2 == 1
    if kind == "lead":                        # a leading rejected run longer than a group
        return i > T() + 37
    return np.array([rng.random() < 0.5 for _ in range(nrec)], bool)


KINDS = ("all", "none", "alternating", "first", "last", "runs64", "runs65", "runs64_unaligned", "lead", "random")


def check_verdict(bits, off, ok, vbeg, rng, base0=0):
    """one verdict call against numpy; returns (bitmap words, M_i + base0 as out_off, bases)"""
    nrec = len(off) - 1
    n_rev = N_REV[bits]
    accept = np.array([rng.random() < 0.4 for _ in range(n_rev)], np.uint8)
    accept[1], accept[2] = 1, 0                # both kinds exist
    yes, no = np.flatnonzero(accept == 1), np.flatnonzero(accept == 0)
    total = int(off[-1]) + nrec
    syms = np.array([rng.randrange(n_rev) for _ in range(vbeg + total + 2)], np.uint16)       # (noise everywhere else)
    s = vbeg + np.asarray(off[:-1], np.int64) + np.arange(nrec)
    for i in range(nrec):
        syms[s[i]] = rng.choice(yes if ok[i] else no)
    sym = lay_out(syms, bits)
    words, groups = (nrec + 63) // 64, (nrec + T() - 1) // T()
    valid = np.full(max(words, 1), 0x5555555555555555, np.uint64)
    out_off = np.full(nrec + 1, -1, np.int64)
    local = np.zeros(max(nrec, 1), np.int64)
    cnt = np.zeros(max(groups, 1), np.uint64)
    base = np.zeros(groups + 1, np.uint64)
    offa = np.ascontiguousarray(off, dtype=np.int64)
    rc = lib().shim_match_verdict(bits, sym.ctypes.data, vbeg, offa.ctypes.data, nrec, accept.ctypes.data, n_rev, base0, ptr(valid), out_off.ctypes.data,
                                  local.ctypes.data, cnt.ctypes.data, base.ctypes.data)
    assert rc == 0, (bits, nrec, rc)
    ok = np.asarray(ok, bool)
    want_bits = np.zeros(words * 64, np.uint8)
    want_bits[:nrec] = ok
    want_words = np.packbits(want_bits, bitorder="little").view(np.uint64) if words else np.zeros(0, np.uint64)
    assert valid[:words].tolist() == want_words.tolist(), (bits, nrec)                 # (the tail of the last word is zero)
    per_group = [int(ok[g * T():(g + 1) * T()].sum()) for g in range(groups)]
    assert cnt[:groups].tolist() == per_group, (bits, nrec)
    assert base.tolist() == [base0 + int(x) for x in np.concatenate([[0], np.cumsum(per_group)])], (bits, nrec)
    assert local[:nrec].tolist() == [int(ok[i // T() * T():i + 1].sum()) for i in range(nrec)], (bits, nrec)
    assert out_off[0] == -1                                                             # (entry 0 is the locate pass's)
    assert out_off[1:].tolist() == (base0 + np.cumsum(ok)).tolist(), (bits, nrec)
    return valid[:words], out_off, base


def offsets_for(starts):
    """offsets whose strings' first staged bytes are at `starts` (0 first, strictly increasing); the last string is 3 bytes"""
    assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))
    lens = [b - a - 1 for a, b in zip(starts, starts[1:])] + [3]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def sizes():
    t = T()
    return [0, 1, 63, 64, 65, 127, 128, 129, t - 1, t, t + 1, 3 * t + 5]


def test_geometry():
    assert T() == 256 and [lib().shim_match_tile(g) for g in GEOS] == [64, 128, 1024, 16 << 10]


def test_verdicts_every_size_pattern_and_layout():
    rng = random.Random(5)
    for bits in (4, 8, 16):
        for nrec in sizes():
            for kind in KINDS:
                lens = [rng.choice([0, 0, 1, 2, 5]) for _ in range(nrec)]
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                check_verdict(bits, off, verdicts_of(kind, nrec, rng), rng.choice([0, 0, 1, 7, 15]), rng)


def test_first_bytes_at_nibbles_pieces_and_tile_edges():
    """s_i odd and even; at 63, 64, 127, 128 mod 128 (the sweep's pieces); at the staged text's 16 KiB tile edges - 1, 0, + 1"""
    rng = random.Random(6)
    tile = 16 << 10
    starts = [0, 1, 2, 5, 8, 63, 64, 127, 128, 191, 192, 255, 256, 300, 301]
    for b in (1, 2, 3):
        starts += [b * tile - 1, b * tile, b * tile + 1, b * tile + 63, b * tile + 64, b * tile + 127, b * tile + 128]
    off = offsets_for(starts)
    for bits in (4, 8, 16):
        for vbeg in (0, 1):
            for kind in ("all", "none", "alternating", "random"):
                check_verdict(bits, off, verdicts_of(kind, len(off) - 1, rng), vbeg, rng)


def test_ranks_beyond_32_bits():
    rng = random.Random(7)
    base0 = (5 << 32) + 12345
    for bits in (4, 8, 16):
        nrec = 3 * T() + 5
        off = np.arange(nrec + 1, dtype=np.int64) * 2
        check_verdict(bits, off, verdicts_of("random", nrec, rng), 3, rng, base0=base0)


def scan_like(rec):
    """the stand-in program: a string of digits is accepted and printed with every 7 doubled, the empty string is accepted too"""
    return rec.replace(b"7", b"77") if all(48 <= c <= 57 for c in rec) else None


def end_to_end(geo, recs, dst_mis, rng, bits=8):
    nrec = len(recs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    outs = [scan_like(r) for r in recs]
    ok = np.array([o is not None for o in outs], bool)
    valid, out_off, base = check_verdict(bits, off, ok, rng.randrange(16), rng)
    framed = b"".join(o + b"\n" for o in outs if o is not None)
    m, matched = len(framed), int(ok.sum())
    want_off = [0] + np.cumsum([len(o) if o is not None else 0 for o in outs]).tolist()
    want = b"".join(o for o in outs if o is not None)
    if nrec == 0:
        return
    if m == 0:                                 # (the runtime writes zeros without a launch)
        assert matched == 0 and set(want_off) == {0}
        return
    src = np.frombuffer(framed, dtype=np.uint8).copy()
    out_off[0] = 0
    assert rec_lib().shim_rec_locate(geo, src.ctypes.data, m, 0, out_off.ctypes.data, nrec, 0) == 0
    assert out_off[-1] == m                    # (trailing rejected strings share the last accepted one's rank)
    assert lib().shim_match_final(ptr(valid), base.ctypes.data, out_off.ctypes.data, nrec) == 0
    assert out_off.tolist() == want_off, (geo, nrec)
    out = np.zeros(max(m - matched, 1), np.uint8)
    rc = lib().shim_match_unframe(geo, src.ctypes.data, m, matched, dst_mis, out.ctypes.data)
    assert rc == 0, (geo, dst_mis, rc)
    assert out[:m - matched].tobytes() == want, (geo, dst_mis)


def make_recs(rng, ok, lens=(0, 1, 2, 3, 9, 40)):
    recs = []
    for good in ok:
        n = rng.choice(lens)
        r = bytes(rng.choice(b"0123456789777") for _ in range(n))
        if not good:
            r = r[:n // 2] + b"x" + r[n // 2:]
        recs.append(r)
    return recs


def test_end_to_end_sizes_and_patterns():
    rng = random.Random(8)
    for trial, nrec in enumerate(sizes()):
        for k, kind in enumerate(KINDS):
            geo = GEOS[(trial + k) % 3]
            end_to_end(geo, make_recs(rng, verdicts_of(kind, nrec, rng)), (trial * 5 + k) % 16, rng, bits=(4, 8, 16)[k % 3])


def test_every_destination_misalignment():
    rng = random.Random(9)
    recs = make_recs(rng, verdicts_of("random", 700, rng))
    for geo in (0, 2):
        for dst_mis in range(16):
            end_to_end(geo, recs, dst_mis, rng)


def test_all_rejected_and_runs_of_empty_strings():
    rng = random.Random(10)
    for geo in GEOS:
        end_to_end(geo, [b"x"] * 1000, 3, rng)                                  # out_len 0, every offset 0
        end_to_end(geo, [b""] * (3 * T() + 5), 5, rng)                          # every string empty and accepted: m = nrec newlines
        end_to_end(geo, [b""] * 700 + [b"x"] * 700 + [b"17"] + [b""] * 70, 9, rng)


def test_device_geometry():
    """the device's 16 KiB tiles: outputs of ~40 bytes, a third of the strings rejected; outputs that span tiles"""
    rng = random.Random(11)
    ok = np.array([rng.random() < 0.66 for _ in range(3000)], bool)
    recs = make_recs(rng, ok, lens=(10, 40, 90))
    for dst_mis in (0, 3, 15):
        end_to_end(3, recs, dst_mis, rng, bits=4)
    big = [bytes(rng.choice(b"0123456789") for _ in range(40000)), b"x" * 5000, b"", bytes(rng.choice(b"789") for _ in range(20000))]
    end_to_end(3, big, 7, rng, bits=16)


def test_stand_alone_program_under_sanitizers():
    """match_shim.cpp with its own main, built with -fsanitize=address,undefined, over nrec around the words and groups, seven
    verdict patterns, the three symbol layouts and the destination misalignments: a process of its own, on the CPU"""
    r = column_shim_lib.sanitized("match")
    assert r.returncode == 0 and b"shapes ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
