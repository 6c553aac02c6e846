"""Found strings on the GPU (include/trre_mi355x.h: trre_find_device_strings; Program.find_strings / find_list) against the
oracle: every match of every string — the outputs of the scan loop's successful attempts — as one list per string.  Every
expectation is the oracle's under the wrapped pattern (tests/find_lib.py), in the run.  Each case goes once through
Program.find_strings and once through the C ABI with sentinel-filled outputs of exactly the size asked for: the bytes behind
*out_len, the words behind d_match_off[n_matches] and behind d_list_off[nrec] stay as they were."""
import ctypes
import random

import pytest

import find_lib
import trre_amd
from find_lib import EXTRA, Finder, lines_of
from gpu_column_lib import BFILL as SENTINEL
from gpu_column_lib import FILL, PAD, assert_prefix, assert_untouched, blob, dev, lst, off_dev, pack, to_dev
from gpu_column_lib import words as filled      # (words() here makes strings of words)
from oracle_lib import OracleError
from trre_amd import api

pytestmark = pytest.mark.gpu

def expect(finder, recs):
    """the specification: (bytes, match offsets, list offsets)"""
    per = finder.lines(recs) if len(recs) > 1 else [finder(r) for r in recs]
    flat = [o for w in per for o in w]
    data, moff = pack(flat)
    _, loff = pack([b"." * len(w) for w in per])
    return data, moff, loff


def raw(p, values, n, offsets, nrec, out_ptr, cap, match_cap, moff=None, null_moff=False):
    """the C ABI itself, with sentinel-filled offset arrays: (rc, *out_len, *n_matches, d_match_off, d_list_off)"""
    if moff is None:
        moff = filled(match_cap + 1 + PAD)
    loff = filled(nrec + 1 + PAD)
    m, k = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_find_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, out_ptr, cap,
                                            None if null_moff else moff.data_ptr(), match_cap, loff.data_ptr(), ctypes.byref(k), ctypes.byref(m), None)
    return rc, m.value, k.value, moff, loff


def check(p, finder, recs, label, out_mis=0):
    """one call through Program.find_strings and one through the C ABI with exact room, against the oracle"""
    import torch
    want = expect(finder, recs)
    need, found, nrec = len(want[0]), len(want[1]) - 1, len(recs)
    data, off = pack(recs)
    values, offsets = to_dev(data), off_dev(off)
    out, mo, lo = p.find_strings(values, offsets)
    assert blob(out) == want[0], label
    assert lst(mo) == want[1], label
    assert lst(lo) == want[2], label
    big = torch.full((out_mis + need + 64,), SENTINEL, dtype=torch.uint8, device=dev())
    rc, m, k, mo2, lo2 = raw(p, values, len(data), offsets, nrec, big.data_ptr() + out_mis, need, found)
    assert (rc, m, k) == (0, need, found), (label, rc, m, k, api.lib().trre_last_error())
    assert big[out_mis:out_mis + m].cpu().numpy().tobytes() == want[0], label
    assert bool((big[:out_mis] == SENTINEL).all()) and bool((big[out_mis + m:] == SENTINEL).all()), label
    assert_prefix(mo2, want[1], label)
    assert_prefix(lo2, want[2], label)
    return want


def test_golden_vectors():
    """the first 2 000 lines of every usable golden NFT vector as strings, and three more patterns (a byte per symbol, the last
    nibble-packed size, 16-bit symbols): bytes, match offsets, list offsets, n_matches and out_len are the oracle's; a program
    that prints a '\\n' of its own is refused; every vector the reference does not survive gives TRRE_E_DIVERGES with out_len = 0"""
    import torch
    rng = random.Random(51)
    usable, dead, _, _ = find_lib.vectors()
    soup = [bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randrange(0, 30))) for _ in range(300)]
    cases = [(pat, name, lines_of(data)[:2000]) for pat, name, data in usable]
    cases += [(pat, "extra", lines_of(usable[0][2])[:50] + soup + [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd"]) for pat in EXTRA]
    progs, compared, newline_printing, no_tables, layouts, n_matches = {}, 0, 0, 0, set(), 0
    for pat, name, recs in cases:
        if pat not in progs:
            try:
                progs[pat] = (trre_amd.Program(pat, "nft", "find"), Finder(pat))
            except trre_amd.TrreError as e:
                assert e.code == api.E_UNSUPPORTED and "guided tables" in e.message, (pat, e)
                progs[pat] = None
        if progs[pat] is None:
            no_tables += 1
            continue
        p, finder = progs[pat]
        assert p.info.kernel == trre_amd.KERNEL_GUIDED_GEN
        try:
            want = check(p, finder, recs, (pat, name))
        except trre_amd.TrreError as e:
            assert e.code == api.E_UNSUPPORTED and "newline" in e.message, (pat, name, e)
            newline_printing += 1
            continue
        compared += 1
        n_matches += len(want[1]) - 1
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert compared + newline_printing + no_tables == len(cases) and compared > 400 and no_tables < 10, (compared, newline_printing, no_tables)
    assert layouts == {4, 8, 16} and n_matches > 10000, (layouts, n_matches)
    assert len(dead) == 13
    out = torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device=dev())
    for pat, name, data in dead:
        recs = lines_of(data)
        values, offsets = to_dev(b"".join(recs)), off_dev(pack(recs)[1])
        rc, m, k, _, _ = raw(trre_amd.Program(pat, "nft", "find"), values, values.numel(), offsets, len(recs), out.data_ptr(), out.numel(), 1 << 16)
        assert rc == api.E_DIVERGES and m == 0, (pat, name, rc, m)
        assert "stack max capacity" in api.lib().trre_last_error().decode(), (pat, name)


def test_sizes_and_string_edges():
    """nrec around the waves and workgroups of the string passes; all strings empty; no string with a match; a string that starts
    with a NUL; a NUL in mid-string; nrec = 0"""
    import torch
    rng = random.Random(52)
    pat = "[0-9]+:N|(cat:dog)"
    p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
    pool = [b"", b"7", b"a12b345", b"cat", b"the cat 9", b"xyz", b"\0 12", b"12\0 34 cat", b"1" * 40, b"catcatcat 0"]
    assert finder(b"\0 12") == [] and finder(b"12\0 34 cat") == [b"N"] and finder(b"a12b345") == [b"N", b"N"]
    for nrec in (1, 63, 64, 65, 255, 256, 257):
        check(p, finder, [rng.choice(pool) for _ in range(nrec)], (pat, nrec))
        check(p, finder, [b""] * nrec, (pat, nrec, "empty"))
        want = check(p, finder, [rng.choice([b"xyz", b"", b"\0 12", b"ca t"]) for _ in range(nrec)], (pat, nrec, "no match"))
        assert want[0] == b"" and want[1] == [0] and want[2] == [0] * (nrec + 1)
    # nrec == 0: d_list_off[0] = 0, d_match_off[0] = 0 if it is not null
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    out, mo, lo = p.find_strings(empty, zero)
    assert out.numel() == 0 and mo.cpu().tolist() == [0] and lo.cpu().tolist() == [0]
    assert p.find_list([]) == []
    rc, m, k, mo, lo = raw(p, empty, 0, zero, 0, None, 0, 0)
    assert (rc, m, k) == (0, 0, 0) and mo.cpu().tolist() == [0] + [FILL] * PAD and lo.cpu().tolist() == [0] + [FILL] * PAD
    rc, m, k, mo, lo = raw(p, empty, 0, zero, 0, None, 0, 0, null_moff=True)
    assert (rc, m, k) == (0, 0, 0) and lo.cpu().tolist() == [0] + [FILL] * PAD


def words(rng, total):
    recs, size = [], 0
    while size < total:
        r = b" ".join(bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(1, 12))) for _ in range(rng.randrange(0, 30)))
        recs.append(r)
        size += len(r)
    return recs


def test_tile_edges():
    """'x*' on strings without x: every match is empty, the framed text is all newlines and crosses a 16 KiB tile — a tile owes
    16 384 offsets; '[a-z]+' on 40 KiB of words: matches straddle the staged and framed tile edges; '(a:xyzxyzxyzxyz)' on 3 000 a
    in one string: one string's list spans three framed tiles; '(cat:dog|dog:cat)'; d_out at misalignments 0, 1, 7, 15"""
    rng = random.Random(53)
    dense = [bytes(rng.choice(b"abc ") for _ in range(rng.randrange(40, 95))) for _ in range(300)]
    assert 19000 < sum(map(len, dense)) < 21000
    animals = [b" ".join(rng.choice([b"cat", b"dog", b"cow", b"catdog", b"do", b""]) for _ in range(rng.randrange(0, 12))) for _ in range(700)]
    for pat, recs in (("x*", dense), ("[a-z]+", words(rng, 40 << 10)), ("(a:xyzxyzxyzxyz)", [b"b", b"a" * 3000, b"", b"ba"]), ("(cat:dog|dog:cat)", animals)):
        p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
        for mis in (0, 1, 7, 15):
            want = check(p, finder, recs, (pat, mis), out_mis=mis)
        if pat == "x*":
            assert want[0] == b"" and len(want[1]) - 1 == sum(map(len, dense)) + len(dense) > 16384 and set(want[1]) == {0}
        if pat == "(a:xyzxyzxyzxyz)":
            assert want[2] == [0, 0, 3000, 3000, 3001] and len(want[0]) + len(want[1]) - 1 > 2 * 16384


def test_in_place():
    """d_in == d_out with '[a-z]+' on 40 KiB of words: the result of separate buffers, the sentinels around intact; after
    TRRE_E_CAPACITY the input is intact"""
    import torch
    rng = random.Random(54)
    pat = "[a-z]+"
    p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
    recs = words(rng, 40 << 10)
    want = expect(finder, recs)
    need, found, nrec = len(want[0]), len(want[1]) - 1, len(recs)
    data, off = pack(recs)
    assert 0 < need <= len(data)
    offsets = off_dev(off)
    for base in (0, 5):
        t = torch.full((base + len(data) + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
        t[base:base + len(data)] = to_dev(data)
        v = t[base:base + len(data)]
        rc, m, k, mo, lo = raw(p, v, len(data), offsets, nrec, v.data_ptr(), need - 1, found)
        assert (rc, m, k) == (api.E_CAPACITY, need, found)
        assert blob(v) == data and bool((mo == FILL).all())
        assert lo[:nrec + 1].cpu().numpy().tolist() == want[2]
        rc, m, k, mo, lo = raw(p, v, len(data), offsets, nrec, v.data_ptr(), len(data), found)
        assert (rc, m, k) == (0, need, found)
        assert t[base:base + need].cpu().numpy().tobytes() == want[0]
        assert t[base + need:base + len(data)].cpu().numpy().tobytes() == data[need:]          # (nothing behind *out_len is written)
        assert bool((t[:base] == SENTINEL).all()) and bool((t[base + len(data):] == SENTINEL).all())
        assert mo[:found + 1].cpu().numpy().tolist() == want[1] and lo[:nrec + 1].cpu().numpy().tolist() == want[2]


def test_capacity_protocol():
    """the size query (cap = 0, match_cap = 0, both null): TRRE_E_CAPACITY, both sizes, valid list offsets; cap one short with
    match_cap exact, match_cap one short with cap exact: the same, d_out and d_match_off untouched; exact room for both succeeds"""
    import torch
    rng = random.Random(55)
    for pat, alpha in (("[0-9]+:N", b"0123456789xy "), ("(a:xyz|b)+", b"aabc"), ("x*", b"xxy")):
        p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
        recs = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
        want = expect(finder, recs)
        need, found, nrec = len(want[0]), len(want[1]) - 1, len(recs)
        assert need > 0 and found > nrec // 2, pat
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        rc, m, k, _, lo = raw(p, values, len(data), offsets, nrec, None, 0, 0, null_moff=True)
        assert (rc, m, k) == (api.E_CAPACITY, need, found), (pat, rc, m, k)
        assert_prefix(lo, want[2], pat)
        out = torch.full((need + 64,), SENTINEL, dtype=torch.uint8, device=dev())
        for cap, mcap in ((need - 1, found), (need, found - 1)):
            rc, m, k, mo, lo = raw(p, values, len(data), offsets, nrec, out.data_ptr(), cap, mcap)
            assert (rc, m, k) == (api.E_CAPACITY, need, found), (pat, cap, mcap, rc, m, k)
            assert_untouched(out, (pat, cap, mcap))
            assert_untouched(mo, (pat, cap, mcap))
            assert lo[:nrec + 1].cpu().numpy().tolist() == want[2], pat
        rc, m, k, mo, lo = raw(p, values, len(data), offsets, nrec, out.data_ptr(), need, found)
        assert (rc, m, k) == (0, need, found), (pat, rc, m, k)
        assert_prefix(out, want[0], pat)
        assert_prefix(mo, want[1], pat)


def test_refusals_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev())

    def untouched(rc_want, p, vals=values, offs=offsets, **kw):
        rc, m, k, mo, lo = raw(p, vals, len(data), offs, 4, out.data_ptr(), out.numel(), 64, **kw)
        assert rc == rc_want and m == 0 and k == 0, (rc, m, k, api.lib().trre_last_error())
        for name, t in (("out", out), ("loff", lo), ("moff", mo)):
            if name not in kw:
                assert_untouched(t, name)

    untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft"))                                    # a scan-mode program
    untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", "match"))
    untouched(api.E_UNSUPPORTED, trre_amd.Program("x:\n", "nft", "find"))                        # prints a newline of its own
    p = trre_amd.Program("[0-9]+:N", "nft", "find")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        untouched(api.E_ARG, p, offs=off_dev(bad))                                               # bad offsets: nothing written
    untouched(api.E_ARG, p, moff=out[8:8 + 8 * 80].view(torch.int64))                            # d_match_off inside d_out
    untouched(api.E_ARG, p, moff=offsets)                                                        # ... on the offsets
    assert offsets.cpu().tolist() == off
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        untouched(api.E_ARG, p, vals=to_dev(bytes(holed)))
        assert "newline" in api.lib().trre_last_error().decode()
    # a find program given to the other calls
    with pytest.raises(trre_amd.TrreError) as e:
        p.scan_strings(values, offsets)
    assert e.value.code == api.E_ARG
    with pytest.raises(trre_amd.TrreError) as e:
        p.match_strings(values, offsets)
    assert e.value.code == api.E_ARG
    m = ctypes.c_size_t(5)
    assert api.lib().trre_scan_device(p._h, values.data_ptr(), len(data), out.data_ptr(), out.numel(), ctypes.byref(m), None) == api.E_ARG and m.value == 0
    assert bool((out == SENTINEL).all())
    # ... and the same strings go through
    rc, m, k, mo, lo = raw(p, values, len(data), offsets, 4, out.data_ptr(), out.numel(), 64)
    assert (rc, m, k) == (0, 2, 2) and lo[:5].cpu().tolist() == [0, 1, 1, 2, 2] and mo[:3].cpu().tolist() == [0, 1, 2]
    assert out[:2].cpu().numpy().tobytes() == b"NN" and bool((out[2:] == SENTINEL).all())


def test_find_list():
    pat = "[0-9]+:N|(cat:dog)"
    p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
    recs = [b"2024", b"", b"cat", b"catcat 7", b"dog", b"12a3", b"cat\0dog 5", b"x"]
    want = [finder(r) for r in recs]
    assert [] in want and [b"N", b"N"] in want and [b"dog", b"dog", b"N"] in want, want
    assert p.find_list(recs) == want
    assert trre_amd.Program("x*", "nft", "find").find_list([b"bb", b""]) == [[b"", b"", b""], [b""]]
