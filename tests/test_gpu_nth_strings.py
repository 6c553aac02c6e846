"""Match k of every string on the GPU (include/trre_mi355x.h: trre_nth_device_strings; Program.nth_strings / nth_list) against
the oracle: one entry of every string's list of matches, from either end, with a validity bitmap.  Every expectation is the
oracle's find(s) under the wrapped pattern (tests/find_lib.py), indexed in Python (tests/nth_lib.py).  Each case goes once
through Program.nth_strings, plain and packed, and once through the C ABI with sentinel-filled arrays of exactly the size asked
for — the bytes behind d_out[out_len], the words behind d_out_off[nrec] and behind the bitmap's last word stay as they were.  On
top of the oracle, never instead of it: entry i is match list_off[i] + k (list_off[i + 1] + k for k < 0) of the device's own
find_strings."""
import ctypes
import random

import pytest

import nth_lib
import trre_amd
from find_lib import EXTRA, Finder
from gpu_column_lib import (BFILL, FILL, PAD, assert_prefix, assert_untouched, bitmap_of, blob, carve, dev, lst, off_dev, pack, sequence,
                            soup, to_dev, words)
from span_lib import PAIRS
from test_gpu_filter_strings import POOL          # the filter tests' pool, NULs and empties in it
from trre_amd import api

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, -1, -2, 5, -(1 << 63))
PATTERNS = [prog for prog, _ in PAIRS] + [pat for pat in EXTRA if pat not in [prog for prog, _ in PAIRS]]
ALPHABET = b"abcdefgh ingxt059"
HAND = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
CHUNK = 1024                # strings per workgroup of the plan and offsets passes (records_block.hpp: THREADS * kNthPer)


def raw(p, values, n, offsets, nrec, k, cap, null=False, out=None, ooff=None, valid=None, out_mis=0):
    """the C ABI itself, with sentinel-filled arrays: (rc, *n_valid, *out_len, d_out, d_out_off, d_valid as words); d_out lies
    `out_mis` past a 16-byte boundary; null: the size query, without d_out and d_out_off"""
    if out is None:
        out = carve(cap, out_mis)
    if ooff is None:
        ooff = words(nrec + 1 + PAD)
    if valid is None:
        valid = words((nrec + 63) // 64 + PAD)
    v, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_nth_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, None if null else out.data_ptr(),
                                           cap, None if null else ooff.data_ptr(), valid.data_ptr(), ctypes.byref(v), ctypes.byref(m), None)
    return rc, v.value, m.value, out, ooff, valid


def device_find(p, recs, mis=0):
    data, off = pack(recs)
    out, mo, lo = p.find_strings(to_dev(data, mis), off_dev(off))
    return blob(out), lst(mo), lst(lo)


def check(p, lists, recs, label, ks=KS, mis=0, out_mis=0, found=None):
    """for every k: one call through Program.nth_strings (plain and packed) and one through the C ABI with exact room, against
    the strings' lists; with `found` (the device's find as (out, match_off, list_off)) the cross-check on top"""
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data, mis), off_dev(off)
    got = {}
    for k in ks:
        want = nth_lib.expect(lists, k)
        need, n_valid = len(want[0]), sum(want[2])
        out, oo, valid = p.nth_strings(values, offsets, k)
        assert lst(valid) == want[2], (label, k)
        assert lst(oo) == want[1], (label, k)
        assert blob(out) == want[0], (label, k)
        _, _, packed = p.nth_strings(values, offsets, k, packed=True)
        assert blob(packed) == nth_lib.bitmap(want[2]), (label, k)
        rc, v, m, out2, oo2, valid2 = raw(p, values, len(data), offsets, nrec, k, need, out_mis=out_mis)
        assert (rc, v, m) == (0, n_valid, need), (label, k, rc, v, m, api.lib().trre_last_error())
        assert_prefix(out2, want[0], (label, k))
        assert_prefix(oo2, want[1], (label, k))
        assert bitmap_of(valid2, nrec) == (nth_lib.bitmap(want[2]), [FILL] * PAD), (label, k)
        assert sum(bin(b).count("1") for b in bitmap_of(valid2, nrec)[0]) == v, (label, k)      # *n_valid is the bitmap's population
        if found is not None and k > -(1 << 62):
            fout, mo, lo = found
            for i in range(nrec):
                j = lo[i] + k if k >= 0 else lo[i + 1] + k
                if want[2][i]:
                    assert lo[i] <= j < lo[i + 1] and want[0][want[1][i]:want[1][i + 1]] == fout[mo[j]:mo[j + 1]], (label, k, i)
                else:
                    assert not lo[i] <= j < lo[i + 1], (label, k, i)
        got[k] = want
    return got


def test_patterns_and_symbol_layouts():
    """the find programs of the paired patterns and three more (the backward-state layouts of 4, 8 and 16 bits) on a few hundred
    random short strings and the pool with NULs and empties, every k, at a random misalignment of d_in and d_out, against the
    yardstick and against the device's own find"""
    rng = random.Random(491)
    layouts, n_valid, n_absent, n_valid_empty = set(), 0, 0, 0
    for pat in PATTERNS:
        recs = soup(rng, ALPHABET, 300) + HAND + POOL
        p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)
        mis = rng.randrange(16)
        got = check(p, finder.lines(recs), recs, pat, mis=mis, out_mis=rng.randrange(16), found=device_find(p, recs, mis))
        for k, want in got.items():
            n_valid += sum(want[2])
            n_absent += len(recs) - sum(want[2])
            n_valid_empty += sum(ok and want[1][i] == want[1][i + 1] for i, ok in enumerate(want[2]))
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert layouts == {4, 8, 16}, layouts
    assert n_valid > 2000 and n_absent > 2000 and n_valid_empty >= 100, (n_valid, n_absent, n_valid_empty)


def test_edges():
    """nrec = 0; one empty string, valid-and-empty and absent; the null size query with no bytes; 70 000 empty strings under ':y';
    nrec around a wave and around the plan's chunk; entries of exactly one output tile and of one more byte; an entry over more
    than two tiles; 40 000 empty entries at one output position, then 100 bytes; sources at every offset mod 16 with d_in and
    d_out misaligned by 1 .. 15; a NUL ends the search; k = -1 on strings with 0, 1 and many matches"""
    import torch
    rng = random.Random(492)
    star, plus = (trre_amd.Program(q, "nft", "find") for q in ("x*", "a+"))
    xs, ap = Finder("x*"), Finder("a+")
    # nrec == 0: d_out_off[0] and nothing else
    empty, zero = torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0])
    for k in KS:
        out, oo, valid = star.nth_strings(empty, zero, k)
        assert out.numel() == 0 and lst(oo) == [0] and lst(valid) == []
        assert star.nth_list([], k) == []
        rc, v, m, out, oo, valid = raw(star, empty, 0, zero, 0, k, 0)
        assert (rc, v, m) == (0, 0, 0) and lst(oo) == [0] + [FILL] * PAD and lst(valid) == [FILL] * PAD and bool((out == BFILL).all())
        rc, v, m, _, _, valid = raw(star, empty, 0, zero, 0, k, 0, null=True)
        assert (rc, v, m) == (0, 0, 0) and lst(valid) == [FILL] * PAD
    # one empty string: the one empty match under 'x*' (valid, empty), none under 'a+' (absent)
    got = check(star, [xs(b"")], [b""], "one empty, x*")
    assert got[0] == got[-1] == (b"", [0, 0], [True]) and got[1] == got[-2] == (b"", [0, 0], [False])
    got = check(plus, [ap(b"")], [b""], "one empty, a+")
    assert got[0] == got[-1] == (b"", [0, 0], [False])
    # no entry has bytes with nrec > 0 and the null size query: TRRE_OK, the bitmap written
    rc, v, m, _, _, valid = raw(star, empty, 0, off_dev([0, 0]), 1, 0, 0, null=True)
    assert (rc, v, m) == (0, 1, 0) and lst(valid) == [1] + [FILL] * PAD
    rc, v, m, _, _, valid = raw(plus, empty, 0, off_dev([0, 0]), 1, 0, 0, null=True)
    assert (rc, v, m) == (0, 0, 0) and lst(valid) == [0] + [FILL] * PAD
    # x* on bb and [aie]: on kiwi by hand: an empty output with the bit set is not an absent match
    assert [star.nth_list([b"bb"], k) for k in range(4)] == [[b""], [b""], [b""], [None]]
    assert [trre_amd.Program("[aie]:", "nft", "find").nth_list([b"kiwi", b"xyz"], k) for k in (0, 1, 2)] == [[b"", None], [b"", None], [None, None]]
    # 70 000 empty strings under ':y': 70 000 bytes, every bit set, the bitmap's 1 094 words and its tail
    colon, cy = trre_amd.Program(":y", "nft", "find"), Finder(":y")
    many = [b""] * 70000
    lists = cy.lines(many)
    got = check(colon, lists, many, "70 000 empty, :y", ks=(0, 1))
    assert got[0] == (b"y" * 70000, list(range(70001)), [True] * 70000) and got[1] == (b"", [0] * 70001, [False] * 70000)
    assert len(nth_lib.bitmap(got[0][2])) == 8 * 1094
    # nrec around a wave and around the plan's chunk
    cats, cf = trre_amd.Program("(cat:dog|dog:cat)", "nft", "find"), Finder("(cat:dog|dog:cat)")
    for nrec in (63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
        recs = [rng.choice(POOL) for _ in range(nrec)]
        check(cats, cf.lines(recs), recs, ("nrec", nrec), ks=(0, 1, -1, -2) if nrec < 100 else (0, -2))
    # the output tile edge: an entry of exactly 16 384 and of 16 385 bytes between short neighbours; one over more than two tiles
    # — k = 1 selects "aa", the long entry and "aaa": the long one starts at output position 2 with selected bytes on either side.  With
    # n = 16 384 - 2 - out_mis it ends exactly on the edge of the output's first tile and the next entry starts in the second one
    for n, out_mis in ((16384, 0), (16384, 5), (16385, 0), (16385, 13), (40000, 5), (16382, 0), (16379, 3), (16367, 15)):
        recs = [b"ba aa", b"xa" + b"b" + b"a" * n + b"b aaa", b"", b"a baaa"]
        got = check(plus, ap.lines(recs), recs, ("edge", n, out_mis), ks=(1, -2, 0), out_mis=out_mis, found=device_find(plus, recs))
        assert got[1] == (b"aa" + b"a" * n + b"aaa", [0, 2, 2 + n, 2 + n, 5 + n], [True, True, False, True])
        assert got[-2] == (b"a" + b"a" * n + b"a", [0, 1, 1 + n, 1 + n, 2 + n], [True, True, False, True]) and got[0][0] == b"aaa"
        assert n in (16384, 16385, 40000) or 2 + n + out_mis == 16384
    # a run of empty entries at one output position, longer than a tile's window of offsets, then one with bytes
    recs = [b"b"] * 40000 + [b"x" * 100]
    got = check(star, xs.lines(recs), recs, "40 000 empty entries", ks=(0, -1), out_mis=3)
    assert got[0] == (b"x" * 100, [0] * 40001 + [100], [True] * 40001) and got[-1][0] == b""
    # the sources at every offset mod 16 (a text of 0 .. 15 bytes in front of each), d_in and d_out misaligned by 1 .. 15
    word, wf = trre_amd.Program("[a-z]+", "nft", "find"), Finder("[a-z]+")
    recs = [bytes(rng.choice(b"abcdefghij") for _ in range(lead)) + b" " + bytes(rng.choice(b"klmnopqrst") for _ in range(40)) for lead in range(16)] * 2
    lists = wf.lines(recs)
    assert [len(l[-1]) for l in lists] == [40] * 32 and [len(l[0]) for l in lists[1:16]] == list(range(1, 16))
    for mis in range(1, 16):
        check(word, lists, recs, ("mis", mis), ks=((-1, 0), (-1, 1), (-1, -2))[mis % 3], mis=mis, out_mis=(mis + 7) % 15 + 1)
    # a NUL ends the search
    cd = trre_amd.Program("(cat|dog)", "nft", "find")
    assert [cd.nth_list([b"a cat\0dog"], k) for k in (0, 1, -2)] == [[b"cat"], [None], [None]]
    recs = [b"a cat\0dog", b"\0cat", b"dog\0", b"cat dog\0 cat"]
    got = check(cd, Finder("(cat|dog)").lines(recs), recs, "nuls", found=device_find(cd, recs))
    assert nth_lib.per_string(*got[-1]) == [b"cat", None, b"dog", b"dog"]
    # k = -1 on strings with 0, 1 and many matches
    assert cats.nth_list([b"", b"cow", b"a cat", b"cat dog cat dog dog"], -1) == [None, None, b"dog", b"cat"]
    assert cats.nth_list([b"cat dog cat"], 0) + cats.nth_list([b"cat dog cat"], 1) + cats.nth_list([b"cat dog cat"], -1) == [b"dog", b"cat", b"dog"]


def test_capacity_and_sizes():
    """the null size query, cap = 0 and cap = out_len - 1: TRRE_E_CAPACITY, both sizes and the bitmap right, d_out and d_out_off
    all sentinel; exact room succeeds"""
    rng = random.Random(493)
    p, finder = trre_amd.Program("[0-9]+", "nft", "find"), Finder("[0-9]+")
    recs = [bytes(rng.choice(b"0123456789xy ") for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))) for _ in range(3000)]
    lists = finder.lines(recs)
    data, off = pack(recs)
    nrec = len(recs)
    values, offsets = to_dev(data), off_dev(off)
    for k in (0, 1, -1, -2):
        want = nth_lib.expect(lists, k)
        need, n_valid = len(want[0]), sum(want[2])
        assert need > 0 and (k in (0, -1) or (n_valid >= 300 and nrec - n_valid >= 300)), (k, n_valid)

        def refused(rc, v, m, out, oo, valid):
            assert (rc, v, m) == (api.E_CAPACITY, n_valid, need), (k, rc, v, m)
            assert_untouched(out, k)
            assert_untouched(oo, k)
            assert bitmap_of(valid, nrec) == (nth_lib.bitmap(want[2]), [FILL] * PAD), k

        refused(*raw(p, values, len(data), offsets, nrec, k, 0, null=True))
        refused(*raw(p, values, len(data), offsets, nrec, k, 0))
        refused(*raw(p, values, len(data), offsets, nrec, k, need - 1))
        rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, nrec, k, need)
        assert (rc, v, m) == (0, n_valid, need), (k, rc, v, m)
        assert_prefix(out, want[0], k)
        assert_prefix(oo, want[1], k)
        assert bitmap_of(valid, nrec) == (nth_lib.bitmap(want[2]), [FILL] * PAD), k


def test_errors_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)

    def untouched(rc_want, p, vals=values, offs=offsets, cap=700, k=1, **kw):
        rc, v, m, out, oo, valid = raw(p, vals, len(data), offs, 4, k, cap, **kw)
        assert rc == rc_want and (v, m) == (0, 0), (rc, v, m, api.lib().trre_last_error())
        for name, t in (("out", out), ("ooff", oo), ("valid", valid)):
            if name not in kw:
                assert_untouched(t, name)
        assert lst(offsets) == off and blob(values) == data

    for mode in ("scan", "match", "spans", "sub"):
        untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft", mode))                          # wrong-mode programs
    untouched(api.E_UNSUPPORTED, trre_amd.Program("x:\n", "nft", "find"))                        # prints a newline of its own
    p = trre_amd.Program("[0-9]+:N", "nft", "find")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        for k in (0, -1):
            untouched(api.E_ARG, p, offs=off_dev(bad), k=k)                                      # bad offsets: nothing written
    # every pairwise overlap of the five arrays
    as_words = lambda t: t.view(torch.int64)
    untouched(api.E_ARG, p, out=values[:64], cap=64)                                             # d_in / d_out (no in-place form)
    untouched(api.E_ARG, p, out=values[601:], cap=1)
    untouched(api.E_ARG, p, offs=as_words(values[:40]))                                          # d_in / d_off
    untouched(api.E_ARG, p, ooff=as_words(values[:40]))                                          # d_in / d_out_off
    untouched(api.E_ARG, p, valid=as_words(values[592:600]))                                     # d_in / d_valid
    untouched(api.E_ARG, p, out=offsets.view(torch.uint8), cap=40)                               # d_off / d_out
    untouched(api.E_ARG, p, ooff=offsets)                                                        # d_off / d_out_off
    untouched(api.E_ARG, p, valid=offsets[4:])                                                   # d_off / d_valid
    shared = words(65 + PAD)
    untouched(api.E_ARG, p, out=shared.view(torch.uint8), cap=520, ooff=shared[64:])             # d_out / d_out_off
    untouched(api.E_ARG, p, out=shared.view(torch.uint8)[512:], cap=64, valid=shared[71:])       # d_out / d_valid
    untouched(api.E_ARG, p, ooff=shared, valid=shared[4:])                                       # d_out_off / d_valid
    assert bool((shared == FILL).all())
    untouched(api.E_ARG, p, valid=words(2 + PAD).view(torch.uint8)[4:].view(torch.int32))        # a bitmap that is not 8-byte aligned
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        rc, v, m, out, oo, valid = raw(p, to_dev(bytes(holed)), len(data), offsets, 4, 0, 700)
        assert rc == api.E_ARG and (v, m) == (0, 0) and "newline" in api.lib().trre_last_error().decode()
        for t in (out, oo, valid):
            assert_untouched(t, at)
    # ... and the same strings go through: [12 x 50], [], [12 x 250], [ab]: one match, none, one, none
    rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, 4, 0, 700)
    assert (rc, v, m) == (0, 2, 2) and lst(oo[:5]) == [0, 1, 1, 2, 2] and blob(out[:2]) == b"NN" and lst(valid[:1]) == [5]
    assert bool((out[2:] == BFILL).all()) and bool((oo[5:] == FILL).all()) and bool((valid[1:] == FILL).all())
    rc, v, m, out, oo, valid = raw(p, values, len(data), offsets, 4, 1, 700)
    assert (rc, v, m) == (0, 0, 0) and lst(oo[:5]) == [0] * 5 and lst(valid[:1]) == [0]
    assert bool((out == BFILL).all()) and bool((oo[5:] == FILL).all()) and bool((valid[1:] == FILL).all())


def test_interleaved_with_find_strings_on_one_program():
    """nth_strings, find_strings and nth_strings with another k, back to back on ONE program: a small input, a 330 KiB one, none,
    an input of exactly one tile and of one tile and a byte, the large one again.  The buffers the calls share only grow and every
    pass carves them anew: every result stays right, find's among them"""
    seq = sequence(495, b"a1b", lambda rng, k: bytes(rng.choice(b"ab12 ,") for _ in range(k)))
    p, finder = trre_amd.Program("[0-9]+:N|(a:xyz)", "nft", "find"), Finder("[0-9]+:N|(a:xyz)")
    for label in ("tiny", "large", "none", "one tile", "one tile and a byte", "large again"):
        recs = seq[label]
        lists = finder.lines(recs)
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        flat = [o for l in lists for o in l]
        want_find = (b"".join(flat), pack(flat)[1] if flat else [0], pack([b"." * len(l) for l in lists])[1] if lists else [0])
        for k, k2 in ((1, -1), (0, -2)):
            out, oo, valid = p.nth_strings(values, offsets, k)
            assert (blob(out), lst(oo), lst(valid)) == nth_lib.expect(lists, k), (label, k)
            out, mo, lo = p.find_strings(values, offsets)
            assert (blob(out), lst(mo), lst(lo)) == (want_find[0], list(want_find[1]), list(want_find[2])), (label, k)
            out, oo, valid = p.nth_strings(values, offsets, k2)
            assert (blob(out), lst(oo), lst(valid)) == nth_lib.expect(lists, k2), (label, k2)
