"""Matched strings on the GPU (include/trre_mi355x.h: trre_match_device_strings; Program.match_strings / match_list) against
the oracle: string i is the content of one line, valid[i] says whether `trre -m` prints anything for it, its output is what it
prints without the framing newline, out_offsets[i] where that starts.  Every expectation is the oracle's, in the run."""
import ctypes
import os
import random
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_lib
import trre_amd
from gpu_column_lib import dev, off_dev, pack, to_dev
from oracle_lib import Oracle, OracleError
from trre_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SENTINEL = 0xA5
THREADS = 16
WIDE = "[a-h]{8}(a|b)[a-z ]*"                              # this build: 772 backward states, 16-bit symbols
EXTRA = [".*(cat:dog).*(a|b){4}", "(a|b)*a(a|b){5}", WIDE]  # ... 19 (a byte per symbol), 16 (the last nibble-packed size)


class Memo:
    """the oracle's m_i = M(rec + b"\\n"), once per distinct string"""

    def __init__(self, pat):
        self.o = Oracle(pat, "nft")
        self.seen = {}

    def __call__(self, rec):
        if rec not in self.seen:
            self.seen[rec] = self.o.match(rec + b"\n")
        return self.seen[rec]


def expect(memo, recs):
    """the specification: (bytes, offsets, verdicts)"""
    per = [memo(r) for r in recs]
    data, off = pack([m[:-1] for m in per])
    return data, off, [m != b"" for m in per]


def bitmap_of(verdicts):
    words = (len(verdicts) + 63) // 64
    bits = np.zeros(words * 64, np.uint8)
    bits[:len(verdicts)] = verdicts
    return np.packbits(bits, bitorder="little").tobytes()


def raw(p, values, n, offsets, nrec, out_ptr, cap, fill=-7, valid=None, valid_shift=0):
    """the C ABI itself, with sentinel-filled outputs: (rc, *out_len, *n_matched, out_offsets, the bitmap's words)"""
    import torch
    oo = torch.full((nrec + 1,), fill, dtype=torch.int64, device=dev())
    if valid is None:
        valid = torch.full(((nrec + 63) // 64 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev())
    m, k = ctypes.c_size_t(77), ctypes.c_size_t(77)
    rc = api.lib().trre_match_device_strings(p._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, out_ptr, cap, oo.data_ptr(),
                                             valid.data_ptr() + valid_shift, ctypes.byref(k), ctypes.byref(m), None)
    return rc, m.value, k.value, oo, valid


def check(p, memo, recs, label):
    """one call through Program.match_strings (both forms of valid) and one through the C ABI, against the oracle"""
    want = expect(memo, recs)
    data, off = pack(recs)
    values, offsets = to_dev(data), off_dev(off)
    out, oo, valid = p.match_strings(values, offsets)
    assert out.cpu().numpy().tobytes() == want[0], label
    assert oo.cpu().numpy().tolist() == want[1], label
    assert valid.cpu().numpy().tolist() == want[2], label
    import torch
    big = torch.full((len(want[0]) + 64,), SENTINEL, dtype=torch.uint8, device=dev())
    rc, m, k, oo2, words = raw(p, values, len(data), offsets, len(recs), big.data_ptr(), len(want[0]))
    assert (rc, m, k) == (0, len(want[0]), sum(want[2])), (label, rc, m, k)
    nw = (len(recs) + 63) // 64
    assert words[:nw].cpu().numpy().tobytes() == bitmap_of(want[2]), label                       # (the last word's tail is zero)
    assert bool((words[nw:] == 0x5A5A5A5A5A5A5A5A).all()), label
    assert big[:m].cpu().numpy().tobytes() == want[0] and bool((big[m:] == SENTINEL).all()), label
    assert oo2.cpu().numpy().tolist() == want[1], label
    return want


def test_golden_match_vectors_every_family():
    """every golden match vector's lines as strings, and three more patterns (a byte per symbol, the last nibble-packed size,
    16-bit symbols), under AUTO and every family the program allows: bytes, offsets, bitmap and n_matched equal the per-string
    oracle; the backtracking family is refused; a vector the reference does not survive gives TRRE_E_DIVERGES with out_len = 0; a
    program that prints a '\\n' of its own is refused"""
    rng = random.Random(31)
    cases = [(pat, name, data) for pat, name, data, exp in golden_lib.match_cases()]
    some = cases[0][2]
    soup = b"\n".join(bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randrange(0, 30))) for _ in range(300)) + b"\n"
    cases += [(pat, "extra", some + soup) for pat in EXTRA]
    n_cases = compared = diverged = newline_printing = n_fam = 0
    layouts = set()
    progs = {}
    for pat, name, data in cases:
        n_cases += 1
        if pat not in progs:
            progs[pat] = (trre_amd.Program(pat, "nft", "match"), Memo(pat))
        p, memo = progs[pat]
        recs = data.split(b"\n")
        if recs and recs[-1] == b"":
            recs.pop()
        try:
            want = expect(memo, recs)
        except OracleError:
            want = None
        values, offsets = to_dev(b"".join(recs)), off_dev(pack(recs)[1])
        refused = False
        for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
            p.set_kernel(fam)
            try:
                out, oo, valid = p.match_strings(values, offsets)
            except trre_amd.TrreError as e:
                if e.code == api.E_UNSUPPORTED and "newline" in e.message:
                    refused = True
                    break
                if fam == trre_amd.KERNEL_BACKTRACK:
                    assert e.code == api.E_UNSUPPORTED and "guided tables" in e.message, (pat, name, e)
                    continue
                assert want is None and e.code == api.E_DIVERGES, (pat, name, trre_amd.KERNEL_NAMES[fam], e)
                continue
            assert fam != trre_amd.KERNEL_BACKTRACK
            assert want is not None, (pat, name, trre_amd.KERNEL_NAMES[fam], "diverges in the reference")
            assert out.cpu().numpy().tobytes() == want[0], (pat, name, trre_amd.KERNEL_NAMES[fam])
            assert oo.cpu().numpy().tolist() == want[1], (pat, name, trre_amd.KERNEL_NAMES[fam])
            assert valid.cpu().numpy().tolist() == want[2], (pat, name, trre_amd.KERNEL_NAMES[fam])
            n_fam += fam != trre_amd.KERNEL_AUTO
        p.set_kernel(trre_amd.KERNEL_AUTO)
        if refused:
            newline_printing += 1
        elif want is None:
            import torch
            out = torch.empty(len(data) + 4096, dtype=torch.uint8, device=dev())
            rc, m, k, _, _ = raw(p, values, values.numel(), offsets, len(recs), out.data_ptr(), out.numel())
            assert rc == api.E_DIVERGES and m == 0, (pat, name, rc, m)
            diverged += 1
        else:
            check(p, memo, recs, (pat, name))                       # (the bitmap and n_matched, through the C ABI)
            compared += 1
            n_rev = p.info.guided_rev_states
            layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
    assert trre_amd.Program(WIDE, "nft", "match").info.guided_rev_states > 256
    assert compared + diverged + newline_printing == n_cases == 126, (compared, diverged, newline_printing, n_cases)
    assert compared > 90 and n_fam >= compared and diverged > 0 and layouts == {4, 8, 16}, (compared, n_fam, diverged, layouts)


def shapes():
    t = 256                                                    # strings per workgroup of the verdict pass
    return [1, 63, 64, 65, 127, 128, 129, t - 1, t, t + 1, 3 * t + 5]


def verdict_kinds(nrec, rng):
    i = np.arange(nrec)
    return {"all": np.ones(nrec, bool), "none": np.zeros(nrec, bool), "alternating": (i & 1) == 1, "first": i == 0, "last": i == nrec - 1,
            "runs64": (i // 64) % 2 == 1, "runs65": (i // 65) % 2 == 1, "runs64_unaligned": ((i + 13) // 64) % 2 == 1, "lead": i > 256 + 37,
            "random": np.array([rng.random() < 0.5 for _ in range(nrec)], bool)}


def test_sizes_and_verdict_patterns():
    """nrec around the bitmap's words and the verdict pass's workgroups, every verdict pattern of the host shim's tests, under a
    program that rejects the empty string ('[0-9]+:N') and one that accepts it ('(a:x)*'); nrec = 0"""
    import torch
    rng = random.Random(32)
    for pat, good, bad in (("[0-9]+:N", [b"7", b"2024", b"0" * 40], [b"", b"x", b"12a", b"a12"]), ("(a:x)*", [b"", b"a", b"aaaa", b"a" * 33], [b"b", b"ab", b"aab"])):
        p, memo = trre_amd.Program(pat, "nft", "match"), Memo(pat)
        assert all(memo(g) != b"" for g in good) and all(memo(b) == b"" for b in bad), pat
        for nrec in shapes():
            for kind, ok in verdict_kinds(nrec, rng).items():
                recs = [rng.choice(good if x else bad) for x in ok]
                want = check(p, memo, recs, (pat, nrec, kind))
                assert want[2] == ok.tolist()
        out, oo, valid = p.match_strings(torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0]))
        assert out.numel() == 0 and oo.cpu().tolist() == [0] and valid.numel() == 0


def test_runs_of_empty_strings():
    """thousands of empty strings (n = 0: the staged text is nrec newlines) under a program that accepts the empty line, one that
    rejects it and one that prints for it; runs of them between other strings"""
    for pat, rec_out in (("(a:x)*", b""), ("a+:x", None), (":x", b"x")):
        p, memo = trre_amd.Program(pat, "nft", "match"), Memo(pat)
        assert memo(b"") == (b"" if rec_out is None else rec_out + b"\n"), pat
        for nrec in (1, 64, 1000, 40000):
            want = check(p, memo, [b""] * nrec, (pat, nrec))
            assert want[2] == [rec_out is not None] * nrec
        check(p, memo, [b""] * 700 + [b"a"] * 3 + [b"b"] * 700 + [b""] * 300 + [b"aa"], pat)


def test_million_one_byte_strings():
    """2^20 + 1 one-byte strings, accepted and rejected in turn"""
    import torch
    n = (1 << 20) + 1
    memo = Memo("[0-9]+:N")
    assert memo(b"1") == b"N\n" and memo(b"x") == b""
    data = np.where(np.arange(n) % 2 == 0, ord("1"), ord("x")).astype(np.uint8)
    x = torch.from_numpy(data).to(dev())
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev())
    out, oo, valid = trre_amd.Program("[0-9]+:N", "nft", "match").match_strings(x, offs)
    ok = np.arange(n) % 2 == 0
    assert out.cpu().numpy().tobytes() == b"N" * int(ok.sum())
    assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], np.cumsum(ok)]))
    assert np.array_equal(valid.cpu().numpy(), ok)


def test_capacity_query_and_retry():
    """cap = 0 with d_out = NULL: TRRE_E_CAPACITY, *out_len and *n_matched the oracle's, the bitmap right; the retry with exactly
    *out_len succeeds; one byte less fails and leaves a sentinel-filled d_out untouched"""
    import torch
    rng = random.Random(33)
    def soup(alpha):
        return lambda: bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 2, 3, 8, 30])))

    def catdog():
        return rng.choice([b"", b"x", b"the "]) + rng.choice([b"cat", b"ca", b"dog"]) + rng.choice([b"", b" sat "]) + bytes(rng.choice(b"ab") for _ in range(rng.choice([3, 4, 4, 9])))
    for pat, gen in (("[0-9]+:N", soup(b"0123456789x")), ("(a:x)*", soup(b"aaab")), (".*(cat:dog).*(a|b){4}", catdog), ("(a:xyz|b)*", soup(b"abbc"))):
        p, memo = trre_amd.Program(pat, "nft", "match"), Memo(pat)
        recs = [gen() for _ in range(5000)]
        want = expect(memo, recs)
        need, matched = len(want[0]), sum(want[2])
        assert need > 0 and 0 < matched < len(recs), pat
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        nw = (len(recs) + 63) // 64
        rc, m, k, oo, words = raw(p, values, len(data), offsets, len(recs), None, 0)
        assert (rc, m, k) == (api.E_CAPACITY, need, matched), (pat, rc, m, k)
        assert words[:nw].cpu().numpy().tobytes() == bitmap_of(want[2]), pat
        out = torch.full((need + 64,), SENTINEL, dtype=torch.uint8, device=dev())
        rc, m, k, oo, words = raw(p, values, len(data), offsets, len(recs), out.data_ptr(), need - 1)
        assert (rc, m, k) == (api.E_CAPACITY, need, matched), (pat, rc, m, k)
        assert bool((out == SENTINEL).all()), pat
        assert words[:nw].cpu().numpy().tobytes() == bitmap_of(want[2]), pat
        rc, m, k, oo, words = raw(p, values, len(data), offsets, len(recs), out.data_ptr(), need)
        assert (rc, m, k) == (0, need, matched), (pat, rc, m, k)
        assert out[:need].cpu().numpy().tobytes() == want[0] and bool((out[need:] == SENTINEL).all()), pat
        assert oo.cpu().numpy().tolist() == want[1], pat


def test_in_place():
    """d_in == d_out (at offsets 0 and 5 of a buffer): the result of separate buffers, the sentinels around intact; after
    TRRE_E_CAPACITY the input is intact"""
    import torch
    rng = random.Random(34)
    grew = 0
    for pat, alpha, rare in (("(a:xyz|b)*", b"aab", b"abc"), ("[0-9]+:N", b"0123456789", b"12x"), ("(a:x)*", b"a", b"aaab")):
        p, memo = trre_amd.Program(pat, "nft", "match"), Memo(pat)
        recs = []
        for _ in range(4000):
            src = alpha if rng.random() < 0.8 else rare
            recs.append(bytes(rng.choice(src) for _ in range(rng.choice([0, 1, 2, 3, 8, 30]))))
        want = expect(memo, recs)
        need = len(want[0])
        assert 0 < sum(want[2]) < len(recs), pat
        data, off = pack(recs)
        offsets = off_dev(off)
        for base in (0, 5):
            cap = max(len(data), need) + 64
            t = torch.full((base + cap + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
            t[base:base + len(data)] = to_dev(data)
            v = t[base:base + len(data)]
            out, oo, valid = p.match_strings(v, offsets, out=t[base:base + cap])
            assert out.data_ptr() == v.data_ptr()
            assert out.cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1] and valid.cpu().numpy().tolist() == want[2], (pat, base)
            assert bool((t[base + max(need, len(data)):] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())
            # too small a capacity, in place (a cap below the input's size is a cap like any other): nothing of the caller's data is written
            grew += need > len(data)
            for small in sorted({need - 1, min(need - 1, len(data))}):
                t.fill_(SENTINEL)
                t[base:base + len(data)] = to_dev(data)
                rc, m, k, _, _ = raw(p, v, len(data), offsets, len(recs), v.data_ptr(), small)
                assert (rc, m, k) == (api.E_CAPACITY, need, sum(want[2])), (pat, rc, m, k)
                assert v.cpu().numpy().tobytes() == data, pat
                assert bool((t[base + len(data):] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())
                rc, m, k, oo, _ = raw(p, v, len(data), offsets, len(recs), v.data_ptr(), cap)
                assert (rc, m) == (0, need) and t[base:base + need].cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1], pat
    assert grew == 2                                               # (one of the programs outgrows its input, at both offsets)


def test_refusals_touch_nothing():
    import torch
    data = b"12" * 300 + b"ab"
    off = [0, 100, 100, 600, 602]
    values, offsets = to_dev(data), off_dev(off)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev())

    def untouched(rc_want, p, vals=values, offs=offsets, nrec=4, n=len(data), **kw):
        rc, m, k, oo, words = raw(p, vals, n, offs, nrec, out.data_ptr(), out.numel(), **kw)
        assert rc == rc_want and m == 0 and k == 0, (rc, m, k, api.lib().trre_last_error())
        assert bool((out == SENTINEL).all())
        return oo, words

    def all_untouched(rc_want, p, **kw):
        oo, words = untouched(rc_want, p, **kw)
        assert bool((oo == -7).all()) and bool((words == 0x5A5A5A5A5A5A5A5A).all())

    all_untouched(api.E_ARG, trre_amd.Program("[0-9]+:N", "nft"))                                # a scan-mode program
    all_untouched(api.E_UNSUPPORTED, trre_amd.Program("x:\n", "nft", "match"))                 # prints a newline of its own
    p = trre_amd.Program("[0-9]+:N", "nft", "match")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    all_untouched(api.E_UNSUPPORTED, p)
    p.set_kernel(trre_amd.KERNEL_AUTO)
    for bad in ([1, 100, 100, 600, 602], [0, 100, 90, 600, 602], [0, 100, 100, 600, 601], [0, 100, 100, 603, 602]):
        all_untouched(api.E_ARG, p, offs=off_dev(bad))                                           # bad offsets: nothing written
    all_untouched(api.E_ARG, p, valid_shift=4)                                                   # an unaligned d_valid
    untouched(api.E_ARG, p, valid=out[8:].view(torch.int64))                                     # d_valid inside d_out
    # a string with an inner '\n': at the start, in the middle, as the last byte of the buffer (d_out_off and d_valid are unspecified)
    for at in (0, 300, len(data) - 1):
        holed = bytearray(data)
        holed[at] = 10
        untouched(api.E_ARG, p, vals=to_dev(bytes(holed)))
        assert "newline" in api.lib().trre_last_error().decode()
    # ... and the same strings without it go through
    rc, m, k, oo, words = raw(p, values, len(data), offsets, 4, out.data_ptr(), out.numel())
    assert (rc, m, k) == (0, 2, 2) and oo.cpu().tolist() == [0, 1, 1, 2, 2] and out[:2].cpu().numpy().tobytes() == b"NN"


def test_long_lines():
    """a 200 KiB string of z under 'abc:x' between two accepted short strings: its verdict is the symbol the long-line walker left at
    its first byte; one accepted string of 60 000 a under '(a:x)*' (below the reference's 65 536-item stack: the oracle survives it)"""
    p, memo = trre_amd.Program("abc:x", "nft", "match"), Memo("abc:x")
    want = check(p, memo, [b"abc", b"z" * (200 << 10), b"abc", b"abz", b""], "abc:x")
    assert want[2] == [True, False, True, False, False] and want[0] == b"xx"
    p, memo = trre_amd.Program("(a:x)*", "nft", "match"), Memo("(a:x)*")
    want = check(p, memo, [b"a", b"a" * 60000, b"ab", b"a" * 60000 + b"b", b""], "(a:x)*")
    assert want[2] == [True, True, False, False, True] and len(want[0]) == 60001


def test_32_mib_of_lines():
    """32 MiB of printable lines, about a third of them accepted, against the oracle (16 threads, a line at a time)"""
    import corpora
    import torch
    pat = "[a:A-m:M].*"
    x = corpora.printable_lines(32 << 20, corpora.SEED0 + 11, dev())
    data = x.cpu().numpy().tobytes()
    lines = data.split(b"\n")[:-1]
    step = (len(lines) + THREADS - 1) // THREADS

    def part(k):
        o = Oracle(pat, "nft")
        return [o.match(l + b"\n") for l in lines[k * step:(k + 1) * step]]
    with ThreadPoolExecutor(THREADS) as pool:
        per = [m for chunk in pool.map(part, range(THREADS)) for m in chunk]
    ok = np.array([m != b"" for m in per], bool)
    assert 0.25 < ok.mean() < 0.5, ok.mean()
    nl = x == 10
    ends = torch.nonzero(nl).flatten()
    offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev()), ends + 1 - torch.arange(1, ends.numel() + 1, device=dev())])
    out, oo, valid = trre_amd.Program(pat, "nft", "match").match_strings(x[~nl], offs)
    assert np.array_equal(valid.cpu().numpy(), ok)
    assert out.cpu().numpy().tobytes() == b"".join(m[:-1] for m in per)
    assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], np.cumsum([max(len(m) - 1, 0) for m in per])]))


def test_match_list():
    p = trre_amd.Program("[0-9]+:N|(cat:dog)*", "nft", "match")
    recs = [b"2024", b"", b"cat", b"catcat", b"dog", b"12a", b"0", b"cat\0dog", b"x", b"catca", b"007", b"catcatcat"]
    memo = Memo("[0-9]+:N|(cat:dog)*")
    want = [memo(r)[:-1] if memo(r) else None for r in recs]
    assert None in want and b"" in want and b"N" in want and b"dogdog" in want, want
    assert p.match_list(recs) == want
    assert p.match_list([]) == []
    out, oo, bitmap = p.match_strings(to_dev(b"".join(recs)), off_dev(pack(recs)[1]), packed=True)
    assert bitmap.cpu().numpy().tobytes() == bitmap_of([w is not None for w in want])
