"""Matched strings (include/trre_mi355x.h: trre_match_device_strings) without a GPU.

The device path rests on one identity.  The STAGED text b"".join(r + b"\\n") of strings that hold no '\\n' is exactly the
strings' lines, its match scan M is the concatenation of m_i = M(r_i + b"\\n"), and a program that prints no '\\n' of its own
prints one per ACCEPTED line and nothing for a rejected one: with M_i the number of accepted strings among 0 .. i, string i's
framed output ends just past framed newline number M_i, d_out_off[i + 1] is that position minus M_i (0 when M_i is 0), and the
output bytes are the framed output without its newlines.  It is pinned here on the oracle over every golden match vector and
random strings over each pattern's bytes.  Then the verdict table: accept[symbol at a string's first staged byte] is the oracle's
verdict, for every one of those patterns and two more at the nibble-packed and byte-symbol sizes.  Then what needs no device:
the symbol, the refusals."""
import ctypes
import random

import numpy as np

import golden_lib
import shim_lib
import trre_amd
from oracle_lib import Oracle, OracleError
from trre_amd import api

IN, OUT, OFF, VAL = 0x10000000, 0x20000000, 0x30000000, 0x40000000
EXTRA = [".*(cat:dog).*(a|b){4}", "(a|b)*a(a|b){5}"]      # this build: 19 backward states (a byte per symbol), 16 (the last nibble-packed size)


def match_rc(p, d_ooff=OFF + 8, d_valid=VAL):
    """fake device pointers and overlapping offset arrays: every program taken is refused (TRRE_E_ARG) after the pattern checks
    and before anything touches a device"""
    m, k = ctypes.c_size_t(12345), ctypes.c_size_t(777)
    rc = api.lib().trre_match_device_strings(p._h, IN, 1000, OFF, 10, OUT, 2000, d_ooff, d_valid, ctypes.byref(k), ctypes.byref(m), None)
    assert m.value == 0 and k.value == 0
    return rc


def prints_newline(p):
    rc = match_rc(p)
    assert rc in (api.E_UNSUPPORTED, api.E_ARG), rc
    return rc == api.E_UNSUPPORTED


def pattern_bytes(pat, data):
    """the bytes random strings are made of: the pattern's own literals, a few of the vector's, a NUL"""
    own = bytes(c for c in set(pat.encode("latin-1") if isinstance(pat, str) else pat) if c not in b"\n\\()[]{}|*+?:.-^,")
    return (own or b"ab") + bytes(set(data) - {10})[:6] + b"\0"


def strings_of(rng, pat, data):
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    alpha = pattern_bytes(pat, data)
    extra = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 8, 13]))) for _ in range(40)]
    recs = lines + extra
    rng.shuffle(recs)
    return recs


def derive(framed, verdicts):
    """the rule the passes implement: ranks, located positions, final offsets, the bytes"""
    nl = [i for i, c in enumerate(framed) if c == 10]
    offs, rank = [0], 0
    for ok in verdicts:
        rank += ok
        offs.append(nl[rank - 1] + 1 - rank if rank else 0)
    return framed.replace(b"\n", b""), offs, rank == len(nl)


def programs():
    """(pattern, vectors) of the golden match set, the two extra patterns on the first vector's input"""
    by_pat = {}
    for pat, name, data, exp in golden_lib.match_cases():
        by_pat.setdefault(pat, []).append((name, data))
    some = next(iter(by_pat.values()))[0]
    for pat in EXTRA:
        by_pat.setdefault(pat, []).append(some)
    return by_pat


def test_identity_on_golden_match_vectors():
    rng = random.Random(1212)
    n_cases = compared = diverged = refused = n_rejected = n_accepted = n_empty = n_nul = 0
    progs = {}
    for pat, name, data, exp in golden_lib.match_cases():
        n_cases += 1
        if pat not in progs:
            progs[pat] = (prints_newline(trre_amd.Program(pat, "nft", "match")), Oracle(pat, "nft"))
        no, o = progs[pat]
        if no:
            refused += 1
            continue
        recs = strings_of(rng, pat, data)
        assert not any(b"\n" in r for r in recs)
        try:
            per = [o.match(r + b"\n") for r in recs]
            framed = o.match(b"".join(r + b"\n" for r in recs))
        except OracleError:
            diverged += 1
            continue
        assert framed == b"".join(per), (pat, name)                      # the match scan of the staged text: the m_i, concatenated
        verdicts = [m != b"" for m in per]
        assert all(m.endswith(b"\n") and m.count(b"\n") == 1 for m in per if m), (pat, name)
        got, offs, whole = derive(framed, verdicts)
        want = [m[:-1] for m in per]
        assert whole and got == b"".join(want), (pat, name)
        assert offs == [0] + np.cumsum([len(w) for w in want]).tolist(), (pat, name)
        compared += 1
        n_accepted += sum(verdicts)
        n_rejected += len(verdicts) - sum(verdicts)
        n_empty += b"" in recs
        n_nul += any(b"\0" in r for r in recs)
    assert compared + diverged + refused == n_cases == 123, (compared, diverged, refused, n_cases)
    assert compared > 90 and n_accepted > 200 and n_rejected > 1000 and n_empty > 50 and n_nul > 50, (compared, n_accepted, n_rejected, n_empty, n_nul)


def test_accept_table_is_the_oracles_verdict():
    """accept[symbol at s_i] == (the oracle prints something for string i), s_i = off[i] + i: the string's first staged byte, its
    '\\n' when it is empty"""
    rng = random.Random(77)
    sizes, checked, n_patterns = set(), 0, 0
    for pat, vectors in programs().items():
        p = trre_amd.Program(pat, "nft", "match")
        if prints_newline(p):
            continue
        accept = p.export_accept_table()
        n_rev = p.info.guided_rev_states
        if not n_rev:
            assert accept == b""
            continue
        assert len(accept) == n_rev and set(accept) <= {0, 1}, pat
        if n_rev > 256:
            continue                                             # (the host shim's sweep stores a byte per symbol)
        sizes.add("nibble" if n_rev <= 16 else "byte")
        n_patterns += 1
        rblob, _ = p.export_guided_tables()
        o = Oracle(pat, "nft")
        for name, data in vectors:
            recs = strings_of(rng, pat, data)
            staged = b"".join(r + b"\n" for r in recs)
            sym = shim_lib.rev_symbols(rblob, staged, geo=1, in_mis=rng.randrange(16))
            at = 0
            for r in recs:
                try:
                    want = o.match(r + b"\n") != b""
                except OracleError:
                    want = None                                  # (a line the reference does not survive has no verdict)
                if want is not None:
                    assert bool(accept[sym[at]]) == want, (pat, name, r, sym[at])
                    checked += 1
                at += len(r) + 1
    assert sizes == {"nibble", "byte"}, sizes
    assert n_patterns >= 30 and checked > 3000, (n_patterns, checked)


def test_extra_patterns_cover_both_symbol_layouts():
    n = [trre_amd.Program(pat, "nft", "match").info.guided_rev_states for pat in EXTRA]
    assert 16 < n[0] <= 256 and 0 < n[1] <= 16, n


def test_specification_by_hand():
    for pat, rec, want in (("(a:x)*", b"", b"\n"), ("(a:x)*", b"aa", b"xx\n"), ("(a:x)*", b"ab", b""), ("a+:x", b"", b""), ("a+:x", b"aaa", b"x\n"),
                           (":x", b"", b"x\n"), (":x", b"a", b""), ("(a:x)*", b"a\0b", b"x\n")):
        assert Oracle(pat, "nft").match(rec + b"\n") == want, (pat, rec)


def test_library_exports_match_symbol():
    assert hasattr(api.lib(), "trre_match_device_strings")
    assert hasattr(trre_amd.Program, "match_strings") and hasattr(trre_amd.Program, "match_list")
    assert trre_amd.Program("a:b", "nft").export_accept_table() == b""          # (scan mode has no verdicts)


def test_refusals_before_the_device():
    last = lambda: api.lib().trre_last_error().decode()
    assert match_rc(trre_amd.Program("a:b", "nft")) == api.E_ARG and "TRRE_MODE_MATCH" in last()
    assert match_rc(trre_amd.Program("[a:A-z:Z]", "dft")) == api.E_ARG and "TRRE_MODE_MATCH" in last()
    assert match_rc(trre_amd.Program("x:\n", "nft", "match")) == api.E_UNSUPPORTED and "newline" in last()
    p = trre_amd.Program("[0-9]+:N", "nft", "match")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert match_rc(p) == api.E_UNSUPPORTED and "guided tables" in last()
    p.set_kernel(trre_amd.KERNEL_AUTO)
    assert match_rc(p) == api.E_ARG and "offsets array overlaps" in last()


def test_overlaps_alignment_and_nulls_are_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "match")
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    f = api.lib().trre_match_device_strings
    tail = (ctypes.byref(k), ctypes.byref(m), None)
    last = lambda: api.lib().trre_last_error().decode()
    good = OFF + 4096
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, VAL + 4, *tail) == api.E_ARG and "8-byte aligned" in last()
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, VAL + 1, *tail) == api.E_ARG and "8-byte aligned" in last()
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, OUT + 8, *tail) == api.E_ARG and "bitmap overlaps" in last()      # d_valid inside d_out
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, IN + 992, *tail) == api.E_ARG and "bitmap overlaps" in last()    # ... the input
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, OFF + 80, *tail) == api.E_ARG and "bitmap overlaps" in last()    # ... the offsets
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, good + 80, *tail) == api.E_ARG and "bitmap overlaps" in last()
    assert f(p._h, IN, 1000, IN + 500, 10, OUT, 2000, good, VAL, *tail) == api.E_ARG
    assert f(p._h, IN, 1000, OFF, 10, IN + 10, 2000, good, VAL, *tail) == api.E_ARG
    assert f(p._h, None, 1000, OFF, 10, OUT, 2000, good, VAL, *tail) == api.E_ARG
    assert f(p._h, IN, 1000, None, 10, OUT, 2000, good, VAL, *tail) == api.E_ARG
    assert f(p._h, IN, 1000, OFF, 10, None, 2000, good, VAL, *tail) == api.E_ARG
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, None, VAL, *tail) == api.E_ARG
    assert f(p._h, IN, 1000, OFF, 10, OUT, 2000, good, None, *tail) == api.E_ARG
