"""Match spans (include/trre_mi355x.h: trre_span_device_strings; TRRE_MODE_SPANS) without a GPU.

The spans table (guided_build.cpp: span_cell) goes through the general guided family's bodies on the host; its framed text —
a position byte per staged byte, A in front of every match, B behind it — is decoded by the arithmetic the kernels do
(position = q - A before - B before - newlines before) and compared with the yardstick of tests/span_lib.py: the oracle under
the wrapped acceptor, for programs with output under their hand-written input projection.  Also: the framed-length identity,
a program that prints its own newline, the builder's and the call's refusals that need no device, the vectors the reference
does not survive."""
import ctypes
import random

import find_lib
import shim_lib
import span_lib
import trre_amd
from find_lib import Finder
from oracle_lib import Oracle, OracleError
from span_lib import LAYOUTS, PAIRS, Spanner, Weak
from trre_amd import api

A, B = 1, 2
IN, OFF, START, END, LOFF = 0x10000000, 0x30000000, 0x40000000, 0x48000000, 0x50000000
FAMILIES = (shim_lib.GUIDED_GEN, shim_lib.GUIDED_GEN8, shim_lib.GUIDED_GEN_EXACT)      # 16-byte entries, 8-byte entries, exact sub-ranges
GEOS = (1, 3)


class Tables:
    """what shim_lib.shim_scan_guided asks a program for"""

    def __init__(self, blobs):
        self.blobs = blobs

    def export_guided_tables(self):
        return self.blobs


def span_rc(p, d_in=IN, d_off=OFF, d_start=START, d_end=END, d_loff=LOFF, cap=50):
    """fake device pointers: callers pass an overlap or a program the call refuses — every one is refused after the pattern
    checks and before anything touches a device"""
    k = ctypes.c_size_t(777)
    rc = api.lib().trre_span_device_strings(p._h, d_in, 1000, d_off, 10, d_start, d_end, cap, d_loff, ctypes.byref(k), None)
    assert k.value == 0
    return rc


def decode(framed, staged):
    """per line the spans relative to it, by the kernels' arithmetic; checks the framed-length identity on the way"""
    a = b = l = 0
    starts, ends, per, plain = [], [], [], bytearray()
    line_start = 0                                      # staged position of the current line's first byte
    for q, c in enumerate(framed):
        pos = q - a - b                                 # the staged position (the kernels subtract l as well: positions in d_in)
        if c == A:
            starts.append(pos - line_start)
            a += 1
        elif c == B:
            ends.append(pos - line_start)
            b += 1
        else:
            plain.append(c)
            if c == 10:
                assert len(starts) == len(ends)
                per.append(list(zip(starts, ends)))
                starts, ends = [], []
                l += 1
                line_start = pos + 1
    assert a == b and not starts
    # markers out: the staged text's length, its newlines in place, '.' everywhere else
    assert len(framed) == len(staged) + 2 * a
    assert bytes(plain) == bytes(10 if c == 10 else ord(".") for c in staged)
    return per


def run_table(p, lines, rng, label):
    """the spans of `lines` from the table, the same on every family and geometry"""
    staged = b"".join(l + b"\n" for l in lines)
    blobs = p.export_span_tables()
    assert blobs[0] and blobs[1], label
    got = None
    for fam in FAMILIES:
        for geo in GEOS:
            try:
                framed, st = shim_lib.shim_scan_guided(Tables(blobs), fam, staged, geo, in_mis=rng.randrange(16), out_mis=rng.randrange(16))
            except RuntimeError as e:
                assert "rc -5" in str(e) and fam == shim_lib.GUIDED_GEN_EXACT, (label, fam, e)     # (tables without that form)
                continue
            assert not st & (shim_lib.ST_MISMATCH | shim_lib.ST_DIVERGE), (label, fam, geo, st)
            per = decode(framed, staged)
            assert len(per) == len(lines), (label, fam, geo)
            assert got is None or per == got, (label, fam, geo)
            got = per
    return got


def soup(rng, alphabet, n, longest=30):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, longest))) for _ in range(n)]


def test_specification_by_hand():
    for pat, s, want in (("x*", b"bb", [(0, 0), (1, 1), (2, 2)]), ("x*", b"", [(0, 0)]), ("x*", b"xxbx", [(0, 2), (2, 2), (3, 4), (4, 4)]),
                         ("(cat|dog)", b"a cat\0dog", [(2, 5)]), ("[a-z]+", b"ab 1 c", [(0, 2), (5, 6)]), ("[a-z]+", b"\0abc", []),
                         ("[0-9]+", b"abc", [])):
        assert Spanner(pat)(s) == want, (pat, s)
        p = trre_amd.Program(pat, "nft", "spans")
        assert run_table(p, [s], random.Random(1), (pat, s)) == [want], (pat, s)


def test_pairs_project_their_programs():
    """a paired program and its projection have the same matches by the oracle: the same number per line, the same raw bytes
    between them (300 random lines each)"""
    rng = random.Random(61)
    for prog, acc in PAIRS:
        lines = soup(rng, b"abcdoginxt 0189", 300)
        spans = Spanner(acc).lines(lines)
        weak = Weak(prog).lines(lines)
        for l, sp, (n, raw) in zip(lines, spans, weak):
            assert len(sp) == n and span_lib.gaps(l, sp) == raw, (prog, acc, l)


def test_tables_against_the_oracle():
    """golden acceptors, the pairs and the three symbol layouts: the table's spans are the yardstick's.  No case is skipped."""
    rng = random.Random(62)
    golden = span_lib.golden_acceptors()
    assert len(golden) >= 18, len(golden)
    cases = [(pat, pat, name, lines) for pat, vs in golden.items() for name, lines in vs]
    extra = [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd", b"sing a thing", b"a  b   ", b"12 ab 345", b"", b"a\0cat", b"\0", b"cat\0"]
    for prog, acc in PAIRS + LAYOUTS:
        cases.append((prog, acc, "pair", soup(rng, b"abcdefgh ingxt059", 200) + extra))
    layouts, n_matches, n_empty, n_nul = set(), 0, 0, 0
    progs = {}
    for prog, acc, name, lines in cases:
        if prog not in progs:
            progs[prog] = (trre_amd.Program(prog, "nft", "spans"), Spanner(acc))
        p, spanner = progs[prog]
        assert p.info.kernel == trre_amd.KERNEL_GUIDED_GEN, prog
        want = spanner.lines(lines)
        got = run_table(p, lines, rng, (prog, name))
        assert got == want, (prog, name)
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
        n_matches += sum(len(w) for w in want)
        n_empty += sum(s == e for w in want for s, e in w)
        n_nul += sum(b"\0" in l for l in lines)
    assert layouts == {4, 8, 16} and n_matches > 10000 and n_empty > 100 and n_nul > 20, (layouts, n_matches, n_empty, n_nul)


def test_counts_and_gaps_on_every_usable_golden_vector():
    """the wide check, transducers included: per line the number of spans is the length of Finder(P)'s list and the bytes outside
    the spans are the bytes outside A..B of the oracle's output for the wrapped program.  Nothing is skipped but the vectors
    the reference does not survive; a pattern beyond the guided tables is refused by the builder, as the call documents, exactly
    when scan mode has no guided tables either — asserted, and its vectors counted."""
    rng = random.Random(63)
    usable, dead, left_out, n = find_lib.vectors()
    assert len(usable) + len(dead) + len(left_out) == n and len(dead) == 13
    progs, compared, refused = {}, 0, 0
    for pat, name, data in usable:
        lines = find_lib.lines_of(data)
        if pat not in progs:
            try:
                progs[pat] = (trre_amd.Program(pat, "nft", "spans"), Finder(pat), Weak(pat))
            except trre_amd.TrreError as e:
                assert e.code == api.E_UNSUPPORTED and "guided tables" in e.message, (pat, e)
                assert trre_amd.Program(pat, "nft").info.guided_rev_states == 0, pat
                progs[pat] = None
        if progs[pat] is None:
            refused += 1
            continue
        p, finder, weak = progs[pat]
        staged = b"".join(l + b"\n" for l in lines)
        framed, st = shim_lib.shim_scan_guided(Tables(p.export_span_tables()), shim_lib.GUIDED_GEN, staged, rng.choice(GEOS))
        assert not st & (shim_lib.ST_MISMATCH | shim_lib.ST_DIVERGE), (pat, name, st)
        got = decode(framed, staged)
        assert [len(w) for w in got] == [len(w) for w in finder.lines(lines)], (pat, name)
        for l, sp, (k, raw) in zip(lines, got, weak.lines(lines)):
            assert len(sp) == k and span_lib.gaps(l, sp) == raw, (pat, name, l)
            assert all(0 <= s <= e <= len(span_lib.cut(l)) for s, e in sp) and all(sp[j][1] <= sp[j + 1][0] for j in range(len(sp) - 1)), (pat, l, sp)
        compared += 1
    assert compared + refused == len(usable) and compared > 400 and refused < 10, (compared, refused)


def test_framed_length_identity_on_nuls_and_empty_lines():
    """decode() asserts it on every call; here on lines made of NULs, empty lines and NULs at either end"""
    rng = random.Random(64)
    lines = [b"", b"\0", b"\0\0\0", b"cat\0", b"\0cat", b"a cat\0dog\0cat", b""] * 3 + soup(rng, b"cat\0dog ", 300, 12) + [b""] * 70
    for pat in ("(cat|dog)", "x*", "[a-z]+", "(cat:dog|dog:cat)"):
        p = trre_amd.Program(pat, "nft", "spans")
        got = run_table(p, lines, rng, pat)
        want = Spanner(dict(PAIRS).get(pat, pat)).lines(lines)
        assert got == want, pat
    assert any(b"\0" in l[:-1] for l in lines)


def test_a_program_that_prints_its_own_newline():
    """nothing the program prints reaches the framed text: 'a:\\n' has the spans of 'a'"""
    rng = random.Random(65)
    lines = soup(rng, b"ab \0", 200, 20) + [b"banana", b"", b"aaa"]
    for prog, acc in (("a:\n", "a"), ("(a:\n\n|b:\nx)", "(a|b)"), ("a+:\n", "a+")):
        p = trre_amd.Program(prog, "nft", "spans")
        assert run_table(p, lines, rng, prog) == Spanner(acc).lines(lines), prog
        assert span_rc(p, d_loff=OFF + 8) == api.E_ARG                                   # (refused for the overlap, not for the newline)


def test_extra_patterns_cover_the_symbol_layouts():
    n = [trre_amd.Program(prog, "nft", "spans").info.guided_rev_states for prog, _ in LAYOUTS]
    assert 16 < n[0] <= 256 and n[1] == 16 and n[2] > 256, n


def test_builder_and_call_refusals():
    last = lambda: api.lib().trre_last_error().decode()
    h = ctypes.c_void_p()
    assert api.MODE_SPANS == 8
    for mode in (5, 6, 7, 9, 12):                       # what was no mode before is none now
        assert api.lib().trre_compile_mode(b"a:b", 3, api.ENGINE_NFT, mode, ctypes.byref(h)) == api.E_ARG and not h.value
    for pat in (b"a:b", b"[a:A-z:Z]", b"[0-9]+"):
        assert api.lib().trre_compile_mode(pat, len(pat), api.ENGINE_DFT, api.MODE_SPANS, ctypes.byref(h)) == api.E_UNSUPPORTED and not h.value
        assert "non-deterministic engine" in last()
    # a program of any other mode is no spans program
    for mode in ("scan_all", "match_all", "scan", "match", "find"):
        assert span_rc(trre_amd.Program("a:b", "nft", mode)) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert span_rc(p) == api.E_UNSUPPORTED and "backtracking" in last()
    p.set_kernel(trre_amd.KERNEL_AUTO)
    assert span_rc(p, d_loff=OFF + 8) == api.E_ARG and "offsets array overlaps" in last()
    for fam in (trre_amd.KERNEL_TILE_GEN, trre_amd.KERNEL_STREAM_GEN, trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_BYTEMAP):
        assert api.lib().trre_set_kernel(p._h, fam) == api.E_UNSUPPORTED
    # a spans program given to the other scan calls
    m = ctypes.c_size_t(5)
    L = api.lib()
    OUT, MOFF = 0x20000000, 0x60000000
    assert L.trre_scan_device(p._h, IN, 100, OUT, 200, ctypes.byref(m), None) == api.E_ARG and m.value == 0 and "TRRE_MODE_SPANS" in last()
    assert L.trre_scan_device_records(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, ctypes.byref(m), None) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    assert L.trre_scan_device_strings(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, ctypes.byref(m), None) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    assert L.trre_match_device_strings(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, MOFF, ctypes.byref(m), ctypes.byref(m), None) == api.E_ARG
    assert L.trre_find_device_strings(p._h, IN, 100, OFF, 2, OUT, 200, MOFF, 5, LOFF, ctypes.byref(m), ctypes.byref(m), None) == api.E_ARG
    assert L.trre_scan_enqueue(p._h, IN, 100, OUT, 200, None) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    buf = ctypes.create_string_buffer(64)
    assert L.trre_scan_host(p._h, b"12\n", 3, buf, 64, ctypes.byref(m), 0) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    assert L.trre_scan_host_multi(p._h, b"12\n", 3, buf, 64, ctypes.byref(m), 1) == api.E_ARG and "TRRE_MODE_SPANS" in last()


def test_overlaps_and_nulls_are_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    E = api.E_ARG
    assert span_rc(p, d_start=IN + 992) == E and span_rc(p, d_start=OFF + 80) == E and span_rc(p, d_start=LOFF + 80) == E      # starts in in / off / list offsets
    assert span_rc(p, d_end=IN + 992) == E and span_rc(p, d_end=OFF + 80) == E and span_rc(p, d_end=LOFF - 392) == E
    assert span_rc(p, d_end=START + 392) == E and span_rc(p, d_end=START) == E                                                # the two span arrays
    assert span_rc(p, d_loff=IN + 992) == E and span_rc(p, d_loff=OFF + 80) == E and span_rc(p, d_off=IN + 500) == E
    assert span_rc(p, d_in=None) == E and span_rc(p, d_off=None) == E and span_rc(p, d_loff=None) == E
    assert span_rc(p, d_start=None) == E and span_rc(p, d_end=None) == E                                                      # null with span_cap != 0
    assert api.lib().trre_span_device_strings(None, IN, 10, OFF, 1, START, END, 5, LOFF, None, None) == E


def test_library_exports_span_symbol():
    assert hasattr(api.lib(), "trre_span_device_strings")
    for name in ("span_strings", "span_list", "count_strings"):
        assert hasattr(trre_amd.Program, name)
    assert trre_amd.Program("a:b", "nft").export_span_tables() == (b"", b"")
    assert trre_amd.Program("a:b", "nft", "find").export_span_tables() == (b"", b"")


def test_vectors_the_reference_does_not_survive():
    """such a vector shows: a diverge mark in the status of the table's scan, or the stack guard's hit"""
    _, dead, _, _ = find_lib.vectors()
    by_status = by_guard = 0
    for pat, name, data in dead:
        try:
            Oracle(pat, "nft").scan(data)
            assert False, (pat, name, "the reference survives")
        except OracleError:
            pass
        p = trre_amd.Program(pat, "nft", "spans")
        st = shim_lib.shim_scan_guided(Tables(p.export_span_tables()), shim_lib.GUIDED_GEN, data, 1)[1]
        if st & shim_lib.ST_DIVERGE:
            by_status += 1
            continue
        r = shim_lib.stack_guard(p, data)
        assert r is not None and r[0] == 1, (pat, name, r)
        by_guard += 1
    assert by_status + by_guard == len(dead) == 13 and by_status > 0, (by_status, by_guard)
