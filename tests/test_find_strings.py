"""Found strings (include/trre_mi355x.h: trre_find_device_strings; TRRE_MODE_FIND) without a GPU.

find(s) is the list of the outputs of the scan loop's successful attempts on the line s.  The yardstick is the oracle under the
wrapped pattern (tests/find_lib.py): (a) pins the yardstick itself on the NFT golden scan vectors; (b) runs the two forward
tables of a find program — texts: every match's output and a '\\n'; marks: a byte per match and the line's '\\n' — through the
general guided family's bodies on the host and compares them with the framed expectations built from the oracle's pieces;
(c) the builder's and the call's refusals that need no device; (d) a vector the reference does not survive shows in the tables'
status or in the stack guard, as in scan mode."""
import ctypes
import random

import find_lib
import shim_lib
import trre_amd
from find_lib import EXTRA, Finder, lines_of
from oracle_lib import Oracle, OracleError
from trre_amd import api

IN, OUT, OFF, MOFF, LOFF = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
FAMILIES = (shim_lib.GUIDED_GEN, shim_lib.GUIDED_GEN8, shim_lib.GUIDED_GEN_EXACT)      # 16-byte entries, 8-byte entries, exact sub-ranges
GEOS = (1, 3)


def find_rc(p, d_loff=LOFF, d_moff=MOFF, d_in=IN, d_out=OUT, d_off=OFF):
    """fake device pointers: with the default arguments a find program gets as far as the device (not wanted here), so callers pass
    an overlap — every program is refused after the pattern checks and before anything touches a device"""
    m, k = ctypes.c_size_t(12345), ctypes.c_size_t(777)
    rc = api.lib().trre_find_device_strings(p._h, d_in, 1000, d_off, 10, d_out, 2000, d_moff, 50, d_loff, ctypes.byref(k), ctypes.byref(m), None)
    assert m.value == 0 and k.value == 0
    return rc


def prints_newline(p):
    rc = find_rc(p, d_loff=OFF + 8)
    assert rc in (api.E_UNSUPPORTED, api.E_ARG), rc
    return rc == api.E_UNSUPPORTED


class Tables:
    """what shim_lib.shim_scan_guided asks a program for"""

    def __init__(self, rblob, fwd):
        self.blobs = (rblob, fwd)

    def export_guided_tables(self):
        return self.blobs


def framed(want):
    """the two scans of the staged text, as the tables are to print them"""
    return b"".join(o + b"\n" for w in want for o in w), b"".join(b"m" * len(w) + b"\n" for w in want)


def test_yardstick_on_golden_vectors():
    """(a) the wrapped pattern scans like the plain one and its markers nest on all but a few of the NFT golden scan vectors"""
    usable, dead, left_out, n = find_lib.vectors()
    assert len(usable) + len(dead) + len(left_out) == n == 465, (len(usable), len(dead), len(left_out), n)
    assert len(left_out) <= 0.05 * n, left_out
    assert len(dead) == 13 and len(usable) > 400, (len(dead), len(usable))
    assert {why for _, _, why in left_out} <= {"marker", "identity"}, left_out


def test_specification_by_hand():
    for pat, s, want in (("x*", b"bb", [b"", b"", b""]), ("x*", b"", [b""]), ("x*", b"xxbx", [b"xx", b"", b"x", b""]), ("[a-z]+", b"ab 1 c", [b"ab", b"c"]),
                         ("[0-9]+:N", b"abc", []), ("(cat:dog|dog:cat)", b"a cat, a dog", [b"dog", b"cat"]), ("(a:xyz)", b"a\0a", [b"xyz"]),
                         ("[a-z]+", b"\0abc", [])):
        assert Finder(pat)(s) == want, (pat, s)


def test_tables_against_the_oracle():
    """(b) both forward tables over the lines of every usable golden vector and of three more patterns (more than 16 backward
    states, exactly 16, 16-bit symbols), on every general guided shim id and two geometries"""
    rng = random.Random(404)
    usable, _, _, _ = find_lib.vectors()
    soup = [bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randrange(0, 30))) for _ in range(200)]
    cases = [(pat, name, lines_of(data)) for pat, name, data in usable]
    cases += [(pat, "extra", lines_of(usable[0][2])[:50] + soup + [b"xcat aabb", b"the cat sat abab", b"aabbaa", b"abcdefghab cd"]) for pat in EXTRA]
    progs, compared, newline_printing, no_tables, layouts, n_matches, n_empty = {}, 0, 0, 0, set(), 0, 0
    for pat, name, lines in cases:
        if pat not in progs:
            try:
                p = trre_amd.Program(pat, "nft", "find")
                progs[pat] = (p, prints_newline(p), p.export_find_tables(), Finder(pat))
            except trre_amd.TrreError as e:
                # a pattern beyond the guided tables' limits is refused by the builder — exactly when scan mode has none either
                assert e.code == api.E_UNSUPPORTED and "guided tables" in e.message, (pat, e)
                assert trre_amd.Program(pat, "nft").info.guided_rev_states == 0, pat
                progs[pat] = None
        if progs[pat] is None:
            no_tables += 1
            continue
        p, no, (rblob, texts, marks), finder = progs[pat]
        assert p.info.kernel == trre_amd.KERNEL_GUIDED_GEN and rblob and texts and marks, pat
        if no:
            newline_printing += 1
            continue
        want = finder.lines(lines)
        staged = b"".join(l + b"\n" for l in lines)
        exp_texts, exp_marks = framed(want)
        n_rev = p.info.guided_rev_states
        layouts.add(4 if n_rev <= 16 else 8 if n_rev <= 256 else 16)
        for fam in FAMILIES:
            for geo in GEOS:
                mis = rng.randrange(16)
                for blob, exp, what in ((texts, exp_texts, "texts"), (marks, exp_marks, "marks")):
                    try:
                        got, st = shim_lib.shim_scan_guided(Tables(rblob, blob), fam, staged, geo, in_mis=mis, out_mis=rng.randrange(16))
                    except RuntimeError as e:
                        assert "rc -5" in str(e) and fam == shim_lib.GUIDED_GEN_EXACT, (pat, name, fam, e)     # (tables without that form)
                        continue
                    assert not st & (shim_lib.ST_MISMATCH | shim_lib.ST_DIVERGE), (pat, name, fam, geo, what, st)
                    assert got == exp, (pat, name, fam, geo, what)
        compared += 1
        n_matches += sum(len(w) for w in want)
        n_empty += sum(o == b"" for w in want for o in w)
    assert compared + newline_printing + no_tables == len(cases) and compared > 400 and no_tables < 10, (compared, newline_printing, no_tables)
    assert layouts == {4, 8, 16} and n_matches > 10000 and n_empty > 100, (layouts, n_matches, n_empty)


def test_extra_patterns_cover_the_symbol_layouts():
    n = [trre_amd.Program(pat, "nft", "find").info.guided_rev_states for pat in EXTRA]
    assert 16 < n[0] <= 256 and n[1] == 16 and n[2] > 256, n


def test_builder_and_call_refusals():
    """(c)"""
    last = lambda: api.lib().trre_last_error().decode()
    h = ctypes.c_void_p()
    for pat in (b"a:b", b"[a:A-z:Z]", b"[0-9]+:N"):
        assert api.lib().trre_compile_mode(pat, len(pat), api.ENGINE_DFT, api.MODE_FIND, ctypes.byref(h)) == api.E_UNSUPPORTED and not h.value
        assert "non-deterministic engine" in last()
    # the generator modes and find mode are modes of their own: a generator program is no find program, an unknown mode is none at all
    for mode in ("scan_all", "match_all", "scan", "match"):
        assert find_rc(trre_amd.Program("a:b", "nft", mode)) == api.E_ARG and "TRRE_MODE_FIND" in last()
    assert api.lib().trre_compile_mode(b"a:b", 3, api.ENGINE_NFT, api.MODE_FIND | 2, ctypes.byref(h)) == api.E_ARG and not h.value
    assert api.lib().trre_compile_mode(b"a:b", 3, api.ENGINE_NFT, 5, ctypes.byref(h)) == api.E_ARG and not h.value
    # a pattern that prints a '\n' of its own
    assert find_rc(trre_amd.Program("x:\n", "nft", "find")) == api.E_UNSUPPORTED and "newline" in last()
    p = trre_amd.Program("[0-9]+:N", "nft", "find")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert find_rc(p) == api.E_UNSUPPORTED and "backtracking" in last()
    p.set_kernel(trre_amd.KERNEL_AUTO)
    assert find_rc(p, d_loff=OFF + 8) == api.E_ARG and "offsets array overlaps" in last()
    for fam in (trre_amd.KERNEL_TILE_GEN, trre_amd.KERNEL_STREAM_GEN, trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_BYTEMAP):
        assert api.lib().trre_set_kernel(p._h, fam) == api.E_UNSUPPORTED
    # a find program given to the other scan calls
    m = ctypes.c_size_t(5)
    L = api.lib()
    assert L.trre_scan_device(p._h, IN, 100, OUT, 200, ctypes.byref(m), None) == api.E_ARG and m.value == 0 and "TRRE_MODE_FIND" in last()
    assert L.trre_scan_device_records(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, ctypes.byref(m), None) == api.E_ARG and "TRRE_MODE_FIND" in last()
    assert L.trre_scan_device_strings(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, ctypes.byref(m), None) == api.E_ARG and "TRRE_MODE_FIND" in last()
    assert L.trre_match_device_strings(p._h, IN, 100, OFF, 2, OUT, 200, LOFF, MOFF, ctypes.byref(m), ctypes.byref(m), None) == api.E_ARG
    assert L.trre_scan_enqueue(p._h, IN, 100, OUT, 200, None) == api.E_ARG and "TRRE_MODE_FIND" in last()
    buf = ctypes.create_string_buffer(64)
    assert L.trre_scan_host(p._h, b"12\n", 3, buf, 64, ctypes.byref(m), 0) == api.E_ARG and "TRRE_MODE_FIND" in last()
    assert L.trre_scan_host_multi(p._h, b"12\n", 3, buf, 64, ctypes.byref(m), 1) == api.E_ARG and "TRRE_MODE_FIND" in last()


def test_overlaps_and_nulls_are_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "find")
    E = api.E_ARG
    assert find_rc(p, d_moff=OUT + 8) == E and find_rc(p, d_moff=IN + 992) == E and find_rc(p, d_moff=OFF + 80) == E     # match_off in out / in / off
    assert find_rc(p, d_moff=LOFF + 80) == E and find_rc(p, d_moff=LOFF - 400) == E                                       # ... and the list offsets
    assert find_rc(p, d_loff=OUT + 8) == E and find_rc(p, d_loff=IN + 992) == E and find_rc(p, d_loff=OFF + 80) == E
    assert find_rc(p, d_off=IN + 500) == E and find_rc(p, d_out=IN + 10) == E
    assert find_rc(p, d_in=None) == E and find_rc(p, d_off=None) == E and find_rc(p, d_out=None) == E
    assert find_rc(p, d_moff=None) == E and find_rc(p, d_loff=None) == E
    assert api.lib().trre_find_device_strings(None, IN, 10, OFF, 1, OUT, 10, MOFF, 5, LOFF, None, None, None) == E


def test_library_exports_find_symbol():
    assert hasattr(api.lib(), "trre_find_device_strings")
    assert hasattr(trre_amd.Program, "find_strings") and hasattr(trre_amd.Program, "find_list")
    assert trre_amd.Program("a:b", "nft").export_find_tables() == (b"", b"", b"")           # (scan mode has one forward table)


def test_vectors_the_reference_does_not_survive():
    """(d) such a vector shows: a diverge mark in the status of both tables' scans, or the stack guard's hit"""
    _, dead, _, _ = find_lib.vectors()
    by_status = by_guard = 0
    for pat, name, data in dead:
        try:
            Oracle(pat, "nft").scan(data)
            assert False, (pat, name, "the reference survives")
        except OracleError:
            pass
        p = trre_amd.Program(pat, "nft", "find")
        rblob, texts, marks = p.export_find_tables()
        sts = [shim_lib.shim_scan_guided(Tables(rblob, blob), shim_lib.GUIDED_GEN, data, 1)[1] for blob in (texts, marks)]
        if all(st & shim_lib.ST_DIVERGE for st in sts):
            by_status += 1
            continue
        assert not any(st & shim_lib.ST_DIVERGE for st in sts), (pat, name, sts)
        r = shim_lib.stack_guard(p, data)
        assert r is not None and r[0] == 1, (pat, name, r)
        by_guard += 1
    assert by_status + by_guard == len(dead) == 13 and by_status > 0, (by_status, by_guard)
