"""Filtered strings (include/trre_mi355x.h: trre_filter_device_strings; Program.filter_strings / filter_list) without a GPU: the
refusals that are found before the device is touched — with fake device pointers, as tests/test_split_strings.py does for the
split call — and the definition of tests/filter_lib.py against re.search through the oracle's spans."""
import ctypes
import itertools
import re

import filter_lib
import trre_amd
from span_lib import Spanner
from trre_amd import api

IN, OFF, OUT, OOFF, ROWS = 0x10000000, 0x30000000, 0x20000000, 0x40000000, 0x50000000
# d_in 1000 bytes, d_off 88 bytes, d_out 2000 bytes, d_out_off 408 bytes, d_rows 400 bytes
SIZES = {"d_in": 1000, "d_off": 88, "d_out": 2000, "d_ooff": 408, "d_rows": 400}
BASES = {"d_in": IN, "d_off": OFF, "d_out": OUT, "d_ooff": OOFF, "d_rows": ROWS}


def filter_rc(p, d_in=IN, d_off=OFF, d_out=OUT, d_ooff=OOFF, d_rows=ROWS, cap=2000, rcap=50, flags=0):
    """fake device pointers: callers pass an overlap or a program the call refuses — every one is refused before anything touches
    a device; both sizes are 0 then"""
    k, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = api.lib().trre_filter_device_strings(p._h if p else None, d_in, 1000, d_off, 10, flags, d_out, cap, d_ooff, d_rows, rcap, ctypes.byref(k),
                                              ctypes.byref(m), None)
    assert k.value == 0 and m.value == 0
    return rc


def last():
    return api.lib().trre_last_error().decode()


def test_library_exports_filter_symbol():
    assert hasattr(api.lib(), "trre_filter_device_strings")
    for name in ("filter_strings", "filter_list"):
        assert hasattr(trre_amd.Program, name)
    assert api.FILTER_INVERT == 1


def test_programs_the_call_refuses():
    for mode in ("scan_all", "match_all", "scan", "match", "find"):
        assert filter_rc(trre_amd.Program("a:b", "nft", mode)) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert filter_rc(p) == api.E_UNSUPPORTED and "backtracking" in last()
    assert filter_rc(p, flags=api.FILTER_INVERT) == api.E_UNSUPPORTED
    p.set_kernel(trre_amd.KERNEL_AUTO)
    assert filter_rc(p, rcap=1 << 58) == api.E_ARG and "too many" in last()
    L = api.lib()
    assert L.trre_filter_device_strings(p._h, IN, 1 << 55, OFF, 10, 0, OUT, 2000, OOFF, ROWS, 50, None, None, None) == api.E_ARG and "too many" in last()
    assert L.trre_filter_device_strings(p._h, IN, 1000, OFF, 1 << 55, 0, OUT, 2000, OOFF, ROWS, 50, None, None, None) == api.E_ARG and "too many" in last()


def test_an_unknown_flag_bit_is_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE):
        assert filter_rc(p, flags=flags) == api.E_ARG and "flag" in last(), flags


def test_nulls_are_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    E = api.E_ARG
    assert filter_rc(None) == E
    assert filter_rc(p, d_in=None) == E and filter_rc(p, d_off=None) == E
    assert filter_rc(p, d_out=None) == E                                                # null with room promised
    assert filter_rc(p, d_ooff=None) == E and filter_rc(p, d_rows=None) == E
    assert filter_rc(p, d_ooff=None, d_rows=None) == E
    assert "null argument" in last()


def test_every_pairwise_overlap_is_refused():
    """each pair of the five arrays sharing its last / first byte either way round, and one array starting inside another"""
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    pairs = list(itertools.combinations(sorted(SIZES), 2))
    assert len(pairs) == 10
    for a, b in pairs:
        for moved, fixed in ((a, b), (b, a)):
            for at in (BASES[fixed] + SIZES[fixed] - 1, BASES[fixed] - SIZES[moved] + 1, BASES[fixed] + 8):
                assert filter_rc(p, **{moved: at}) == api.E_ARG, (moved, fixed, hex(at))
                assert "overlaps" in last(), (moved, fixed, last())
    assert filter_rc(p, d_out=IN) == api.E_ARG and "not made in place" in last()        # (d_in == d_out: no in-place form)


def test_the_expectation_is_re_search():
    """the yardstick itself: kept exactly when re.search finds something, for patterns both understand"""
    for pat, lines in ((",", [b"a,b,,c", b"", b",", b"no comma", b",,", b"x,"]),
                       ("[0-9]+", [b"12ab345", b"ab", b"7", b"a1b22c333", b"", b"x y"]),
                       ("x*", [b"bb", b"", b"xx"]),
                       ("(cat|dog)", [b"a cat", b"cow", b"", b"hotdog", b"ca t"])):
        spans = Spanner(pat).lines(lines)
        for invert in (False, True):
            out, oo, rows = filter_lib.expect(lines, spans, invert)
            want = [i for i, l in enumerate(lines) if (re.search(pat.encode(), l) is not None) != invert]
            assert rows == want, (pat, invert)
            assert filter_lib.kept_strings(out, oo) == [lines[i] for i in want], (pat, invert)
            assert oo[0] == 0 and oo[-1] == len(out) and len(oo) == len(rows) + 1
    # the search ends at a NUL; a kept string is copied whole
    nuls = [b"\0cat dog", b"a cat\0dog", b"cat dog\0", b"\0", b"cat", b"dog\0\0cat"]
    out, oo, rows = filter_lib.filter_lines(Spanner("(cat|dog)"), nuls)
    assert rows == [1, 2, 4, 5] and filter_lib.kept_strings(out, oo) == [nuls[i] for i in rows]
    out, oo, rows = filter_lib.filter_lines(Spanner("(cat|dog)"), nuls, invert=True)
    assert rows == [0, 3] and out == b"\0cat dog\0" and oo == [0, 8, 9]
    # empty matches count: x* keeps every string, the empty one included
    assert filter_lib.filter_lines(Spanner("x*"), [b"", b"b"]) == (b"b", [0, 0, 1], [0, 1])
    assert filter_lib.filter_lines(Spanner("x*"), [b"", b"b"], invert=True) == (b"", [0], [])
