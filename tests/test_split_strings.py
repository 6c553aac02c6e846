"""Split strings (include/trre_mi355x.h: trre_split_device_strings; Program.split_strings / split_list) without a GPU: the
refusals that are found before the device is touched — with fake device pointers, as tests/test_span_strings.py does for the span
call — and the pieces' definition of tests/split_lib.py against re.split through the oracle's spans."""
import ctypes
import re

import split_lib
import trre_amd
from span_lib import Spanner
from trre_amd import api

IN, OFF, OUT, POFF, LOFF = 0x10000000, 0x30000000, 0x20000000, 0x40000000, 0x50000000


def split_rc(p, d_in=IN, d_off=OFF, d_out=OUT, d_poff=POFF, d_loff=LOFF, cap=2000, pcap=50):
    """fake device pointers: callers pass an overlap or a program the call refuses — every one is refused before anything touches
    a device; both sizes are 0 then"""
    k, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = api.lib().trre_split_device_strings(p._h if p else None, d_in, 1000, d_off, 10, d_out, cap, d_poff, pcap, d_loff, ctypes.byref(k),
                                             ctypes.byref(m), None)
    assert k.value == 0 and m.value == 0
    return rc


def last():
    return api.lib().trre_last_error().decode()


def test_library_exports_split_symbol():
    assert hasattr(api.lib(), "trre_split_device_strings")
    for name in ("split_strings", "split_list"):
        assert hasattr(trre_amd.Program, name)


def test_programs_the_call_refuses():
    for mode in ("scan_all", "match_all", "scan", "match", "find"):
        assert split_rc(trre_amd.Program("a:b", "nft", mode)) == api.E_ARG and "TRRE_MODE_SPANS" in last()
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert split_rc(p) == api.E_UNSUPPORTED and "backtracking" in last()
    p.set_kernel(trre_amd.KERNEL_AUTO)
    assert split_rc(p, pcap=1 << 58) == api.E_ARG and "too many" in last()
    L = api.lib()
    assert L.trre_split_device_strings(p._h, IN, 1 << 55, OFF, 10, OUT, 2000, POFF, 50, LOFF, None, None, None) == api.E_ARG and "too many" in last()
    assert L.trre_split_device_strings(p._h, IN, 1000, OFF, 1 << 55, OUT, 2000, POFF, 50, LOFF, None, None, None) == api.E_ARG and "too many" in last()


def test_nulls_are_refused():
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    E = api.E_ARG
    assert split_rc(None) == E
    assert split_rc(p, d_in=None) == E and split_rc(p, d_off=None) == E and split_rc(p, d_loff=None) == E
    assert split_rc(p, d_out=None) == E and split_rc(p, d_poff=None) == E              # null with room promised
    assert "null argument" in last()


def test_every_pairwise_overlap_is_refused():
    """d_in 1000 bytes, d_off and d_list_off 88 bytes, d_out 2000 bytes, d_piece_off 408 bytes: each pair sharing its last / first
    byte, and one array inside another"""
    p = trre_amd.Program("[0-9]+:N", "nft", "spans")
    E = api.E_ARG
    assert split_rc(p, d_out=IN + 999) == E and "not made in place" in last()           # in / out
    assert split_rc(p, d_out=IN) == E and split_rc(p, d_out=IN - 1999) == E             # (d_in == d_out: no in-place form)
    assert split_rc(p, d_off=IN + 999) == E and "offsets array overlaps" in last()      # in / off
    assert split_rc(p, d_loff=IN - 87) == E                                             # in / list offsets
    assert split_rc(p, d_poff=IN + 500) == E                                            # in / piece offsets
    assert split_rc(p, d_off=OUT + 1999) == E                                           # out / off
    assert split_rc(p, d_loff=OUT + 8) == E                                             # out / list offsets
    assert split_rc(p, d_poff=OUT - 407) == E                                           # out / piece offsets
    assert split_rc(p, d_loff=OFF + 80) == E                                            # off / list offsets
    assert split_rc(p, d_poff=OFF + 87) == E                                            # off / piece offsets
    assert split_rc(p, d_poff=LOFF - 400) == E                                          # piece offsets / list offsets


def test_pieces_by_the_definition_are_re_split():
    """the yardstick itself: pieces cut from the oracle's spans are what re.split gives, for patterns both understand"""
    lines = [b"a,b,,c", b"", b",", b"no comma", b",,", b"x,"]
    per = split_lib.split_lines(Spanner(","), lines)
    assert per[:3] == [[b"a", b"b", b"", b"c"], [b""], [b"", b""]]
    assert per == [re.split(b",", l) for l in lines]
    assert split_lib.split_lines(Spanner("x*"), [b"bb"]) == [[b"", b"b", b"b", b""]] == [re.split(b"x*", b"bb")]
    nums = [b"12ab345", b"ab", b"7", b"a1b22c333"]
    assert split_lib.split_lines(Spanner("[0-9]+"), nums) == [re.split(b"[0-9]+", l) for l in nums]
    # the search ends at a NUL: the last piece keeps it and everything behind it
    assert split_lib.split_lines(Spanner("(cat|dog)"), [b"a cat\0dog", b"\0cat", b"cat dog\0"]) == [[b"a ", b"\0dog"], [b"\0cat"], [b"", b" ", b"\0"]]
    out, po, lo = split_lib.expect(per)
    assert out == b"abcno commax" and lo == [0, 4, 5, 7, 8, 11, 13] and po[-1] == len(out) and len(po) == lo[-1] + 1
    assert split_lib.per_string(out, po, lo) == per
