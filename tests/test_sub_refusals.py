"""What trre_sub_device_strings refuses before a device is touched — the return code and the whole text of trre_last_error(),
for every refusal in the order the call makes it, for every pair of its four arrays placed to overlap three ways, for first < 0
and the limits — and what the eight other column calls say to a program compiled with TRRE_MODE_SUB.  Fake device pointers
throughout, in the manner of tests/test_column_refusals.py: no call here is one the library would take."""
import ctypes
import itertools

import trre_amd
from test_column_refusals import CALLS, refused as column_refused
from trre_amd import api

N, NREC, CAP = 1000, 100, 2000
OB = (NREC + 1) * 8
ARRAYS = [("in", N), ("off", OB), ("out", CAP), ("ooff", OB)]
BASES = {name: 0x10000000 * (i + 1) for i, (name, _) in enumerate(ARRAYS)}
E_ARG, E_UNSUPPORTED = api.E_ARG, api.E_UNSUPPORTED

NULL = "error: null argument"
TAKES = "error: replaced strings take a program compiled with TRRE_MODE_SUB"
NEWLINE = "error: the pattern can print a newline of its own: the matches' outputs could not be told apart"
BACKTRACK = "error: sub mode runs on the guided tables, which this program was told not to use (the backtracking family)"
FIRST = "error: first must not be negative (count < 0 selects every match from first on)"
TOO_MANY = "error: too many records or bytes"
NOT_IN_PLACE = "error: the output overlaps the input (the replaced strings are not made in place)"
OFFSETS = "error: an offsets array overlaps the data or another offsets array"
SUB_ONLY = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only"

_programs = {}


def program(pattern="[0-9]+:N", mode="sub"):
    if (pattern, mode) not in _programs:
        _programs[(pattern, mode)] = trre_amd.Program(pattern, "nft", mode)
    return _programs[(pattern, mode)]


def backtracking():
    p = trre_amd.Program("[0-9]+:N", "nft", "sub")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    return p


def refused(prog="own", **changed):
    """one call with fake pointers: (rc, trre_last_error()); both sizes are 0 afterwards"""
    p = program() if prog == "own" else prog
    a = dict(BASES)
    z = dict(n=N, nrec=NREC, cap=CAP, first=0, count=-1)
    for key, value in changed.items():
        (a if key in a else z)[key] = value
    assert len(a) == 4 and len(z) == 5, changed
    r, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = api.lib().trre_sub_device_strings(p._h if p else None, a["in"], z["n"], a["off"], z["nrec"], z["first"], z["count"], a["out"], z["cap"],
                                           a["ooff"], ctypes.byref(r), ctypes.byref(m), None)
    assert (r.value, m.value) == (0, 0)
    return rc, api.lib().trre_last_error().decode()


def test_refusals_in_the_order_of_the_checks():
    assert refused(prog=None) == (E_ARG, NULL)
    for arg in ("in", "off", "out", "ooff"):
        assert refused(**{arg: None}) == (E_ARG, NULL), arg
    assert refused(ooff=None, cap=0) == (E_ARG, NULL) and refused(out=None, ooff=None) == (E_ARG, NULL)      # no size query with an output or room
    for mode in ("scan", "match", "find", "spans", "scan_all", "match_all"):
        assert refused(prog=program("[0-9]+:N", mode)) == (E_ARG, TAKES), mode
    assert refused(prog=program("x:\n")) == (E_UNSUPPORTED, NEWLINE)
    assert refused(prog=backtracking()) == (E_UNSUPPORTED, BACKTRACK)
    for first in (-1, -2, -(1 << 63)):
        for count in (-1, 0, 1):
            assert refused(first=first, count=count) == (E_ARG, FIRST), (first, count)
    for what in ("nrec", "n"):
        assert refused(**{what: 1 << 55}) == (E_ARG, TOO_MANY), what
        rc, message = refused(**{what: (1 << 55) - 1})                   # one less passes this check: so large an array overlaps the next one
        assert rc == E_ARG and "overlaps" in message, (what, message)


def test_of_two_reasons_the_earlier_check_is_reported():
    wrong, nl = program("[0-9]+:N", "spans"), program("x:\n")
    assert refused(prog=wrong, off=None) == (E_ARG, NULL)                                    # null, wrong program
    assert refused(prog=wrong, first=-1) == (E_ARG, TAKES)                                   # wrong program, first
    assert refused(prog=nl, first=-1) == (E_UNSUPPORTED, NEWLINE)                            # newline, first
    assert refused(prog=backtracking(), first=-1) == (E_UNSUPPORTED, BACKTRACK)              # family, first
    assert refused(first=-1, n=1 << 55) == (E_ARG, FIRST)                                    # first, size
    assert refused(n=1 << 55, off=BASES["in"] + 8) == (E_ARG, TOO_MANY)                      # size, overlap
    assert refused(out=BASES["in"] + 8, off=BASES["in"] + 8) == (E_ARG, NOT_IN_PLACE)        # d_in / d_out, offsets
    assert refused(out=BASES["in"]) == (E_ARG, NOT_IN_PLACE)                                 # (d_in == d_out: no in-place form)


def test_every_pair_of_arrays_overlapping():
    """each pair sharing its last / first byte either way round, and one array starting inside the other"""
    size = dict(ARRAYS)
    pairs = list(itertools.combinations(sorted(size), 2))
    assert len(pairs) == 6
    for x, y in pairs:
        for moved, fixed in ((x, y), (y, x)):
            for at in (BASES[fixed] + size[fixed] - 1, BASES[fixed] - size[moved] + 1, BASES[fixed] + 8):
                assert refused(**{moved: at}) == (E_ARG, NOT_IN_PLACE if {x, y} == {"in", "out"} else OFFSETS), (moved, fixed, hex(at))


def test_every_other_call_refuses_a_sub_program():
    """the eight existing column calls, and the plain scan calls: TRRE_E_ARG and one fixed message"""
    p = program()
    assert sorted(CALLS) == ["field", "filter", "find", "match", "records", "span", "split", "strings"]
    for name, call in CALLS.items():
        assert column_refused(call, prog=p) == (E_ARG, SUB_ONLY), name
    L = api.lib()
    m = ctypes.c_size_t(777)
    assert L.trre_scan_device(p._h, BASES["in"], N, BASES["out"], CAP, ctypes.byref(m), None) == E_ARG and m.value == 0
    assert L.trre_last_error().decode() == SUB_ONLY
    assert L.trre_scan_enqueue(p._h, BASES["in"], N, BASES["out"], CAP, None) == E_ARG and L.trre_last_error().decode() == SUB_ONLY
    out = ctypes.create_string_buffer(64)
    assert L.trre_scan_host(p._h, b"12 ab", 5, out, 64, ctypes.byref(m), 0) == E_ARG and L.trre_last_error().decode() == SUB_ONLY
    assert L.trre_scan_host_multi(p._h, b"12 ab", 5, out, 64, ctypes.byref(m), 1) == E_ARG and L.trre_last_error().decode() == SUB_ONLY
