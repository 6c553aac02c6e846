"""What trre_splitn_device_strings and trre_fieldn_device_strings (include/trre_mi355x.h) refuse before a device is touched: the
return code and the whole text of trre_last_error(), in the order the calls make their checks — a null argument, a flag bit other
than TRRE_SPLIT_FROM_END, a sub program (with the message every other call gives it), any other program not compiled with
TRRE_MODE_SPANS, the forced backtracking family, the sizes, the bitmap's alignment, the overlaps — with the split and field
calls' codes and messages, for every pair of the arrays placed to overlap three ways, and, where two reasons hold at once, for
which of the two is reported.  Fake device pointers throughout, as in tests/test_column_refusals.py: no call here is one the
library would take."""
import ctypes
import itertools

import pytest

import trre_amd
from trre_amd import api

from test_column_refusals import (BITMAP_ALIGNED, BITMAP_OVERLAPS, CAP, E_ARG, E_UNSUPPORTED, FIND, MATCH, N, NOT_IN_PLACE, NREC, NULL, OB,
                                  OFFSETS_ANOTHER, SCAN, SPANS, SPANS_BACKTRACK, TAKES, TOO_MANY, VB, XB, XCAP, program)

SUB = ("[0-9]+:N", "sub")
SUB_ONLY = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only"
UNKNOWN_FLAG = "error: unknown flag (TRRE_SPLIT_FROM_END is the only one)"

CALLS = {
    "splitn": dict(
        fn="trre_splitn_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("xoff", XB), ("loff", OB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], z["limit"], z["flags"], a["out"], z["cap"], a["xoff"], z["xcap"], a["loff"],
                                 k, m, None),
        nulls=["p", "in", "off", "out", "xoff", "loff"], noun="split strings",
        limits=[("nrec", 1 << 55), ("n", 1 << 55), ("xcap", 1 << 58)], in_out=NOT_IN_PLACE % "pieces"),
    "fieldn": dict(
        fn="trre_fieldn_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("ooff", OB), ("valid", VB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], z["field"], z["limit"], z["flags"], a["out"], z["cap"], a["ooff"], a["valid"],
                                 k, m, None),
        nulls=["p", "in", "off", "out", "ooff", "valid"], noun="field strings",
        limits=[("nrec", 1 << 55), ("n", 1 << 55)], in_out=NOT_IN_PLACE % "fields"),
}
BOTH = pytest.mark.parametrize("name", sorted(CALLS))


def bases(call):
    return {name: 0x10000000 * (i + 1) for i, (name, _) in enumerate(call["arrays"])}


def refused(call, prog="own", **changed):
    """one call with fake pointers: (rc, trre_last_error()); both sizes the call reports are 0 afterwards"""
    p = program(SPANS) if prog == "own" else prog
    a = bases(call)
    z = dict(n=N, nrec=NREC, cap=CAP, xcap=XCAP, flags=0, field=1, limit=1)
    for key, value in changed.items():
        (a if key in a else z)[key] = value
    assert set(a) == set(bases(call)) and len(z) == 7, changed
    k, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = getattr(api.lib(), call["fn"])(p._h if p else None, *call["args"](a, z, ctypes.byref(k), ctypes.byref(m)))
    assert (k.value, m.value) == (0, 0)
    return rc, api.lib().trre_last_error().decode()


def backtracking():
    p = trre_amd.Program(SPANS[0], "nft", SPANS[1])
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    return p


def pair_message(call, x, y):
    if {x, y} == {"in", "out"}:
        return call["in_out"]
    return BITMAP_OVERLAPS if "valid" in (x, y) else OFFSETS_ANOTHER


def test_the_symbols_and_the_flag():
    assert api.SPLIT_FROM_END == 1
    for call in CALLS.values():
        assert getattr(api.lib(), call["fn"]).argtypes is not None


@BOTH
def test_every_pair_of_arrays_overlapping(name):
    call = CALLS[name]
    size, base = dict(call["arrays"]), bases(call)
    pairs = list(itertools.combinations(sorted(size), 2))
    assert len(pairs) == 10
    for x, y in pairs:
        for moved, fixed in ((x, y), (y, x)):
            for at in (base[fixed] + size[fixed] - 1, base[fixed] - size[moved] + 1, base[fixed] + 8):
                if moved == "valid":
                    at = (at + 7) & ~7 if at < base[fixed] else at & ~7
                for flags in (0, 1):
                    assert refused(call, flags=flags, **{moved: at}) == (E_ARG, pair_message(call, x, y)), (moved, fixed, hex(at))


@BOTH
def test_refusals_in_the_order_of_the_checks(name):
    call = CALLS[name]
    for arg in call["nulls"]:
        assert (refused(call, prog=None) if arg == "p" else refused(call, **{arg: None})) == (E_ARG, NULL), arg
    for flags in (2, 3, 1 << 31, 0xFFFFFFFE):
        assert refused(call, flags=flags) == (E_ARG, UNKNOWN_FLAG), flags
    assert refused(call, prog=program(SUB)) == (E_ARG, SUB_ONLY)
    for spec in (SCAN, MATCH, FIND):
        assert refused(call, prog=program(spec)) == (E_ARG, TAKES % (call["noun"], "TRRE_MODE_SPANS")), spec
    assert refused(call, prog=backtracking()) == (E_UNSUPPORTED, SPANS_BACKTRACK)
    for what, limit in call["limits"]:
        assert refused(call, **{what: limit}) == (E_ARG, TOO_MANY), what
        rc, message = refused(call, **{what: limit - 1})                 # one less passes this check: so large an array overlaps the next one
        assert rc == E_ARG and ("overlaps" in message or "overlap " in message), (what, message)
    if name == "fieldn":
        for by in (1, 4):
            assert refused(call, valid=bases(call)["valid"] + by) == (E_ARG, BITMAP_ALIGNED), by
    # any limit and any k are legal: the next refusal is the one reported
    for limit in (0, -1, (1 << 63) - 1, -(1 << 63)):
        assert refused(call, limit=limit, field=-(1 << 63), off=None) == (E_ARG, NULL)
        assert refused(call, limit=limit, n=1 << 55) == (E_ARG, TOO_MANY)


@BOTH
def test_of_two_reasons_the_earlier_check_is_reported(name):
    call = CALLS[name]
    base = bases(call)
    limit, at_limit = call["limits"][0]
    inside_off = {"off": base["in"] + 8}
    assert refused(call, flags=2, off=None) == (E_ARG, NULL)                                                  # null, flag
    assert refused(call, prog=program(SUB), off=None) == (E_ARG, NULL)                                        # null, sub program
    assert refused(call, prog=program(SUB), flags=2) == (E_ARG, UNKNOWN_FLAG)                                 # flag, sub program
    assert refused(call, prog=program(FIND), flags=4) == (E_ARG, UNKNOWN_FLAG)                                # flag, wrong program
    assert refused(call, prog=program(SUB), **{limit: at_limit}) == (E_ARG, SUB_ONLY)                         # sub program, size
    assert refused(call, prog=program(SCAN), **{limit: at_limit}) == (E_ARG, TAKES % (call["noun"], "TRRE_MODE_SPANS"))    # wrong program, size
    assert refused(call, prog=backtracking(), **{limit: at_limit}) == (E_UNSUPPORTED, SPANS_BACKTRACK)       # family, size
    if name == "fieldn":
        assert refused(call, valid=base["valid"] + 4, **{limit: at_limit}) == (E_ARG, TOO_MANY)              # size, alignment
        assert refused(call, valid=base["valid"] + 4, **inside_off) == (E_ARG, BITMAP_ALIGNED)               # alignment, overlap
        assert refused(call, valid=base["in"] + 16, **inside_off) == (E_ARG, OFFSETS_ANOTHER)                 # offsets, bitmap
        assert refused(call, out=base["in"] + 8, valid=base["in"] + 16) == (E_ARG, call["in_out"])            # d_in / d_out, bitmap
    else:
        assert refused(call, **{limit: at_limit}, **inside_off) == (E_ARG, TOO_MANY)                          # size, overlap
    assert refused(call, out=base["in"] + 8, **inside_off) == (E_ARG, call["in_out"])                         # d_in / d_out, offsets
    assert refused(call, out=base["in"], off=base["in"] + 8) == (E_ARG, call["in_out"])                       # no in-place form
