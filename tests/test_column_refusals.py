"""What the eight column calls (include/trre_mi355x.h: trre_scan_device_records, trre_scan_device_strings and the
trre_{match,find,span,split,filter,field}_device_strings) refuse before a device is touched, call by call: the return code and the
whole text of trre_last_error(), for every refusal in the order the call makes it, for every pair of the call's arrays placed to
overlap three ways, and, where two reasons hold at once, for which of the two is reported.  Fake device pointers throughout, as in
tests/test_filter_strings.py: no call here is one the library would take."""
import ctypes
import itertools

import pytest

import trre_amd
from trre_amd import api

N, NREC, CAP, XCAP = 1000, 100, 2000, 50
OB, XB, VB = (NREC + 1) * 8, (XCAP + 1) * 8, (NREC + 63) // 64 * 8
E_ARG, E_UNSUPPORTED = api.E_ARG, api.E_UNSUPPORTED

NULL = "error: null argument"
TOO_MANY = "error: too many records or bytes"
IN_PLACE_ONLY = "error: input and output overlap (only d_in == d_out, a scan in place, is allowed)"
OFFSETS_THE_OTHER = "error: an offsets array overlaps the data or the other offsets array"
OFFSETS_ANOTHER = "error: an offsets array overlaps the data or another offsets array"
BITMAP_OVERLAPS = "error: the validity bitmap overlaps the data or an offsets array"
BITMAP_ALIGNED = "error: the validity bitmap must be 8-byte aligned (it is written as 64-bit words)"
FIND_ONLY = "error: a program compiled with TRRE_MODE_FIND runs through trre_find_device_strings only"
SPANS_ONLY = ("error: a program compiled with TRRE_MODE_SPANS runs through trre_span_device_strings, trre_split_device_strings, "
              "trre_filter_device_strings and trre_field_device_strings only")
SCAN_ONLY = "error: %s are offered in scan mode only (a line of -m, -a, -ma prints zero or many newlines)"
OWN_NEWLINE = "error: the pattern can print a newline of its own: record outputs could not be told apart"
FIND_NEWLINE = "error: the pattern can print a newline of its own: the matches' outputs could not be told apart"
TAKES = "error: %s take a program compiled with %s"
NO_VERDICTS = ("error: the verdicts come from the guided tables, which this program does not have or was told not to use "
               "(the backtracking family)")
FIND_BACKTRACK = "error: find mode runs on the guided tables, which this program was told not to use (the backtracking family)"
SPANS_BACKTRACK = "error: spans mode runs on the guided tables, which this program was told not to use (the backtracking family)"
NOT_IN_PLACE = "error: the output overlaps the input (the %s are not made in place)"
UNKNOWN_FLAG = "error: unknown flag (TRRE_FILTER_INVERT is the only one)"

SCAN, MATCH, FIND, SPANS, NEWLINE = ("a:b", "scan"), ("[0-9]+:N", "match"), ("[0-9]+:N", "find"), ("[0-9]+:N", "spans"), ("x:\n", "scan")


def scan_args(a, z, k, m):
    return (a["in"], z["n"], a["off"], z["nrec"], a["out"], z["cap"], a["ooff"], m, None)


def spans_wrong_modes(noun):
    return [(mode, E_ARG, TAKES % (noun, "TRRE_MODE_SPANS")) for mode in (SCAN, MATCH, FIND)]


# per call: the arrays (name, bytes) in ascending fake addresses; the argument list; the program it takes; the arguments whose
# null is refused; the programs it refuses, in the order of the checks; the forced backtracking family's message; the sizes at
# their limits; the message of the d_in / d_out pair (None: the call has no such pair)
CALLS = {
    "records": dict(
        fn="trre_scan_device_records", arrays=[("in", N), ("off", OB), ("out", CAP), ("ooff", OB)], args=scan_args, prog=SCAN,
        nulls=["p", "in", "off", "out", "ooff"], counters="m",
        wrong=[(FIND, E_ARG, FIND_ONLY), (SPANS, E_ARG, SPANS_ONLY), (MATCH, E_UNSUPPORTED, SCAN_ONLY % "records"), (NEWLINE, E_UNSUPPORTED, OWN_NEWLINE)],
        backtrack=None, limits=[("nrec", 1 << 58), ("n", 1 << 56)], in_out=IN_PLACE_ONLY, offsets=OFFSETS_THE_OTHER),
    "strings": dict(
        fn="trre_scan_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("ooff", OB)], args=scan_args, prog=SCAN,
        nulls=["p", "in", "off", "out", "ooff"], counters="m",
        wrong=[(FIND, E_ARG, FIND_ONLY), (SPANS, E_ARG, SPANS_ONLY), (MATCH, E_UNSUPPORTED, SCAN_ONLY % "strings"), (NEWLINE, E_UNSUPPORTED, OWN_NEWLINE)],
        backtrack=None, limits=[("nrec", 1 << 55), ("n", 1 << 55)], in_out=IN_PLACE_ONLY, offsets=OFFSETS_THE_OTHER),
    "match": dict(
        fn="trre_match_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("ooff", OB), ("valid", VB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], a["out"], z["cap"], a["ooff"], a["valid"], k, m, None), prog=MATCH,
        nulls=["p", "in", "off", "out", "ooff", "valid"], counters="km",
        wrong=[(mode, E_ARG, TAKES % ("matched strings", "TRRE_MODE_MATCH")) for mode in (SCAN, FIND, SPANS)] + [(("x:\n", "match"), E_UNSUPPORTED, OWN_NEWLINE)],
        backtrack=NO_VERDICTS, limits=[("nrec", 1 << 55), ("n", 1 << 55)], in_out=IN_PLACE_ONLY, offsets=OFFSETS_THE_OTHER),
    "find": dict(
        fn="trre_find_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("xoff", XB), ("loff", OB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], a["out"], z["cap"], a["xoff"], z["xcap"], a["loff"], k, m, None), prog=FIND,
        nulls=["p", "in", "off", "out", "xoff", "loff"], counters="km",
        wrong=[(mode, E_ARG, TAKES % ("found strings", "TRRE_MODE_FIND")) for mode in (SCAN, MATCH, SPANS)] + [(("x:\n", "find"), E_UNSUPPORTED, FIND_NEWLINE)],
        backtrack=FIND_BACKTRACK, limits=[("nrec", 1 << 55), ("n", 1 << 55), ("xcap", 1 << 58)], in_out=IN_PLACE_ONLY, offsets=OFFSETS_ANOTHER),
    "span": dict(
        fn="trre_span_device_strings", arrays=[("in", N), ("off", OB), ("start", XCAP * 8), ("end", XCAP * 8), ("loff", OB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], a["start"], a["end"], z["xcap"], a["loff"], k, None), prog=SPANS,
        nulls=["p", "in", "off", "start", "end", "loff"], counters="k",
        wrong=spans_wrong_modes("match spans"),
        backtrack=SPANS_BACKTRACK, limits=[("nrec", 1 << 55), ("n", 1 << 55), ("xcap", 1 << 58)], in_out=None, offsets=OFFSETS_ANOTHER),
    "split": dict(
        fn="trre_split_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("xoff", XB), ("loff", OB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], a["out"], z["cap"], a["xoff"], z["xcap"], a["loff"], k, m, None), prog=SPANS,
        nulls=["p", "in", "off", "out", "xoff", "loff"], counters="km",
        wrong=spans_wrong_modes("split strings"),
        backtrack=SPANS_BACKTRACK, limits=[("nrec", 1 << 55), ("n", 1 << 55), ("xcap", 1 << 58)], in_out=NOT_IN_PLACE % "pieces", offsets=OFFSETS_ANOTHER),
    "filter": dict(
        fn="trre_filter_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("xoff", XB), ("rows", XCAP * 8)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], z["flags"], a["out"], z["cap"], a["xoff"], a["rows"], z["xcap"], k, m, None),
        prog=SPANS, nulls=["p", "in", "off", "out", "xoff", "rows"], counters="km",
        wrong=spans_wrong_modes("filtered strings"),
        backtrack=SPANS_BACKTRACK, limits=[("nrec", 1 << 55), ("n", 1 << 55), ("xcap", 1 << 58)], in_out=NOT_IN_PLACE % "kept strings", offsets=OFFSETS_ANOTHER),
    "field": dict(
        fn="trre_field_device_strings", arrays=[("in", N), ("off", OB), ("out", CAP), ("ooff", OB), ("valid", VB)],
        args=lambda a, z, k, m: (a["in"], z["n"], a["off"], z["nrec"], z["field"], a["out"], z["cap"], a["ooff"], a["valid"], k, m, None), prog=SPANS,
        nulls=["p", "in", "off", "out", "ooff", "valid"], counters="km",
        wrong=spans_wrong_modes("field strings"),
        backtrack=SPANS_BACKTRACK, limits=[("nrec", 1 << 55), ("n", 1 << 55)], in_out=NOT_IN_PLACE % "fields", offsets=OFFSETS_ANOTHER),
}
EVERY_CALL = pytest.mark.parametrize("name", sorted(CALLS))

_programs = {}


def program(spec):
    if spec not in _programs:
        _programs[spec] = trre_amd.Program(spec[0], "nft", spec[1])
    return _programs[spec]


def bases(call):
    return {name: 0x10000000 * (i + 1) for i, (name, _) in enumerate(call["arrays"])}


def refused(call, prog="own", **changed):
    """one call with fake pointers: (rc, trre_last_error()); the sizes the call reports are 0 afterwards"""
    p = program(call["prog"]) if prog == "own" else prog
    a = bases(call)
    z = dict(n=N, nrec=NREC, cap=CAP, xcap=XCAP, flags=0, field=1)
    for key, value in changed.items():
        (a if key in a else z)[key] = value
    assert set(a) == set(bases(call)) and len(z) == 6, changed
    k, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = getattr(api.lib(), call["fn"])(p._h if p else None, *call["args"](a, z, ctypes.byref(k), ctypes.byref(m)))
    assert [c.value for c, x in ((k, "k"), (m, "m")) if x in call["counters"]] == [0] * len(call["counters"])
    return rc, api.lib().trre_last_error().decode()


def pair_message(call, x, y):
    if {x, y} == {"in", "out"}:
        return call["in_out"]
    return BITMAP_OVERLAPS if "valid" in (x, y) else call["offsets"]


def backtracking(call):
    p = trre_amd.Program(call["prog"][0], "nft", call["prog"][1])
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    return p


@EVERY_CALL
def test_every_pair_of_arrays_overlapping(name):
    """each pair sharing its last / first byte either way round, and one array starting inside the other (the bitmap, moved, at
    the nearest 8-byte aligned address that still overlaps)"""
    call = CALLS[name]
    size, base = dict(call["arrays"]), bases(call)
    pairs = list(itertools.combinations(sorted(size), 2))
    assert len(pairs) == len(size) * (len(size) - 1) // 2
    for x, y in pairs:
        for moved, fixed in ((x, y), (y, x)):
            for at in (base[fixed] + size[fixed] - 1, base[fixed] - size[moved] + 1, base[fixed] + 8):
                if moved == "valid":
                    at = (at + 7) & ~7 if at < base[fixed] else at & ~7
                assert refused(call, **{moved: at}) == (E_ARG, pair_message(call, x, y)), (moved, fixed, hex(at))


@EVERY_CALL
def test_refusals_in_the_order_of_the_checks(name):
    call = CALLS[name]
    for arg in call["nulls"]:
        assert (refused(call, prog=None) if arg == "p" else refused(call, **{arg: None})) == (E_ARG, NULL), arg
    if name == "filter":
        for flags in (2, 3, 1 << 31):
            assert refused(call, flags=flags) == (E_ARG, UNKNOWN_FLAG), flags
    for spec, rc, message in call["wrong"]:
        assert refused(call, prog=program(spec)) == (rc, message), spec
    if call["backtrack"]:
        assert refused(call, prog=backtracking(call)) == (E_UNSUPPORTED, call["backtrack"])
    for what, limit in call["limits"]:
        assert refused(call, **{what: limit}) == (E_ARG, TOO_MANY), what
        rc, message = refused(call, **{what: limit - 1})                 # one less passes this check: so large an array overlaps the next one
        assert rc == E_ARG and ("overlaps" in message or "overlap " in message), (what, message)
    if "valid" in dict(call["arrays"]):
        for by in (1, 4):
            assert refused(call, valid=bases(call)["valid"] + by) == (E_ARG, BITMAP_ALIGNED), by


@EVERY_CALL
def test_of_two_reasons_the_earlier_check_is_reported(name):
    call = CALLS[name]
    base, size = bases(call), dict(call["arrays"])
    wrong, wrong_rc, wrong_message = call["wrong"][-1]
    limit, at_limit = call["limits"][0]
    assert refused(call, prog=program(wrong), off=None) == (E_ARG, NULL)                                      # null, wrong program
    if name == "filter":
        assert refused(call, flags=2, off=None) == (E_ARG, NULL)                                              # null, flag
        assert refused(call, prog=program(wrong), flags=2) == (E_ARG, UNKNOWN_FLAG)                            # flag, wrong program
    assert refused(call, prog=program(wrong), **{limit: at_limit}) == (wrong_rc, wrong_message)              # wrong program, size
    if call["backtrack"]:
        assert refused(call, prog=backtracking(call), **{limit: at_limit}) == (E_UNSUPPORTED, call["backtrack"])    # family, size
    inside_off = {"off": base["in"] + 8}
    if "valid" in size:
        assert refused(call, valid=base["valid"] + 4, **{limit: at_limit}) == (E_ARG, TOO_MANY)              # size, alignment
        assert refused(call, valid=base["valid"] + 4, **inside_off) == (E_ARG, BITMAP_ALIGNED)               # alignment, overlap
        assert refused(call, valid=base["in"] + 16, **inside_off) == (E_ARG, call["offsets"])                 # offsets, bitmap
    else:
        assert refused(call, **{limit: at_limit}, **inside_off) == (E_ARG, TOO_MANY)                          # size, overlap
    if call["in_out"]:
        assert refused(call, out=base["in"] + 8, **inside_off) == (E_ARG, call["in_out"])                     # d_in / d_out, offsets
        if "valid" in size:
            assert refused(call, out=base["in"] + 8, valid=base["in"] + 16) == (E_ARG, call["in_out"])        # d_in / d_out, bitmap


def test_in_place_is_for_the_scan_mode_calls_alone():
    """d_in == d_out passes the pair's check in the records, strings, match and find calls — the next refusal is reported — and is
    refused by the calls that make nothing in place"""
    for name, call in CALLS.items():
        if not call["in_out"]:
            continue
        base = bases(call)
        rc, message = refused(call, out=base["in"], off=base["in"] + 8)
        assert (rc, message) == (E_ARG, call["offsets"] if call["in_out"] == IN_PLACE_ONLY else call["in_out"]), name
