"""What trre_nth_device_strings refuses before a device is touched — the return code and the whole text of trre_last_error(), for
every refusal in the order the call makes it, for every pair of its five arrays placed to overlap three ways, and for programs
of every other mode.  Fake device pointers throughout, in the manner of tests/test_sub_refusals.py: no call here is one the
library would take."""
import ctypes
import itertools

import trre_amd
from trre_amd import api

N, NREC, CAP = 1000, 100, 2000
OB, VB = (NREC + 1) * 8, (NREC + 63) // 64 * 8
ARRAYS = [("in", N), ("off", OB), ("out", CAP), ("ooff", OB), ("valid", VB)]
BASES = {name: 0x10000000 * (i + 1) for i, (name, _) in enumerate(ARRAYS)}
E_ARG, E_UNSUPPORTED = api.E_ARG, api.E_UNSUPPORTED

NULL = "error: null argument"
SUB_ONLY = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only"
TAKES = "error: match k of every string takes a program compiled with TRRE_MODE_FIND"
NEWLINE = "error: the pattern can print a newline of its own: the matches' outputs could not be told apart"
BACKTRACK = "error: find mode runs on the guided tables, which this program was told not to use (the backtracking family)"
TOO_MANY = "error: too many records or bytes"
ALIGNED = "error: the validity bitmap must be 8-byte aligned (it is written as 64-bit words)"
NOT_IN_PLACE = "error: the output overlaps the input (the selected matches are not made in place)"
OFFSETS = "error: an offsets array overlaps the data or another offsets array"
BITMAP = "error: the validity bitmap overlaps the data or an offsets array"

_programs = {}


def program(pattern="[0-9]+:N", mode="find"):
    if (pattern, mode) not in _programs:
        _programs[(pattern, mode)] = trre_amd.Program(pattern, "nft", mode)
    return _programs[(pattern, mode)]


def backtracking():
    p = trre_amd.Program("[0-9]+:N", "nft", "find")
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    return p


def refused(prog="own", **changed):
    """one call with fake pointers: (rc, trre_last_error()); both sizes are 0 afterwards"""
    p = program() if prog == "own" else prog
    a = dict(BASES)
    z = dict(n=N, nrec=NREC, cap=CAP, k=0)
    for key, value in changed.items():
        (a if key in a else z)[key] = value
    assert len(a) == 5 and len(z) == 4, changed
    v, m = ctypes.c_size_t(777), ctypes.c_size_t(777)
    rc = api.lib().trre_nth_device_strings(p._h if p else None, a["in"], z["n"], a["off"], z["nrec"], z["k"], a["out"], z["cap"], a["ooff"],
                                           a["valid"], ctypes.byref(v), ctypes.byref(m), None)
    assert (v.value, m.value) == (0, 0)
    return rc, api.lib().trre_last_error().decode()


def test_refusals_in_the_order_of_the_checks():
    assert refused(prog=None) == (E_ARG, NULL)
    for arg in ("in", "off", "out", "ooff", "valid"):
        assert refused(**{arg: None}) == (E_ARG, NULL), arg
    assert refused(ooff=None, cap=0) == (E_ARG, NULL) and refused(out=None, ooff=None) == (E_ARG, NULL)      # no size query with an output or room
    assert refused(prog=program("[0-9]+:N", "sub")) == (E_ARG, SUB_ONLY)
    for mode in ("scan", "match", "spans", "scan_all", "match_all"):
        assert refused(prog=program("[0-9]+:N", mode)) == (E_ARG, TAKES), mode
    assert refused(prog=program("x:\n")) == (E_UNSUPPORTED, NEWLINE)
    assert refused(prog=backtracking()) == (E_UNSUPPORTED, BACKTRACK)
    for what in ("nrec", "n"):
        assert refused(**{what: 1 << 55}) == (E_ARG, TOO_MANY), what
        rc, message = refused(**{what: (1 << 55) - 1})                   # one less passes this check: so large an array overlaps the next one
        assert rc == E_ARG and "overlaps" in message, (what, message)
    for mis in range(1, 8):
        assert refused(valid=BASES["valid"] + mis) == (E_ARG, ALIGNED), mis
    assert refused(out=BASES["in"] + 8) == (E_ARG, NOT_IN_PLACE)
    assert refused(off=BASES["in"] + 8) == (E_ARG, OFFSETS)
    assert refused(valid=BASES["in"] + 8) == (E_ARG, BITMAP)
    for k in (0, 1, -1, (1 << 63) - 1, -(1 << 63)):                      # any k is legal: the refusal is the overlap's
        assert refused(k=k, valid=BASES["off"]) == (E_ARG, BITMAP), k


def test_of_two_reasons_the_earlier_check_is_reported():
    wrong, sub, nl = program("[0-9]+:N", "spans"), program("[0-9]+:N", "sub"), program("x:\n")
    assert refused(prog=wrong, off=None) == (E_ARG, NULL)                                    # null, wrong program
    assert refused(prog=sub, n=1 << 55) == (E_ARG, SUB_ONLY)                                 # sub program, size
    assert refused(prog=wrong, n=1 << 55) == (E_ARG, TAKES)                                  # wrong program, size
    assert refused(prog=program("x:\n", "spans")) == (E_ARG, TAKES)                          # wrong program, newline
    nlb = trre_amd.Program("x:\n", "nft", "find")
    nlb.set_kernel(trre_amd.KERNEL_BACKTRACK)
    assert refused(prog=nlb) == (E_UNSUPPORTED, NEWLINE)                                     # newline, family
    assert refused(prog=nl, n=1 << 55) == (E_UNSUPPORTED, NEWLINE)                           # newline, size
    assert refused(prog=backtracking(), n=1 << 55) == (E_UNSUPPORTED, BACKTRACK)             # family, size
    assert refused(n=1 << 55, valid=BASES["valid"] + 4) == (E_ARG, TOO_MANY)                 # size, alignment
    assert refused(valid=BASES["in"] + 4) == (E_ARG, ALIGNED)                                # alignment, overlap
    assert refused(out=BASES["in"] + 8, off=BASES["in"] + 8) == (E_ARG, NOT_IN_PLACE)        # d_in / d_out, offsets
    assert refused(out=BASES["in"]) == (E_ARG, NOT_IN_PLACE)                                 # (d_in == d_out: no in-place form)
    assert refused(off=BASES["in"] + 8, valid=BASES["in"] + 8) == (E_ARG, OFFSETS)           # offsets, bitmap


def test_every_pair_of_arrays_overlapping():
    """each pair sharing its last / first byte either way round, and one array starting inside the other (the bitmap moved by
    whole words: it stays aligned)"""
    size = dict(ARRAYS)
    pairs = list(itertools.combinations(sorted(size), 2))
    assert len(pairs) == 10
    for x, y in pairs:
        want = BITMAP if "valid" in (x, y) else NOT_IN_PLACE if {x, y} == {"in", "out"} else OFFSETS
        for moved, fixed in ((x, y), (y, x)):
            places = (BASES[fixed] + size[fixed] - 1, BASES[fixed] - size[moved] + 1, BASES[fixed] + 8)
            if moved == "valid":
                places = ((BASES[fixed] + size[fixed] - 1) & ~7, BASES[fixed] - size[moved] + 8, BASES[fixed] + 8)
            for at in places:
                assert refused(**{moved: at}) == (E_ARG, want), (moved, fixed, hex(at))


def test_the_size_query_passes_the_entry_checks_up_to_the_overlaps():
    """d_out and d_out_off null with cap == 0 is the size query: not a null argument — the refusal is a later one"""
    assert refused(out=None, ooff=None, cap=0, valid=BASES["off"]) == (E_ARG, BITMAP)
    assert refused(out=None, ooff=None, cap=0, off=BASES["in"] + 992) == (E_ARG, OFFSETS)
