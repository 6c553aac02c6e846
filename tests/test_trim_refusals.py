"""What trre_trim_device_strings (include/trre_mi355x.h) refuses before a device is touched: the return code and the whole text
of trre_last_error(), in the order the call makes its checks — a null argument (only one of d_begin and d_end among them), flags
0 or a bit outside the two defined, a sub program (with the message every other call gives it), any other program not compiled
with TRRE_MODE_SPANS, the forced backtracking family, the sizes, d_out on d_in, any other overlap among the six arrays — for every
pair of the arrays placed to overlap three ways, and, where two reasons hold at once, for which of the two is reported.  Fake
device pointers throughout, as in tests/test_column_refusals.py: no call here is one the library would take."""
import ctypes
import itertools

import trre_amd
from trre_amd import api

from test_column_refusals import (CAP, E_ARG, E_UNSUPPORTED, FIND, MATCH, N, NOT_IN_PLACE, NREC, NULL, OB, OFFSETS_ANOTHER, SCAN, SPANS,
                                  SPANS_BACKTRACK, TAKES, TOO_MANY, program)

SUB = ("[0-9]+:N", "sub")
SUB_ONLY = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only"
BAD_FLAGS = "error: flags must be TRRE_TRIM_LEFT, TRRE_TRIM_RIGHT or both"
IN_OUT = NOT_IN_PLACE % "trimmed strings"
NOUN = "trimmed strings"
RB = NREC * 8
ARRAYS = [("in", N), ("off", OB), ("out", CAP), ("ooff", OB), ("begin", RB), ("end", RB)]
BASES = {name: 0x10000000 * (i + 1) for i, (name, _) in enumerate(ARRAYS)}


def refused(prog="own", **changed):
    """one call with fake pointers: (rc, trre_last_error()); the size the call reports is 0 afterwards"""
    p = program(SPANS) if prog == "own" else prog
    a = dict(BASES)
    z = dict(n=N, nrec=NREC, cap=CAP, flags=3)
    for key, value in changed.items():
        (a if key in a else z)[key] = value
    assert set(a) == set(BASES) and len(z) == 4, changed
    m = ctypes.c_size_t(777)
    rc = api.lib().trre_trim_device_strings(p._h if p else None, a["in"], z["n"], a["off"], z["nrec"], z["flags"], a["out"], z["cap"], a["ooff"],
                                            a["begin"], a["end"], ctypes.byref(m), None)
    assert m.value == 0
    return rc, api.lib().trre_last_error().decode()


def backtracking():
    p = trre_amd.Program(SPANS[0], "nft", SPANS[1])
    p.set_kernel(trre_amd.KERNEL_BACKTRACK)
    return p


def test_the_symbol_and_the_flags():
    assert (api.TRIM_LEFT, api.TRIM_RIGHT) == (1, 2)
    assert api.lib().trre_trim_device_strings.argtypes is not None
    for name in ("trim_strings", "trim_ranges", "trim_list"):
        assert hasattr(trre_amd.Program, name)


def test_every_pair_of_arrays_overlapping():
    size = dict(ARRAYS)
    pairs = list(itertools.combinations(sorted(size), 2))
    assert len(pairs) == 15
    for x, y in pairs:
        for moved, fixed in ((x, y), (y, x)):
            for at in (BASES[fixed] + size[fixed] - 1, BASES[fixed] - size[moved] + 1, BASES[fixed] + 8):
                for flags in (1, 2, 3):
                    want = IN_OUT if {x, y} == {"in", "out"} else OFFSETS_ANOTHER
                    assert refused(flags=flags, **{moved: at}) == (E_ARG, want), (moved, fixed, hex(at))


def test_refusals_in_the_order_of_the_checks():
    assert refused(prog=None) == (E_ARG, NULL)
    for arg in ("in", "off", "out", "ooff"):
        assert refused(**{arg: None}) == (E_ARG, NULL), arg
    assert refused(ooff=None, cap=0) == (E_ARG, NULL)                        # null offsets with an output: no size query
    assert refused(begin=None) == (E_ARG, NULL) and refused(end=None) == (E_ARG, NULL)      # only one of the two
    for flags in (0, 4, 7, 1 << 31, 0xFFFFFFFC):
        assert refused(flags=flags) == (E_ARG, BAD_FLAGS), flags
    assert refused(prog=program(SUB)) == (E_ARG, SUB_ONLY)
    for spec in (SCAN, MATCH, FIND, ("a:b", "scan_all"), ("a:b", "match_all")):
        assert refused(prog=program(spec)) == (E_ARG, TAKES % (NOUN, "TRRE_MODE_SPANS")), spec
    assert refused(prog=backtracking()) == (E_UNSUPPORTED, SPANS_BACKTRACK)
    for what in ("nrec", "n"):
        assert refused(**{what: 1 << 55}) == (E_ARG, TOO_MANY), what
        rc, message = refused(**{what: (1 << 55) - 1})                       # one less passes this check: so large an array overlaps the next one
        assert rc == E_ARG and "overlaps" in message, (what, message)
    assert refused(out=BASES["in"]) == (E_ARG, IN_OUT)                       # d_in == d_out: no in-place form
    assert refused(off=BASES["in"] + 8) == (E_ARG, OFFSETS_ANOTHER)
    # the legal forms pass every one of these checks (they fail later, on the fake pointers' device: not tried here); what is
    # legal is seen from the NEXT refusal being the one reported: both ranges null, and the size query's nulls
    assert refused(begin=None, end=None, n=1 << 55) == (E_ARG, TOO_MANY)
    assert refused(out=None, ooff=None, cap=0, n=1 << 55) == (E_ARG, TOO_MANY)
    assert refused(out=None, ooff=None, cap=0, begin=None, end=None, nrec=1 << 55) == (E_ARG, TOO_MANY)


def test_of_two_reasons_the_earlier_check_is_reported():
    inside_off = {"off": BASES["in"] + 8}
    assert refused(flags=0, off=None) == (E_ARG, NULL)                                                  # null, flags
    assert refused(flags=4, begin=None) == (E_ARG, NULL)                                                # one range, flags
    assert refused(prog=program(SUB), end=None) == (E_ARG, NULL)                                        # null, sub program
    assert refused(prog=program(SUB), flags=0) == (E_ARG, BAD_FLAGS)                                    # flags, sub program
    assert refused(prog=program(FIND), flags=4) == (E_ARG, BAD_FLAGS)                                   # flags, wrong program
    assert refused(prog=backtracking(), flags=7) == (E_ARG, BAD_FLAGS)                                  # flags, family
    assert refused(prog=program(SUB), n=1 << 55) == (E_ARG, SUB_ONLY)                                   # sub program, size
    assert refused(prog=program(SCAN), n=1 << 55) == (E_ARG, TAKES % (NOUN, "TRRE_MODE_SPANS"))         # wrong program, size
    assert refused(prog=backtracking(), nrec=1 << 55) == (E_UNSUPPORTED, SPANS_BACKTRACK)               # family, size
    assert refused(n=1 << 55, **inside_off) == (E_ARG, TOO_MANY)                                        # size, overlap
    assert refused(out=BASES["in"] + 8, **inside_off) == (E_ARG, IN_OUT)                                # d_in / d_out, offsets
    assert refused(out=BASES["in"] + 8, begin=BASES["end"]) == (E_ARG, IN_OUT)                          # d_in / d_out, the ranges
    assert refused(out=BASES["in"], off=BASES["in"] + 8) == (E_ARG, IN_OUT)                             # no in-place form
