"""Ragged records (include/trre_mi355x.h: trre_scan_device_records) without a GPU.

The device path rests on one identity: a copy of the input whose records' last bytes are '\\n' (the staged copy) holds exactly
the records' lines, so the scan of that copy is the concatenation of the records' own outputs, and — every line printing one
framing '\\n' and, for the programs the path takes, no other — record i's output ends just past output newline R_i, the number
of '\\n' in staged[0, off[i+1]).  It is pinned here on the oracle over every golden vector cut at random points (inside lines,
empty records, records without '\\n', NULs), with the compiled reference for the framing of a record without a trailing newline
where it is present.  Then the refusals that need no device: modes other than scan, programs that can print a '\\n' of their
own, overlapping offset arrays."""
import ctypes
import os
import random
import sys

import pytest

import golden_lib
import trre_amd
from oracle_lib import Oracle, OracleError, ref_available, ref_scan
from trre_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def staged_copy(data, off):
    b = bytearray(data)
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            b[off[i + 1] - 1] = 10
    return bytes(b)


def random_offsets(rng, data):
    """cut points anywhere (inside lines too), right behind some newlines, and repeated (empty records)"""
    n = len(data)
    cuts = [rng.randrange(n + 1) for _ in range(rng.randrange(0, 12))]
    nls = [i + 1 for i, c in enumerate(data) if c == 10]
    if nls:
        cuts += rng.sample(nls, min(len(nls), rng.randrange(0, 4)))
    if cuts and rng.random() < 0.4:
        cuts += [rng.choice(cuts)] * 2
    return [0] + sorted(cuts) + [n]


# ---- fake device pointers: every call below is refused on the host before anything touches a device -------------------
IN, OUT, OFF, OOFF = 0x10000000, 0x20000000, 0x30000000, 0x40000000
N, NREC, CAP = 1000, 10, 2000


def records_rc(p, d_in=IN, d_out=OUT, d_off=OFF, d_ooff=OFF + 8, n=N, nrec=NREC, cap=CAP):
    """(the offset arrays overlap unless the caller says otherwise: no call here can get as far as a device)"""
    m = ctypes.c_size_t(12345)
    rc = api.lib().trre_scan_device_records(p._h, d_in, n, d_off, nrec, d_out, cap, d_ooff, ctypes.byref(m), None)
    return rc


def prints_newline(p):
    """the program is refused for printing a '\\n' of its own: asked with overlapping offset arrays, which every program
    taken is refused for (TRRE_E_ARG) after the pattern checks"""
    rc = records_rc(p)
    assert rc in (api.E_UNSUPPORTED, api.E_ARG), rc
    return rc == api.E_UNSUPPORTED


@pytest.mark.parametrize("engine", ["nft", "dft"])
def test_staging_identity_on_golden_vectors(engine):
    """every golden scan vector the reference survives, cut twice at random: the records' oracle outputs concatenated are
    the oracle's output of the staged copy, and (programs that print no '\\n' of their own) record i's output ends just past
    output newline R_i"""
    rng = random.Random(4242 if engine == "nft" else 2424)
    oracles, progs = {}, {}
    n_cases = n_ranked = n_nul = 0
    for pat, name, data, eng, exp in golden_lib.cases():
        if eng != engine or exp is None:
            continue
        if pat not in oracles:
            oracles[pat] = Oracle(pat, engine)
            try:
                progs[pat] = prints_newline(trre_amd.Program(pat, engine))
            except trre_amd.TrreError:
                progs[pat] = None
        o = oracles[pat]
        for _ in range(2):
            off = random_offsets(rng, data)
            recs = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
            staged = staged_copy(data, off)
            try:
                # (the deterministic engine's tables grow with what it has seen: a fresh oracle per input, as a fresh
                # process of the reference)
                outs = [(Oracle(pat, engine) if engine == "dft" else o).scan(r) for r in recs]
                whole = (Oracle(pat, engine) if engine == "dft" else o).scan(staged)
            except OracleError:
                continue                         # a record on which the reference does not survive
            assert b"".join(outs) == whole, (pat, name, off)
            n_cases += 1
            n_nul += b"\0" in data
            if progs[pat] is False:
                nl = [i for i, c in enumerate(whole) if c == 10]
                end = 0
                for i, r in enumerate(recs):
                    end += len(outs[i])
                    k = staged[:off[i + 1]].count(b"\n")
                    assert end == (nl[k - 1] + 1 if k else 0), (pat, name, off, i)
                n_ranked += 1
    assert n_cases > 700 and n_ranked > 600 and n_nul > 10, (n_cases, n_ranked, n_nul)


def test_framing_of_a_record_without_newline_oracle():
    """printf 'abc' | trre 'c:X' prints "ab\\n", as "ab\\n" does; several lines; empty; a NUL cuts its line"""
    for engine in ("nft", "dft"):
        o = Oracle("c:X", engine)
        assert o.scan(b"abc") == b"ab\n" == o.scan(b"ab\n")
        assert o.scan(b"cc\nacb") == b"XX\naX\n"
        assert o.scan(b"") == b""
        assert o.scan(b"ac\0c\nc") == b"aX\n\n"


@pytest.mark.skipif(not ref_available(), reason="the compiled reference binaries are not built here")
def test_framing_of_a_record_without_newline_reference():
    rng = random.Random(17)
    for pat in ("c:X", "[a:A-z:Z]", "(cat:dog|dog:cat)", "a:xyz"):
        for engine in ("nft", "dft"):
            o = Oracle(pat, engine)
            assert ref_scan(pat, engine, b"abc") == o.scan(b"abc")
            for _ in range(5):
                rec = bytes(rng.choice(b"abcdot\n\0") for _ in range(rng.randrange(1, 30)))
                assert ref_scan(pat, engine, rec) == o.scan(rec), (pat, engine, rec)
    assert ref_scan("c:X", "nft", b"abc") == b"ab\n"


def test_library_exports_records_symbol():
    assert hasattr(api.lib(), "trre_scan_device_records")
    with open(os.path.join(ROOT, "include", "trre_mi355x.h")) as f:
        assert "int trre_scan_device_records(" in f.read()


def test_modes_other_than_scan_are_refused():
    for mode in ("match", "scan_all", "match_all"):
        p = trre_amd.Program("a:b", "nft", mode=mode)
        assert records_rc(p) == api.E_UNSUPPORTED, mode


def test_newline_printing_programs_are_refused():
    for pat in (b"x:\n", b":\n", b"(a:\n)*", b"[a:\t-c:\x0b]", b"[\x01:\x02-\x7f:\x80]"):
        for engine in ("nft", "dft"):
            p = trre_amd.Program(pat, engine)
            assert records_rc(p) == api.E_UNSUPPORTED, (pat, engine)
            assert "newline" in api.lib().trre_last_error().decode()


def test_copies_and_the_dictionary_are_taken():
    import dictgen
    keys, vals = dictgen.make_dictionary(1000)
    pats = [".", "[a-z]", "[a:A-z:Z]", "a:xyz", "[aie]:", "(cat:dog|dog:cat)", "\n", "(\n)*x:y", "\n:x", "(.:x)*.*", "[a:b-y:zz:a]"]
    for pat in pats:
        for engine in ("nft", "dft"):
            assert not prints_newline(trre_amd.Program(pat, engine)), (pat, engine)
    assert not prints_newline(trre_amd.Program(dictgen.pattern(keys, vals), "dft"))


def test_overlaps_are_refused():
    p = trre_amd.Program("[a:A-z:Z]", "dft")
    ob = (NREC + 1) * 8
    cases = [dict(d_ooff=OFF + ob - 1),                  # the offsets overlap each other
             dict(d_ooff=OFF),
             dict(d_off=IN + N - 1),                     # ... the input
             dict(d_off=OUT + CAP - 8),                  # ... the output
             dict(d_ooff=IN - ob + 1),
             dict(d_ooff=OUT + 100),
             dict(d_out=IN + 1),                         # input and output overlap other than in place
             dict(d_in=None)]                            # a null pointer
    for kw in cases:
        kw.setdefault("d_ooff", OOFF)
        assert records_rc(p, **kw) == api.E_ARG, kw
