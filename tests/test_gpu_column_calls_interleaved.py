"""The column calls back to back on one program and one context (include/trre_mi355x.h: trre_scan_device_records, _strings,
trre_match_device_strings, trre_find_device_strings, trre_span_device_strings).  Their host passes share the context's buffers,
which only grow and which every pass carves anew: a small input after a large one runs in the large one's room, a large one
after a small one makes them grow in mid-call.  Each program goes through one sequence of sizes — 3 bytes; about 330 KiB in
strings of mixed length, more than five record tiles (64 KiB) and twenty string tiles (16 KiB); 3 bytes again; no string at all;
the large input again; a staged text (n + nrec bytes) of exactly one string tile; of one string tile and a byte — and every result
is the oracle's, computed as the files of the single calls compute it: by their own expect() (test_gpu_records.py,
test_gpu_strings.py, test_gpu_match_strings.py, test_gpu_find_strings.py) and span_lib's.  The second large result is also the
first; the sequence is gpu_column_lib's."""
import pytest

import span_lib
import trre_amd
from find_lib import Finder
from gpu_column_lib import blob, lst, off_dev, pack, sequence, to_dev
from oracle_lib import Oracle
from span_lib import Spanner
from test_gpu_find_strings import expect as expect_find
from test_gpu_match_strings import Memo
from test_gpu_match_strings import expect as expect_match
from test_gpu_records import expect as expect_records
from test_gpu_strings import expect as expect_strings

pytestmark = pytest.mark.gpu


def run_sequence(seq, calls):
    """calls: name -> (run(values, offsets) -> result, want(recs) -> result); every input through every call in turn, the
    expectations computed once per distinct input"""
    wants, large = {}, {}
    for label, recs in seq.items():
        data, off = pack(recs)
        values, offsets = to_dev(data), off_dev(off)
        for name, (run, want) in calls.items():
            key = (name, label.replace(" again", ""))
            if key not in wants:
                wants[key] = want(recs)
            got = run(values, offsets)
            assert got == wants[key], (name, label)
            if label.startswith("large"):
                assert large.setdefault(name, got) == got, (name, label)


def test_scan_tensor_records_and_strings():
    """a program whose output is longer than its input (a:xyz): the framed text has more tiles than the staged one"""
    pat = "a:xyz"
    p, o = trre_amd.Program(pat, "nft"), Oracle(pat, "nft")

    def word(rng, k):
        return bytes(rng.choice(b"aaabcxyz  \n\0") for _ in range(k))

    def pair(res):
        return blob(res[0]), lst(res[1])

    calls = {
        "scan_tensor": (lambda v, offs: blob(p.scan_tensor(v)), lambda recs: o.scan(b"".join(recs))),
        "scan_records": (lambda v, offs: pair(p.scan_records(v, offs)), lambda recs: expect_records(o, recs)),
        "scan_strings": (lambda v, offs: pair(p.scan_strings(v, offs)), lambda recs: expect_strings(o, recs)),
    }
    run_sequence(sequence(81, b"cab", word), calls)


def test_match_strings():
    pat = "(a:xyz|b)*"
    p, memo = trre_amd.Program(pat, "nft", "match"), Memo(pat)

    def word(rng, k):
        alphabet = b"ab" if rng.random() < 0.7 else b"aabbc"
        return bytes(rng.choice(alphabet) for _ in range(k))

    def run(v, offs):
        out, oo, valid = p.match_strings(v, offs)
        return blob(out), lst(oo), lst(valid)

    def want(recs):
        return expect_match(memo, recs)

    seq = sequence(82, b"aba", word)
    verdicts = want(seq["large"])[2]
    assert 0 < sum(verdicts) < len(verdicts)
    run_sequence(seq, {"match_strings": (run, want)})


def test_find_strings():
    pat = "[0-9]+:N|(cat:dog)"
    p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)

    def word(rng, k):
        return b"".join(rng.choice((b"cat", b"7", b"12", b" ", b"x", b"ca", b"dog")) for _ in range(k))[:k]

    def run(v, offs):
        out, mo, lo = p.find_strings(v, offs)
        return blob(out), lst(mo), lst(lo)

    def want(recs):
        return expect_find(finder, recs)

    run_sequence(sequence(83, b"cat", word), {"find_strings": (run, want)})


def test_count_and_span_strings():
    """count_strings and span_strings by turns"""
    pat = "(cat|dog)"
    p, spanner = trre_amd.Program(pat, "nft", "spans"), Spanner(pat)

    def word(rng, k):
        return b"".join(rng.choice((b"cat", b"dog", b" ", b"x", b"ca", b"do")) for _ in range(k))[:k]

    def spans(v, offs):
        return tuple(lst(t) for t in p.span_strings(v, offs))

    def want_spans(recs):
        return span_lib.expect(spanner.lines(recs), pack(recs)[1])

    def want_counts(recs):
        return [len(w) for w in spanner.lines(recs)]

    run_sequence(sequence(84, b"cat", word), {"count_strings": (lambda v, offs: lst(p.count_strings(v, offs)), want_counts),
                                              "span_strings": (spans, want_spans)})
