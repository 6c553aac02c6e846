"""The column calls back to back on one program and one context (include/trre_mi355x.h: trre_scan_device_records, _strings,
trre_match_device_strings, trre_find_device_strings, trre_span_device_strings).  Their host passes share the context's buffers,
which only grow and which every pass carves anew: a small input after a large one runs in the large one's room, a large one
after a small one makes them grow in mid-call.  Each program goes through one sequence of sizes — 3 bytes; about 330 KiB in
strings of mixed length, more than five record tiles (64 KiB) and twenty string tiles (16 KiB); 3 bytes again; no string at all;
the large input again; a staged text (n + nrec bytes) of exactly one string tile; of one string tile and a byte — and every result
is the oracle's, computed as the files of the single calls compute it (test_gpu_records.py, test_gpu_strings.py,
test_gpu_match_strings.py, find_lib, span_lib).  The second large result is also the first."""
import random

import pytest

import span_lib
import trre_amd
from find_lib import Finder
from oracle_lib import Oracle
from span_lib import Spanner

pytestmark = pytest.mark.gpu

STR_TILE = 16384
REC_TILE = 65536
LARGE = 330 * 1024


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(data):
    import torch
    return torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8)[:len(data)].to(dev())


def off_dev(off):
    import torch
    return torch.tensor(list(off), dtype=torch.int64, device=dev())


def pack(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off


def sequence(seed, tiny, word):
    """the inputs, each a list of strings; word(rng, k): a string of k bytes"""
    rng = random.Random(seed)
    large, total = [], 0
    while total < LARGE:
        large.append(word(rng, rng.choice((0, 0, 1, 2, 5, 17, 40, 100, 300, 2000))))
        total += len(large[-1])
    assert b"" in large and total + len(large) > 20 * STR_TILE and total > 5 * REC_TILE
    tile = [word(rng, STR_TILE // 16 - 1) for _ in range(16)]
    more = tile[:15] + [word(rng, STR_TILE // 16)]
    assert len(tiny) == 3 and sum(map(len, tile)) + 16 == STR_TILE and sum(map(len, more)) + 16 == STR_TILE + 1
    return [("tiny", [tiny]), ("large", large), ("tiny again", [tiny]), ("none", []), ("large again", large), ("one tile", tile),
            ("one tile and a byte", more)]


def run_sequence(seq, calls):
    """calls: name -> (run(values, offsets) -> result, want(recs) -> result); every input through every call in turn, the
    expectations computed once per distinct input"""
    wants, large = {}, {}
    for label, recs in seq:
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
        return res[0].cpu().numpy().tobytes(), res[1].cpu().numpy().tolist()

    calls = {
        "scan_tensor": (lambda v, offs: p.scan_tensor(v).cpu().numpy().tobytes(), lambda recs: o.scan(b"".join(recs))),
        "scan_records": (lambda v, offs: pair(p.scan_records(v, offs)), lambda recs: pack([o.scan(r) for r in recs])),
        "scan_strings": (lambda v, offs: pair(p.scan_strings(v, offs)), lambda recs: pack([o.scan(r + b"\n")[:-1] for r in recs])),
    }
    run_sequence(sequence(81, b"cab", word), calls)


def test_match_strings():
    pat = "(a:xyz|b)*"
    p, o = trre_amd.Program(pat, "nft", "match"), Oracle(pat, "nft")

    def word(rng, k):
        alphabet = b"ab" if rng.random() < 0.7 else b"aabbc"
        return bytes(rng.choice(alphabet) for _ in range(k))

    def run(v, offs):
        out, oo, valid = p.match_strings(v, offs)
        return out.cpu().numpy().tobytes(), oo.cpu().numpy().tolist(), valid.cpu().numpy().tolist()

    def want(recs):
        per = [o.match(r + b"\n") for r in recs]
        data, off = pack([m[:-1] for m in per])
        return data, off, [m != b"" for m in per]

    seq = sequence(82, b"aba", word)
    verdicts = want(seq[1][1])[2]
    assert 0 < sum(verdicts) < len(verdicts)
    run_sequence(seq, {"match_strings": (run, want)})


def test_find_strings():
    pat = "[0-9]+:N|(cat:dog)"
    p, finder = trre_amd.Program(pat, "nft", "find"), Finder(pat)

    def word(rng, k):
        return b"".join(rng.choice((b"cat", b"7", b"12", b" ", b"x", b"ca", b"dog")) for _ in range(k))[:k]

    def run(v, offs):
        return tuple(t.cpu().numpy().tolist() for t in p.find_strings(v, offs))

    def want(recs):
        per = finder.lines(recs)
        data, moff = pack([o for w in per for o in w])
        return list(data), moff, pack([b"." * len(w) for w in per])[1]

    run_sequence(sequence(83, b"cat", word), {"find_strings": (run, want)})


def test_count_and_span_strings():
    """count_strings and span_strings by turns"""
    pat = "(cat|dog)"
    p, spanner = trre_amd.Program(pat, "nft", "spans"), Spanner(pat)

    def word(rng, k):
        return b"".join(rng.choice((b"cat", b"dog", b" ", b"x", b"ca", b"do")) for _ in range(k))[:k]

    def spans(v, offs):
        return tuple(t.cpu().numpy().tolist() for t in p.span_strings(v, offs))

    def want_spans(recs):
        return span_lib.expect(spanner.lines(recs), pack(recs)[1])

    def want_counts(recs):
        return [len(w) for w in spanner.lines(recs)]

    run_sequence(sequence(84, b"cat", word), {"count_strings": (lambda v, offs: p.count_strings(v, offs).cpu().numpy().tolist(), want_counts),
                                              "span_strings": (spans, want_spans)})
