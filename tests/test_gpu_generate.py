"""Generator modes (`-a`, `-ma`) on the GPU at lane, workgroup, chunk and hand-over edges — and WHO enumerated.

The host enumeration (generate.cpp) is the fallback of k_gen and its checker: a k_gen that flagged an overflow on every launch, or went wrong only
where it also happened to flag one, would print the right bytes everywhere.  So every case here says who enumerates each of its chunks, and the
GPU tests read generate_on()'s trace (TRRE_TRACE=1: one line per chunk, `device` or `host (why)`): outside the designated `host` chunks the host
enumeration answers nothing.  The expected bytes are the oracle's, always (tests/gpu_generate_check.py says how).

GPU tier: one test per job, each ONE child (tests/gpu_generate_check.py <job>; the switches are read once per process) under a time limit of its
own; after a child that did not exit 0 nothing more is started on the GPU by this file.
    job           cases                                                                                                        environment
    lanes         five patterns x nine lengths x (final '\\n' | final letter); a '\\n' around lane and workgroup starts; records     TRRE_TRACE=1
                  longer than two lanes / a workgroup; only '\\n'; NULs; misaligned device tensors; an output buffer that grows
    limits        a line one short of / at the depth of a lane's stack, of the size of its path buffer                           TRRE_TRACE=1
    chunks        the cut at 16 MiB: a '\\n' on byte 16 Mi - 1, a record over it, no '\\n' behind it; device, host, device chunks     TRRE_TRACE=1
                  in one call; an epsilon cycle in chunk two (TRRE_E_DIVERGES and its `partial`)
    checker       the lanes inputs of a workgroup and more, and the first chunks case: the same bytes, every chunk `host`        + TRRE_GEN_HOST=1
Wall times of the children on an MI355X (measured once, process start to exit) and the limits — ten times that, not below 120 s — are in TIMES.

CPU tier (no marker): the expectations are pinned on something other than the code under test.  The lane body on the host shim at the runtime's
geometry (shim_lib.generate_on_device_like_runtime(p, data, 0): 512-byte lanes, 512 frames, 2 KiB of path) returns the oracle's bytes for every
lanes and limits input and for every block of the chunks inputs, and hands over to the host exactly where the tables say `host` (whether a record
overflows depends on the record, not on where it lies: the blocks' answers hold for the repeated buffer).  The two edges of `limits` are found on
the shim, never written down: edge stays, edge + 1 is handed over."""
import os
import subprocess
import sys

import pytest

import gpu_generate_check as G                 # (its tables; nothing in it touches a GPU before a job runs)
import shim_lib
import trre_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_generate_check.py")
# job -> (seconds measured on an MI355X, the child's time limit)
TIMES = {"lanes": (7.8, 120), "limits": (2.6, 120), "chunks": (3.1, 120), "checker": (4.4, 120)}
_failed = []

# ---- the documented cases, written out from the axes of the issue (the child builds its tables from its own) ------------------------------
_KEYS = ["shallow", "astar", "insert", "lines", "digits"]
_LENGTHS = [1, 2, 511, 512, 513, 131071, 131072, 131073, 262657]
_NL_AT = [511, 512, 513, 130559, 130560, 130561, 131071, 131072, 131073, 131583, 131584, 131585]
_NULS = ["lane_last", "lane_first", "record_first", "two", "last_line"]
_BIG = {"%s_%d_%s" % (k, n, e) for k in _KEYS for n in (131073, 262657) for e in ("nl", "q1", "tensor")}
DOCUMENTED = {
    "lanes": ["%s_%d_%s" % (k, n, e) for k in _KEYS for n in _LENGTHS for e in ("nl", "q1")]
    + ["%s_nl_at_%d" % (k, pos) for k in ("shallow", "lines") for pos in _NL_AT]
    + ["shallow_record_1400", "shallow_record_140000", "shallow_only_newlines", "insert_only_newlines", "lines_only_newlines"]
    + ["%s_nul_%s" % (k, w) for k in ("shallow", "lines") for w in _NULS]
    + ["%s_%d_tensor" % (k, n) for k in _KEYS for n in (131073, 262657)]
    + ["grow_small", "grow_large", "grow_small_again"],
    "limits": ["stack_edge", "stack_edge_plus_1", "path_edge", "path_edge_plus_1"],
    "chunks": ["c1_newline_at_the_cut", "c2_record_over_the_cut", "c3_no_newline_after_the_cut", "c4_host_chunk_between_device_chunks",
               "c5_diverges_in_chunk_two"],
}
DOCUMENTED["checker"] = [n for n in DOCUMENTED["lanes"] if n in _BIG or "_nl_at_" in n or n.endswith(("_record_140000", "_only_newlines"))] + ["c1_newline_at_the_cut"]


def expected_chunks(c, data=None):
    """[(offset, bytes, who)] of a case: the cut as DESIGN.md words it (G.cuts), the lengths the issue names written out, who from the table"""
    where = G.cuts(data if data is not None else G.input_of(c))
    assert len(where) == len(c.who), (c.name, where)
    if c.name in G.CHUNK_BYTES:
        assert [n for _, n in where] == G.CHUNK_BYTES[c.name], (c.name, where)
    return [(off, n, who) for (off, n), who in zip(where, c.who)]


@pytest.mark.gpu
@pytest.mark.parametrize("job", list(G.JOBS))
def test_who_enumerated_and_the_oracles_bytes(job):
    assert not _failed, "the child of %r did not exit 0: nothing more is started" % _failed[0]
    env, cases = G.JOBS[job]
    e = {k: v for k, v in os.environ.items() if not k.startswith("TRRE_")}
    e.update({"TRRE_TRACE": "1"})
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", str(TIMES[job][1]), sys.executable, CHILD, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    err = r.stderr.decode("latin-1")
    print(err[-20000:])
    if r.returncode != 0:
        _failed.append(job)
    assert r.returncode == 0, "%s: exit status %d\n%s" % (job, r.returncode, err[-3000:])
    res = eval(r.stdout.decode().strip().splitlines()[-1][len("RESULT "):])
    print("%s: %d cases, scans %.1f s, the child %.1f s" % ((job, len(res["cases"])) + tuple(res["seconds"])))
    assert res["bad"] == [], res["bad"]
    assert res["cases"] == DOCUMENTED[job] == [c.name for c in cases]
    why = "TRRE_GEN_HOST" if job == "checker" else "status 0x"
    for c, seen in zip(cases, res["chunks"]):
        assert [t[:3] for t in seen] == expected_chunks(c), (c.name, seen)
        assert all((t[3] or "").startswith(why) == (t[2] == "host") for t in seen), (c.name, seen)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------

def test_the_jobs_are_the_documented_ones():
    assert list(G.JOBS) == list(DOCUMENTED) == list(TIMES)
    for job, (env, cases) in G.JOBS.items():
        assert [c.name for c in cases] == DOCUMENTED[job], job
        assert all(k.startswith("TRRE_") for k in env)
        assert all(limit >= 120 and limit >= 10 * seconds for seconds, limit in TIMES.values())
    assert (G.LANE, G.WG, G.CHUNK, list(G.LENGTHS), list(G.NL_AT)) == (512, 131072, 16 << 20, _LENGTHS, _NL_AT)
    assert [G.PATTERNS[k] for k in _KEYS] == [("(cat:dog|cat:cow|ca:C)", "scan_all"), ("a*", "scan_all"), (":=", "scan_all"), ("[a-z ]*|.*", "match_all"),
                                              ("[0-9]+", "match_all")]
    # the checker: every lanes input of a workgroup and a byte, and more — host everywhere, the same parts otherwise
    by_name = {c.name: c for c in G.LANES + [G.C1]}
    for c in G.CHECKER:
        assert c == by_name[c.name]._replace(who=("host",) * len(c.who)) and len(G.input_of(c)) >= G.WG + 1
    assert all(len(G.input_of(c)) <= G.WG for c in G.LANES if c.name not in DOCUMENTED["checker"])


def test_the_inputs_are_what_their_names_say():
    lanes = {c.name: G.input_of(c) for c in G.LANES}
    for k in _KEYS:
        for n in _LENGTHS:
            assert len(lanes["%s_%d_nl" % (k, n)]) == len(lanes["%s_%d_q1" % (k, n)]) == n
            assert lanes["%s_%d_nl" % (k, n)][-1:] == b"\n" and lanes["%s_%d_q1" % (k, n)][-1:] == b"x"
    assert max(len(line) for line in lanes["lines_262657_nl"].split(b"\n")) <= 400
    assert not any(0x30 <= b <= 0x39 for b in lanes["digits_262657_nl"])
    assert all(G.oracle_of("[0-9]+", "match_all", lanes["digits_%d_%s" % (n, e)]) == (b"", False) for n in _LENGTHS for e in ("nl", "q1"))    # a total of 0
    for pos in _NL_AT:
        d = lanes["shallow_nl_at_%d" % pos]
        assert d[pos] == 0x0A and b"\n" not in d[pos - 2:pos] + d[pos + 1:pos + 3] and len(d) > 257 * 512
    # the long records: lanes 5 and 6 inside one record; workgroup 1 (bytes 131072 .. 262143) inside one record
    for name, first, last in (("shallow_record_1400", 5 * 512, 7 * 512 - 1), ("shallow_record_140000", 131072, 262143)):
        d = lanes[name]
        assert b"\n" not in d[first - 1:last + 1] and d.count(b"\n") > 20, name
    assert lanes["shallow_only_newlines"] == b"\n" * 131073
    at = 3 * 512
    nul = {w: lanes["shallow_nul_%s" % w] for w in _NULS}
    assert nul["lane_last"][at - 1] == 0 and nul["lane_first"][at] == 0 and nul["record_first"][at - 1:at + 1] == b"\n\0"
    assert all(b"\n" not in nul[w][at - 8:at + 8] for w in ("lane_last", "lane_first", "two")) and nul["two"][at - 8:at + 8].count(0) == 2
    assert [nul[w].count(0) for w in _NULS] == [1, 1, 1, 2, 1]
    assert nul["last_line"][-1:] != b"\n" and 0 in nul["last_line"][nul["last_line"].rindex(b"\n"):]
    # limits: three workgroups, the special line starts at byte 200 of a lane of the middle one
    for c in G.LIMITS:
        d, start = G.input_of(c), G.WG + G.WG // 2 + 200
        line = d[start:d.index(b"\n", start)]
        assert d[start - 1] == 0x0A and start % 512 == 200 and len(set(line)) == 1 and 3 * G.WG <= len(d) < 3 * G.WG + 4096
        assert len(line) == G.edge(c.parts[1][0][2]) + c.parts[1][0][3]


def test_the_chunk_cases_cut_where_they_say():
    """the inputs of the chunks jobs against the sentences of the issue (the bytes around 16 Mi), and their chunks"""
    M = 16 << 20
    c1, c2, c3 = (G.input_of(c) for c in G.CHUNKS_A)
    assert c1[M - 1] == 0x0A and len(c1) == M + 300 * 1024
    assert b"\n" not in c2[M - 300:M + 700] and c2[M - 301] == 0x0A and c2[M + 700] == 0x0A
    assert b"\n" not in c3[M - 500:] and c3[M - 501] == 0x0A and len(c3) == M + 500
    for c, d in zip(G.CHUNKS_A, (c1, c2, c3)):
        assert [n for _, n, _ in expected_chunks(c, d)] == G.CHUNK_BYTES[c.name]
    c4, c5 = G.CHUNKS_B
    d = G.input_of(c4)
    (o1, n1, _), (o2, n2, _), (o3, n3, _) = expected_chunks(c4, d)
    assert n1 == M and d[o2:o2 + 601] == b"q" * 600 + b"\n" and n2 >= M and n3 > 0 and 33 << 20 <= len(d) < 34 << 20
    assert d.count(b"q" * 600) == 1
    d = G.input_of(c5)
    (_, n1, _), (o2, _, _) = expected_chunks(c5, d)
    assert n1 == M and d.index(b"Q") > o2 and d.count(b"Q") == 1


def _on_the_shim(pat, mode, data):
    """(the lane body's bytes — the host enumeration's where it hands over —, went to the host, diverged)"""
    p = trre_amd.Program(pat, "nft", mode=mode)
    assert p.info.kernel == trre_amd.api.KERNEL_GENERATE
    try:
        out, host = shim_lib.generate_on_device_like_runtime(p, data, 0)
        return out, host, False
    except trre_amd.TrreError as e:
        assert e.code == trre_amd.api.E_DIVERGES
        return e.partial, True, True


@pytest.mark.parametrize("job", ["lanes", "limits"])
def test_the_lane_body_on_the_shim_answers_what_the_tables_say(job):
    seen = {}
    for c in G.JOBS[job][1]:
        data = G.input_of(c)
        assert len(data) <= 1 << 20                        # (the oracle on the whole input)
        if (c.pat, c.mode, data) not in seen:
            want, diverges = G.want_of(c, data)
            got, host, div = _on_the_shim(c.pat, c.mode, data)
            assert got == want and div == diverges, c.name
            seen[c.pat, c.mode, data] = host
        assert [("host" if seen[c.pat, c.mode, data] else "device")] == list(c.who), c.name
    assert len(seen) >= (100 if job == "lanes" else 4)


def test_the_two_hand_over_edges_are_edges():
    for which, (pat, mode, byte) in G.EDGES.items():
        k = G.edge(which)
        print("%s: %r %s: a line of %d stays, of %d is handed over" % (which, pat, mode, k, k + 1))
        o = G.Oracle(pat, "nft", all_outputs=True)
        for n, host in ((k, False), (k + 1, True)):
            data = b"the cat\n" + byte * n + b"\nthe dog\n"
            got, went, _ = _on_the_shim(pat, mode, data)
            assert went == host and got == o.match(data), (which, n)
    # a lane's stack has 512 frames and a line of n letters under [a-z]* needs n + 1; its path buffer has 2 KiB, eight bytes per 'a'
    assert 256 <= G.edge("stack") < 1024 and 128 <= G.edge("path") < 512


def test_the_blocks_of_the_chunk_cases_on_the_shim():
    """every block of the chunks inputs alone: the oracle's bytes, and who answers it; a chunk is the host's when one of its blocks is"""
    for c in G.CHUNKS_A + G.CHUNKS_B:
        host_at, off = [], 0
        for spec, rep in c.parts:
            b = G.block(spec)
            want, diverges = G.oracle_of(c.pat, c.mode, b)
            got, host, div = _on_the_shim(c.pat, c.mode, b)
            assert got == want and div == diverges, (c.name, spec)
            if host:
                host_at += [off + i * len(b) for i in range(rep)]
            off += rep * len(b)
        who = ["host" if any(o <= h < o + n for h in host_at) else "device" for o, n, _ in expected_chunks(c)]
        assert who == list(c.who), c.name
    # the cycle needs its byte: the oracle dies on that line, with what it had printed — and prints chunk one's blocks without complaint
    assert G.oracle_of(G.CYCLE, "scan_all", G.block(("cycle",)))[1] and not G.oracle_of(G.CYCLE, "scan_all", G.block(G.B1))[1]
