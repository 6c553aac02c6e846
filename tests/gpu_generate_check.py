"""The child of tests/test_gpu_generate.py: generator modes (`-a`, `-ma`) on the GPU at lane, workgroup, chunk and hand-over edges.  One
environment per process (the switches are read once); every job runs with TRRE_TRACE=1 and reads the trace of its own scans back: one line per
chunk of generate_on() (runtime.cpp) says who enumerated it, the device (k_gen) or the host (generate.cpp, the fallback AND the checker).
    python tests/gpu_generate_check.py <job>
The last line of stdout is `RESULT <repr of a dict>`: "cases" (the names of the cases that ran, in order), "chunks" (per case the trace's chunks,
each (offset, bytes, "device" | "host", the reason in the brackets or None)), "bad" (what was wrong; empty: nothing) and "seconds" (wall time of
the scans / of the whole job).

A case: (name, pattern, mode, parts, who enumerates each chunk, route).  Route "scan": host buffers, the entry behind Program.scan (trre_scan_host) —
called ONCE, at a capacity that holds the oracle's output, because Program.scan's second call after TRRE_E_CAPACITY would trace its chunks a second
time; "tensor": Program.scan_tensor on views 3 (input) and 5 (output) bytes off 16-byte alignment.  `parts` is ((block, repeats), ..): the input is the blocks one after the
other, every block but the last ending in '\\n'.  The expected bytes are ALWAYS the oracle's — Oracle(pat, "nft", all_outputs=True) — never the
library's, never TRRE_GEN_HOST's: of the whole input up to 1 MiB; beyond, of every block, repeated (a line's output depends on that line alone).
A block is a tuple that block() turns into bytes: the tables are module-level, importing this module builds no input and touches no GPU.

The geometry (runtime.cpp): a lane owns the records that start in its LANE = 512 bytes, a workgroup is 256 lanes (WG = 128 KiB), a host buffer
goes up in chunks of CHUNK = 16 MiB cut behind the first '\\n' at or after byte CHUNK - 1 of what is left."""
import collections
import functools
import os
import random
import re
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE):
    sys.path.insert(0, d)

import corpus  # noqa: E402
from oracle_lib import Oracle, OracleError  # noqa: E402

LANE, WG, CHUNK = 512, 256 * 512, 16 << 20
KIB, MIB = 1 << 10, 1 << 20
SHALLOW, LINES, GROW, STACK, PATH, CYCLE = "(cat:dog|cat:cow|ca:C)", "[a-z ]*|.*", "(a|a:x)*", "[a-z]*", "(a:xxxxxxxx)*", "cat:dog|Q:*"
PATTERNS = collections.OrderedDict([("shallow", (SHALLOW, "scan_all")), ("astar", ("a*", "scan_all")), ("insert", (":=", "scan_all")),
                                    ("lines", (LINES, "match_all")), ("digits", ("[0-9]+", "match_all"))])
LENGTHS = (1, 2, 511, 512, 513, WG - 1, WG, WG + 1, 2 * WG + 513)
NL_AT = tuple(LANE * k + d for k in (1, 255, 256, 257) for d in (-1, 0, 1))
NULS = ("lane_last", "lane_first", "record_first", "two", "last_line")
TRACE = re.compile(r"^trre: generate: chunk at (\d+), (\d+) bytes: (device|host)(?: \((.*)\))?$", re.M)

Case = collections.namedtuple("Case", "name pat mode parts who route")


def case(name, key_or_pat, parts, who=("device",), route="scan", mode=None):
    pat, m = PATTERNS[key_or_pat] if key_or_pat in PATTERNS else (key_or_pat, mode)
    return Case(name, pat, m, tuple(parts), tuple(who), route)


# ---- the blocks -------------------------------------------------------------------------------------------------------------------------

_streams = {}


def _soup(seed, n):
    """the first n bytes of the seed's word soup (a longer request of one seed begins with the shorter one's bytes)"""
    if len(_streams.get(seed, b"")) < n:
        _streams[seed] = corpus.word_soup(random.Random(seed), max(n + 256, 2 * len(_streams.get(seed, b""))), max_len=60)
    return bytearray(_streams[seed][:n])


def _flat(seed, n):
    """n bytes of word soup without a '\\n'"""
    return bytes(_soup(seed, n)).replace(b"\n", b" ")


@functools.lru_cache(maxsize=256)
def block(spec):
    kind = spec[0]
    if kind == "soup":                       # (seed, n, "nl" | "q1"): exactly n bytes of word soup; the last byte a '\n' / a letter (Q1: it ends its record)
        d = _soup(spec[1], spec[2])
        d[-1] = 0x0A if spec[3] == "nl" else ord("x")
        return bytes(d)
    if kind == "nl_at":                      # (pos): WG + 2 lanes of soup with a '\n' at `pos`, none within two bytes of it: a record starts at pos + 1
        d = _soup(29, 258 * LANE + 100)
        for i in range(spec[1] - 2, spec[1] + 3):
            if d[i] == 0x0A:
                d[i] = ord("y")
        d[spec[1]] = 0x0A
        d[-1] = 0x0A
        return bytes(d)
    if kind == "flat":                       # (seed, n): ONE record of n bytes and its '\n'
        return _flat(spec[1], spec[2]) + b"\n"
    if kind == "tail":                       # (seed, n): n bytes without a '\n' (the end of a buffer)
        return _flat(spec[1], spec[2])
    if kind == "newlines":
        return b"\n" * spec[1]
    if kind == "nul":
        d = _soup(31, 8 * LANE)
        d[-1] = 0x0A
        at = 3 * LANE
        for i in range(at - 8, at + 8):      # (one line around the lane edge: the NUL cuts a record that goes on behind it)
            if d[i] in (0x0A, 0x20):
                d[i] = ord("c")
        if spec[1] == "lane_last":
            d[at - 1] = 0
        elif spec[1] == "lane_first":
            d[at] = 0
        elif spec[1] == "record_first":      # a record that starts at a lane start with a NUL: empty, the rest of the line is nobody's
            d[at - 1], d[at] = 0x0A, 0
        elif spec[1] == "two":
            d[at - 5], d[at + 5] = 0, 0
        elif spec[1] == "last_line":         # ... in a last line without a newline
            tail = bytes(d).rindex(b"\n", 0, len(d) - 1) + 1
            d[-1] = ord("t")
            d[(tail + len(d)) // 2] = 0
            assert tail < (tail + len(d)) // 2 < len(d) - 1
        return bytes(d)
    if kind == "run":                        # (byte, "stack" | "path", 0 | 1): a line of the shim's edge (+ 1) times that byte
        return spec[1] * (edge(spec[2]) + spec[3]) + b"\n"
    if kind == "letters":                    # (n): a line of n letters
        return b"q" * spec[1] + b"\n"
    if kind == "aaa":                        # twenty lines of twelve 'a'
        return b"aaaaaaaaaaaa\n" * 20
    if kind == "cycle":                      # soup, a line with the byte that CYCLE's epsilon cycle needs, soup
        return block(("soup", 37, 100 * KIB, "nl")) + b"the cat had a Q and a cat\n" + block(("soup", 38, 50 * KIB, "nl"))
    raise KeyError(spec)


# ---- the two hand-over edges, found on the host shim at the runtime's geometry (never a constant) -----------------------------------------
EDGES = {"stack": (STACK, "match_all", b"q"), "path": (PATH, "match_all", b"a")}


def went_to_the_host(pat, mode, data):
    import shim_lib
    import trre_amd
    return shim_lib.generate_on_device_like_runtime(trre_amd.Program(pat, "nft", mode=mode), data, 0)[1]


@functools.lru_cache(maxsize=None)
def edge(which):
    """the longest line of one byte the lane body (gen_lane at 512 frames, 2 KiB of path) still answers itself: one more goes to the host"""
    pat, mode, byte = EDGES[which]
    lo, hi = 1, 4096                         # (lo: stays; hi: handed over)
    assert not went_to_the_host(pat, mode, b"ab\n" + byte * lo + b"\ncd\n") and went_to_the_host(pat, mode, b"ab\n" + byte * hi + b"\ncd\n")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if went_to_the_host(pat, mode, b"ab\n" + byte * mid + b"\ncd\n"):
            hi = mid
        else:
            lo = mid
    return lo


# ---- the tables -------------------------------------------------------------------------------------------------------------------------

def _lanes():
    out = []
    for key in PATTERNS:
        for n in LENGTHS:
            for end in ("nl", "q1"):
                out.append(case("%s_%d_%s" % (key, n, end), key, [(("soup", 23, n, end), 1)]))
    for key in ("shallow", "lines"):
        out += [case("%s_nl_at_%d" % (key, pos), key, [(("nl_at", pos), 1)]) for pos in NL_AT]
    # one long record between short lines: 1 400 bytes from byte 300 of lane 4 (lanes 5 and 6 own no record start); 140 000 bytes from 4 000 bytes
    # before workgroup 1 to behind its end (all its 256 lanes count zero)
    out.append(case("shallow_record_1400", "shallow", [(("soup", 23, 4 * LANE + 300, "nl"), 1), (("flat", 24, 1400), 1), (("soup", 25, 2000, "nl"), 1)]))
    out.append(case("shallow_record_140000", "shallow", [(("soup", 23, WG - 4000, "nl"), 1), (("flat", 24, 140000), 1), (("soup", 25, 2000, "nl"), 1)]))
    out += [case("%s_only_newlines" % key, key, [(("newlines", WG + 1), 1)]) for key in ("shallow", "insert", "lines")]
    out += [case("%s_nul_%s" % (key, which), key, [(("nul", which), 1)]) for key in ("shallow", "lines") for which in NULS]
    for key in PATTERNS:
        for n in (WG + 1, 2 * WG + 513):
            out.append(case("%s_%d_tensor" % (key, n), key, [(("soup", 23, n, "q1"), 1)], route="tensor"))
    # d_gen_out grows and is kept: three calls on ONE program (main() keeps a program per pattern and mode)
    small = (("soup", 27, 64 * KIB, "nl"), 1)
    out.append(case("grow_small", GROW, [small], mode="scan_all"))
    out.append(case("grow_large", GROW, [(("soup", 27, 32 * KIB, "nl"), 1), (("aaa",), 1), (("soup", 28, 32 * KIB, "nl"), 1)], mode="scan_all"))
    out.append(case("grow_small_again", GROW, [small], mode="scan_all"))
    return out


def _limits():
    # three workgroups of soup, the special line from byte 200 of a lane in the middle one
    def around(line):
        return [(("soup", 23, WG + WG // 2 + 200, "nl"), 1), (line, 1), (("soup", 25, WG + WG // 2 - 200, "nl"), 1)]
    return [case("stack_edge", STACK, around(("run", b"q", "stack", 0)), ["device"], mode="match_all"),
            case("stack_edge_plus_1", STACK, around(("run", b"q", "stack", 1)), ["host"], mode="match_all"),
            case("path_edge", PATH, around(("run", b"a", "path", 0)), ["device"], mode="match_all"),
            case("path_edge_plus_1", PATH, around(("run", b"a", "path", 1)), ["host"], mode="match_all")]


B1 = ("soup", 23, MIB, "nl")                 # 1 MiB of soup, its last byte a '\n': sixteen of them put a '\n' at byte 16 Mi - 1
B256 = ("soup", 23, 256 * KIB, "nl")
C1 = case("c1_newline_at_the_cut", "shallow", [(B1, 16), (("soup", 25, 300 * KIB, "nl"), 1)], ["device", "device"])
CHUNKS_A = [
    C1,
    # byte 16 Mi - 1 inside a record of 1 000 bytes whose '\n' is byte 16 Mi + 700
    case("c2_record_over_the_cut", "shallow", [(B1, 15), (("soup", 24, MIB - 300, "nl"), 1), (("flat", 24, 1000), 1), (("soup", 25, 300 * KIB, "nl"), 1)],
         ["device", "device"]),
    # no '\n' at or after byte 16 Mi - 1: a tail of 1 000 bytes from 16 Mi - 500
    case("c3_no_newline_after_the_cut", "shallow", [(B1, 15), (("soup", 24, MIB - 500, "nl"), 1), (("tail", 24, 1000), 1)], ["device"]),
]
CHUNKS_B = [
    # three chunks, the middle one with ONE line of 600 letters (deeper than a lane's stack): device output, host output, device output
    case("c4_host_chunk_between_device_chunks", "lines", [(B256, 64), (("letters", 600), 1), (B256, 68)], ["device", "host", "device"]),
    # an epsilon cycle in the second of two chunks: TRRE_E_DIVERGES, and what was printed before it stays
    case("c5_diverges_in_chunk_two", CYCLE, [(B1, 16), (("cycle",), 1)], ["device", "host"], mode="scan_all"),
]
# the lengths of the chunks, where they are the point (the others: cuts() of the input)
CHUNK_BYTES = {"c1_newline_at_the_cut": [16 * MIB, 300 * KIB], "c2_record_over_the_cut": [16 * MIB + 701, 300 * KIB],
               "c3_no_newline_after_the_cut": [16 * MIB + 500]}


def size_of(spec):
    """len(block(spec)) without building it, for the kinds that are large"""
    return {"soup": lambda: spec[2], "nl_at": lambda: 258 * LANE + 100, "flat": lambda: spec[2] + 1, "tail": lambda: spec[2],
            "newlines": lambda: spec[1], "nul": lambda: 8 * LANE}.get(spec[0], lambda: len(block(spec)))()


LANES, LIMITS = _lanes(), _limits()
# TRRE_GEN_HOST=1: the lanes inputs of WG + 1 bytes and more and C1 — the same bytes, and every chunk says `host`
CHECKER = [c._replace(who=("host",) * len(c.who)) for c in LANES + [C1] if sum(size_of(s) * r for s, r in c.parts) >= WG + 1]
# job -> (the environment on top of TRRE_TRACE=1, its cases)
JOBS = collections.OrderedDict([("lanes", ({}, LANES)), ("limits", ({}, LIMITS)), ("chunks", ({}, CHUNKS_A + CHUNKS_B)),
                                ("checker", ({"TRRE_GEN_HOST": "1"}, CHECKER))])


# ---- inputs and expectations ------------------------------------------------------------------------------------------------------------

def input_of(c):
    return b"".join(block(spec) * rep for spec, rep in c.parts)


def cuts(data):
    """the chunks of a host buffer as DESIGN.md 4.6 words them: [(offset, bytes)]"""
    out, off = [], 0
    while off < len(data):
        n = len(data) - off
        if n > CHUNK:
            nl = data.find(b"\n", off + CHUNK - 1)
            n = nl + 1 - off if nl >= 0 else n
        out.append((off, n))
        off += n
    return out


_oracles, _wants = {}, {}


def oracle_of(pat, mode, data):
    """(what the reference prints, it diverged): on a divergence what it had printed when it gave up"""
    if (pat, mode) not in _oracles:
        _oracles[pat, mode] = Oracle(pat, "nft", all_outputs=True)
    o = _oracles[pat, mode]
    try:
        return (o.match(data) if mode == "match_all" else o.scan(data)), False
    except OracleError as e:
        return e.partial, True


def want_of(c, data):
    if len(data) <= MIB:
        return oracle_of(c.pat, c.mode, data)
    out = []
    for spec, rep in c.parts:
        key = (c.pat, c.mode, spec)
        if key not in _wants:
            _wants[key] = oracle_of(c.pat, c.mode, block(spec))
        w, div = _wants[key]
        if div:
            return b"".join(out) + w, True                         # (nothing is printed behind it)
        out.append(w * rep)
    return b"".join(out), False


# ---- the run ----------------------------------------------------------------------------------------------------------------------------

class Stderr:
    """file descriptor 2 into a temporary file for the length of a scan: what the library traced there, read back (and passed on)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("latin-1")
        self.tmp.close()
        sys.stderr.write(self.text)
        return False


def through_host_buffers(p, data, cap):
    """ONE trre_scan_host call at a capacity that holds the oracle's output (Program.scan would call twice, and trace twice): (rc, bytes)"""
    import ctypes
    import numpy as np
    from trre_amd import api
    out = np.empty(cap, dtype=np.uint8)
    m = ctypes.c_size_t()
    rc = api.lib().trre_scan_host(p._h, data, len(data), out.ctypes.data_as(ctypes.c_char_p), cap, ctypes.byref(m), 0)
    return rc, out[:min(m.value, cap)].tobytes()


def through_tensors(p, data, need):
    """trre_scan_device with the input 3 bytes and the output 5 bytes off 16-byte alignment: (bytes, the sentinels around the view are intact)"""
    import torch
    ibase = torch.empty(len(data) + 32, dtype=torch.uint8, device="cuda")
    ioff = (3 - ibase.data_ptr()) % 16
    inp = ibase[ioff:ioff + len(data)]
    inp.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    obase = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    ooff = (5 - obase.data_ptr()) % 16
    out = obase[ooff:ooff + need + 16]
    assert inp.data_ptr() % 16 == 3 and out.data_ptr() % 16 == 5
    got = p.scan_tensor(inp, out=out).cpu().numpy().tobytes()
    return got, bool((obase[ooff + need:] == 0xA5).all()) and bool((obase[:ooff] == 0xA5).all())


def main(job):
    import trre_amd
    t_job = time.time()
    t_scan = 0.0
    env, cases = JOBS[job]
    assert os.environ.get("TRRE_TRACE") and all(os.environ.get(k) == v for k, v in env.items()), "run me through tests/test_gpu_generate.py"
    bad, names, chunks, progs = [], [], [], {}
    for c in cases:
        data = input_of(c)
        want, diverges = want_of(c, data)
        if (c.pat, c.mode) not in progs:
            progs[c.pat, c.mode] = trre_amd.Program(c.pat, "nft", mode=c.mode)
            if progs[c.pat, c.mode].info.kernel != trre_amd.api.KERNEL_GENERATE:
                bad.append("%s: not the generator family" % c.name)
        p = progs[c.pat, c.mode]
        t0 = time.time()
        code, clean = 0, True
        with Stderr() as err:
            if c.route == "tensor":
                got, clean = through_tensors(p, data, len(want))
            else:
                code, got = through_host_buffers(p, data, len(want) + 64)
        dt = time.time() - t0
        t_scan += dt
        seen = [(int(a), int(b), who, why) for a, b, who, why in TRACE.findall(err.text)]
        print("%s: n=%d, %d bytes out, %.2f s, %s" % (c.name, len(data), len(want), dt, [(b, who) for _, b, who, _ in seen]), file=sys.stderr)
        if code != (trre_amd.api.E_DIVERGES if diverges else 0):
            bad.append("%s: error code %d, the reference %s" % (c.name, code, "diverges" if diverges else "does not fail"))
        elif got != want:
            k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            bad.append("%s: %d bytes, the oracle %d, first difference at %d" % (c.name, len(got), len(want), k))
        if not clean:
            bad.append("%s: written outside the output view" % c.name)
        names.append(c.name)
        chunks.append(seen)
    print("RESULT " + repr({"cases": names, "chunks": chunks, "bad": bad[:12], "seconds": (round(t_scan, 2), round(time.time() - t_job, 2))}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
