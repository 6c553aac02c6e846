"""The child of tests/test_gpu_exact_repair.py: the cases of tests/repair_cases.py on the GPU in ONE environment (the switches are read once per
process).  Every job runs with TRRE_TRACE=1 and reads the trace of its own scans back: finish() says one line per repair round of the exact
sub-ranges (runtime.cpp: exact_repair, exact_repair_backward) —
    trre: exact sub-ranges: round N, M lane(s) to repair
    trre: exact sub-ranges, backward pass: round N, M lane(s) to repair
    python tests/gpu_repair_check.py <job>
The last line of stdout is `RESULT <repr of a dict>`: "cases" (the names of the cases that ran, in order), "rounds" (per case (forward rounds,
backward rounds, lanes flagged in each forward round)), "extras" (what ran once per job, in order), "column" (the trace of the column calls),
"bad" (what was wrong; empty: nothing) and "seconds" (wall time of the oracle / the cases' scans / the extras / the whole job).

Per case: a device buffer is scanned once (a capacity that holds the oracle's output: no second call, no second trace) and compared with the
oracle byte for byte — a mismatch names the first differing offset of the output, the input bytes it comes from and their lanes —, and the case's
expectation (repair_cases.Case.expect) is checked on the trace; a case whose rounds the input alone decides (Case.single) runs exactly
repair_cases.forward_rounds() of them.  The parent compares those with the host shim's.

Once per job, on `long_run_aa_nft` and `backward_runs_star_nft`: input and output 5 and 3 bytes off 16-byte alignment; the host path
(Program.scan); the C ABI at a capacity of exactly the oracle's size and of one byte less, a sentinel-filled MiB behind it (the sizes are final
only after the repair: the emit pass that meets the capacity is the second one); in place (`aa:x` prints less than it reads; the first emit pass
has to leave before it writes a byte); twice in a row on one Program.  And one column call, which runs the same scan: the spans of `aa` in three
strings against re.finditer, their pieces against re.split."""
import collections
import ctypes
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE):
    sys.path.insert(0, d)

import repair_cases as R  # noqa: E402
from gpu_generate_check import Stderr  # noqa: E402  (file descriptor 2 into a file for the length of a scan)
from oracle_lib import Oracle  # noqa: E402

FORWARD = re.compile(r"^trre: exact sub-ranges: round (\d+), (\d+) lane\(s\) to repair$", re.M)
BACKWARD = re.compile(r"^trre: exact sub-ranges, backward pass: round (\d+), (\d+) lane\(s\) to repair$", re.M)
SENTINEL, PAD = 0xA5, 1 << 20
ALL = [c.name for c in R.cases(128)]
EXTRAS = ["long_run_aa_nft", "backward_runs_star_nft"]
EXTRA_CHECKS = ["misaligned", "host", "capacity", "capacity_less_1", "in_place", "twice"]
# job -> (the environment on top of test_gpu_exact_repair.BASE_ENV, the lane size the inputs are built for, its cases, what is said of the trace:
#         "expect": every case's expectation; "quiet": no repair line at all; "print": nothing, it is printed)
JOBS = collections.OrderedDict([
    ("lanes2048", ({}, 2048, ALL, "expect")),
    ("lanes128", ({"TRRE_LANE_BYTES": "128"}, 128, ALL, "expect")),
    ("old_way", ({"TRRE_EXACT": "0"}, 2048, [n for n in ALL if n.startswith(("long_run_", "backward_runs_"))], "quiet")),
    ("one_walk", ({"TRRE_ONE": "1"}, 2048, [n for n in ALL if n.startswith(("long_run_", "many_runs_", "backward_runs_"))], "print")),
])


def chunks_of(n, L):
    """workgroups of 256 lanes over n bytes: the runtime gives up after n_chunks + 64 repair rounds and scans the buffer the old way"""
    return (n + 256 * L - 1) // (256 * L)


def input_place(c, want, k):
    """where in the INPUT byte k of the oracle's output comes from (lanes own input bytes): (first, last) input offsets it can come from.  A line
    of the input is a line of the output, so k names its line; inside the line the greedy patterns' output grows with the input read
    (repair_cases.greedy on prefixes of the line names the byte), the others are narrowed to their line, a few lanes at the most"""
    s = 0
    for _ in range(want.count(b"\n", 0, k)):
        s = c.data.index(b"\n", s) + 1
    e = c.data.find(b"\n", s)
    e = len(c.data) if e < 0 else e
    if c.pat not in R.GREEDY:
        return s, e
    d = k - (want.rfind(b"\n", 0, k) + 1)                 # bytes of this line's output in front of byte k
    lo, hi = 0, e - s + 1                                 # the shortest prefix of the line whose output is longer than d
    while lo < hi:
        mid = (lo + hi) // 2
        if len(R.greedy(c.pat, c.data[s:s + mid] + b"\n")) - 1 > d:
            hi = mid
        else:
            lo = mid + 1
    return max(s, s + lo - 3), min(e, s + lo)


def differs(got, want, c, L):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    a, b = input_place(c, want, min(k, max(len(want) - 1, 0)))
    return "%d bytes, the oracle %d, first difference at byte %d of the output: input bytes %d .. %d, lanes %d .. %d of %d bytes" % (
        len(got), len(want), k, a, b, a // L, b // L, L)


def to_dev(data, mis=0, room=0):
    """`data` on the device, `mis` bytes off 16-byte alignment, `room` more bytes behind it: (the view of the data, the whole buffer, its offset)"""
    import torch
    base = torch.full((len(data) + room + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    off = (mis - base.data_ptr()) % 16
    base[off:off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return base[off:off + len(data)], base, off


def scan_once(p, src, need, mis=0):
    """one trre_scan_device call into a sentinel-filled buffer: (bytes, nothing written outside the view)"""
    import torch
    obase = torch.full((need + 64 + 160,), SENTINEL, dtype=torch.uint8, device="cuda")
    ooff = 16 + (mis - obase.data_ptr()) % 16
    got = p.scan_tensor(src, out=obase[ooff:ooff + need + 64]).cpu().numpy().tobytes()
    clean = bool((obase[:ooff] == SENTINEL).all()) and bool((obase[ooff + need + 64:] == SENTINEL).all())
    return got, clean


def abi_call(p, src, need, cap):
    """trre_scan_device at `cap`, a sentinel-filled MiB behind it: (rc, out_len, the first min(cap, need) bytes, the MiB is untouched)"""
    import torch
    from trre_amd import api
    buf = torch.full((cap + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    m = ctypes.c_size_t()
    rc = api.lib().trre_scan_device(p._h, src.data_ptr(), src.numel(), buf.data_ptr(), cap, ctypes.byref(m), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, m.value, buf[:min(cap, need)].cpu().numpy().tobytes(), bool((buf[cap:] == SENTINEL).all())


def extras(p, c, want, L, bad):
    """what runs once per job on a case whose scan repairs (see the module's docstring); returns the names of the checks, in order"""
    import torch
    from trre_amd import api
    need = len(want)
    src, _, _ = to_dev(c.data, 5)
    assert src.data_ptr() % 16 == 5
    got, clean = scan_once(p, src, need, 3)
    if got != want or not clean:
        bad.append("%s misaligned: %s%s" % (c.name, differs(got, want, c, L), "" if clean else "; written outside the output view"))
    got = p.scan(c.data)
    if got != want:
        bad.append("%s host path: %s" % (c.name, differs(got, want, c, L)))
    src, _, _ = to_dev(c.data)
    rc, m, got, clean = abi_call(p, src, need, need)
    if rc != 0 or m != need or got != want or not clean:
        bad.append("%s cap = need: rc %d, out_len %d, need %d, bytes equal %s, behind the capacity untouched %s" % (c.name, rc, m, need, got == want, clean))
    rc, m, _, clean = abi_call(p, src, need, need - 1)
    if rc != api.E_CAPACITY or m != need or not clean:
        bad.append("%s cap = need - 1: rc %d, out_len %d, need %d, behind the capacity untouched %s" % (c.name, rc, m, need, clean))
    # in place, as tests/test_gpu_inplace.py words the contract: the output view starts where the input starts
    n, cap = len(c.data), max(len(c.data), need) + 64
    t = torch.full((cap + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    t[:n] = torch.frombuffer(bytearray(c.data), dtype=torch.uint8).cuda()
    got = p.scan_tensor(t[:n], out=t[:cap]).cpu().numpy().tobytes()
    if got != want or not bool((t[cap:] == SENTINEL).all()):
        bad.append("%s in place: %s" % (c.name, differs(got, want, c, L)))
    for k in (1, 2):
        got, clean = scan_once(p, src, need)
        if got != want or not clean:
            bad.append("%s call %d of two in a row: %s" % (c.name, k, differs(got, want, c, L)))
    return list(EXTRA_CHECKS)


def column(L, bad):
    """span_list and split_list of `aa` over three strings, the first a run over three lanes from an odd offset: (forward, backward) trace lines"""
    import trre_amd
    recs = [b"b" + b"a" * (3 * L + 1), b"aa", b""]
    p = trre_amd.Program("aa", "nft", "spans")
    with Stderr() as err:
        spans = p.span_list(recs)
        pieces = p.split_list(recs)
    if spans != [[m.span() for m in re.finditer(b"aa", r)] for r in recs]:
        bad.append("column: span_list differs from re.finditer: %r" % ([s[:3] for s in spans],))
    if pieces != [re.split(b"aa", r) for r in recs]:
        bad.append("column: split_list differs from re.split: %r" % ([s[:3] for s in pieces],))
    return len(FORWARD.findall(err.text)), len(BACKWARD.findall(err.text)), trre_amd.KERNEL_NAMES[p.info.kernel]


def main(job):
    import trre_amd
    t_job, t_oracle, t_scan, t_extra = time.time(), 0.0, 0.0, 0.0
    fam = {v: k for k, v in trre_amd.KERNEL_NAMES.items()}
    env, L, names, trace = JOBS[job]
    assert os.environ.get("TRRE_TRACE") and all(os.environ.get(k) == v for k, v in env.items()), "run me through tests/test_gpu_exact_repair.py"
    cases = R.by_name(L)
    bad, ran, rounds, did, progs, wants = [], [], [], [], {}, {}
    for name in names:
        c = cases[name]
        t0 = time.time()
        if (c.pat, c.eng, c.data) not in wants:
            wants[c.pat, c.eng, c.data] = Oracle(c.pat, c.eng).scan(c.data)
        t_oracle += time.time() - t0
        want = wants[c.pat, c.eng, c.data]
        if (c.pat, c.eng, c.family) not in progs:
            progs[c.pat, c.eng, c.family] = trre_amd.Program(c.pat, c.eng)
            if c.family:
                progs[c.pat, c.eng, c.family].set_kernel(fam[c.family])
        p = progs[c.pat, c.eng, c.family]
        t0 = time.time()
        src, _, _ = to_dev(c.data)
        with Stderr() as err:
            got, clean = scan_once(p, src, len(want))
        t_scan += time.time() - t0
        fwd = [int(m) for _, m in FORWARD.findall(err.text)]
        bwd = [int(m) for _, m in BACKWARD.findall(err.text)]
        print("%s: %s, n=%d, %d bytes out, forward rounds %d %r, backward rounds %d %r" %
              (name, trre_amd.KERNEL_NAMES[p.info.kernel], len(c.data), len(want), len(fwd), fwd[:8], len(bwd), bwd[:8]), file=sys.stderr)
        if got != want:
            bad.append("%s: %s" % (name, differs(got, want, c, L)))
        if not clean:
            bad.append("%s: written outside the output view" % name)
        if trace == "quiet" and (fwd or bwd):
            bad.append("%s: %d + %d repair rounds with TRRE_EXACT=0" % (name, len(fwd), len(bwd)))
        if trace == "expect" and c.expect:
            if c.expect[0] == "none" and (fwd or bwd):
                bad.append("%s: %d + %d repair rounds, expected none" % (name, len(fwd), len(bwd)))
            if c.expect[0] == "forward" and len(fwd) < c.expect[1]:
                bad.append("%s: %d forward repair rounds, expected at least %d" % (name, len(fwd), c.expect[1]))
            if c.expect[0] == "backward" and len(bwd) != 1:
                bad.append("%s: %d backward repair rounds, one settles every run" % (name, len(bwd)))
            if c.single and (len(fwd) != R.forward_rounds(c.data, L) or any(m != 1 for m in fwd)):
                bad.append("%s: forward rounds %r, the input decides on %d of one lane each" % (name, fwd, R.forward_rounds(c.data, L)))
            # (many runs, several flagged lanes to a workgroup: the number of rounds depends on the order of the threads, but it cannot pass the
            # longest run's lanes that can guess wrong — repair_cases.max_flagged_lanes() says why —, which is under the runtime's n_chunks + 64)
            bound = min(chunks_of(len(c.data), L) + 64, R.max_flagged_lanes(c.data, L))
            if name.startswith("many_runs_") and not 1 <= len(fwd) <= bound:
                bad.append("%s: %d forward rounds, not within 1 .. %d" % (name, len(fwd), bound))
        ran.append(name)
        rounds.append((len(fwd), len(bwd), fwd[:8]))
        if name in EXTRAS:
            t0 = time.time()
            did.append((name, extras(p, c, want, L, bad)))
            t_extra += time.time() - t0
    with_column = column(L, bad)
    print("column calls (%s): %d forward, %d backward repair rounds in the trace" % (with_column[2], with_column[0], with_column[1]), file=sys.stderr)
    print("RESULT " + repr({"cases": ran, "rounds": rounds, "extras": did, "column": with_column, "bad": bad[:12],
                             "seconds": tuple(round(t, 2) for t in (t_oracle, t_scan, t_extra, time.time() - t_job))}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
