"""The child of tests/test_gpu_window.py: the cases of tests/window_cases.py through the positional-window kernel on the GPU in ONE environment (the
switches are read once per process).  Every job runs with TRRE_TRACE=1 and reads the trace of its own scans back (runtime.cpp: route_window,
finish_inner) —
    trre: window kernel: N lane(s) of B bytes, pair|narrow|wide entries
    trre: window kernel: M lane(s) redone, status 0x..
    python tests/gpu_window_check.py <job>
The last line of stdout is `RESULT <repr of a dict>`: "programs" (the tags of the programs that ran, in order), "cases" (the names of the cases
every program ran, in order), "redo" (per (program, case): the lanes the device redid, input aligned), "scans" (how many device scans were
compared), "control" (the programs whose control ran), "bad" (what was wrong; empty: nothing) and "seconds" (wall time of building the cases and
the oracle / the device scans / the whole job).

Per program and case, four placements — aligned; input and output 5 and 15 bytes off 16-byte alignment, the case built again for that offset
(the edges are placed in the offsets the kernel sees); in place (the output view is the input view) — and for each:
    bytes   the oracle's, byte for byte; a mismatch names the first differing offset and the placed edges within 64 bytes of it
    slack   the output view, exactly as long as the input, lies inside a tensor filled with 0xA5: the 256 bytes before and behind it are unchanged
            (the kernel stores whole 16-byte blocks and 128-byte rows)
    route   ONE window line in the trace, with the lane count, the lane size and the entry form the job expects, and ONE redo line whose count
            is the number of lanes window_cases.expected_redo() derives — also for the cases with a NUL, whose window launch is void (which
            family answers then is not asserted: the bytes and the trace are)
Once per program, the control: the main case with the input 3 bytes off alignment and the output aligned (no 16-byte stores possible): the
oracle's bytes and NO window line.  A test that could not tell the routes apart would pass for the wrong reason."""
import collections
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE):
    sys.path.insert(0, d)

import window_cases as W  # noqa: E402
from gpu_generate_check import Stderr  # noqa: E402  (file descriptor 2 into a file for the length of a scan)
from oracle_lib import Oracle  # noqa: E402

WINDOW = re.compile(r"^trre: window kernel: (\d+) lane\(s\) of (\d+) bytes, (\w+) entries$", re.M)
REDONE = re.compile(r"^trre: window kernel: (\d+) lane\(s\) redone, status 0x([0-9a-f]+)$", re.M)
SENTINEL, SLACK = 0xA5, 256
ALL = [p.tag for p in W.PROGRAMS]
PAIR = [p.tag for p in W.PROGRAMS if p.form == "pair"]
PLACEMENTS = [("aligned", 0, False), ("off_5", 5, False), ("off_15", 15, False), ("in_place", 0, True)]
# job -> (the environment on top of test_gpu_window.BASE_ENV, the lane size, the programs, the entry form the trace must name: None = the program's own)
JOBS = collections.OrderedDict([
    ("lanes2048", ({}, 2048, ALL, None)),
    ("lanes128", ({"TRRE_LANE_BYTES": "128"}, 128, ALL, None)),
    ("lanes16k", ({"TRRE_LANE_BYTES": "16384"}, 16384, W.BIG_PROGRAMS, None)),
    ("single", ({"TRRE_NO_LPW_PAIR": "1"}, 2048, PAIR, "narrow")),
])


def differs(got, want, c):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    near = [e.name for e in c.edges if abs(e.off - (k + c.a)) <= 64]
    return "%d bytes, the oracle %d, first difference at byte %d of the output = offset %d of lane %d; placed edges within 64 bytes: %r" % (
        len(got), len(want), k, (k + c.a) % c.B, (k + c.a) // c.B, near)


def on_device(p, c, out_mis, in_place):
    """one scan of the case: the input c.a bytes off alignment, the output view out_mis bytes off, exactly len(data) long, 0xA5 around it:
    (bytes, the slack is untouched, the trace)"""
    import torch
    n = len(c.data)
    data = torch.frombuffer(bytearray(c.data), dtype=torch.uint8).cuda()
    obase = torch.full((n + 2 * SLACK + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ooff = SLACK + (out_mis - (obase.data_ptr() + SLACK)) % 16
    out = obase[ooff:ooff + n]
    if in_place:
        out.copy_(data)
        src = out
    else:
        ibase = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        ioff = (c.a - ibase.data_ptr()) % 16
        src = ibase[ioff:ioff + n]
        src.copy_(data)
    assert src.data_ptr() % 16 == c.a and out.data_ptr() % 16 == out_mis
    torch.cuda.synchronize()
    with Stderr() as err:
        got = p.scan_tensor(src, out=out)
        torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    clean = bool((obase[ooff - SLACK:ooff] == SENTINEL).all()) and bool((obase[ooff + n:ooff + n + SLACK] == SENTINEL).all())
    return got.cpu().numpy().tobytes(), clean, err.text


def main(job):
    import trre_amd
    t_job, t_prep, t_scan = time.time(), 0.0, 0.0
    env, B, tags, form = JOBS[job]
    assert os.environ.get("TRRE_TRACE") and all(os.environ.get(k) == v for k, v in env.items()), "run me through tests/test_gpu_window.py"
    bad, redo, control, scans = [], {}, [], 0
    for tag in tags:
        w = W.program(tag)
        p = trre_amd.Program(w.pat, w.eng)
        oracle = Oracle(w.pat, w.eng)
        expect_form = form or w.form
        for where, a, in_place in PLACEMENTS:
            t0 = time.time()
            cases = W.cases(B, a, w.key)
            wants = [oracle.scan(c.data) for c in cases]
            t_prep += time.time() - t0
            assert [c.name for c in cases] == W.NAMES
            for c, want in zip(cases, wants):
                t0 = time.time()
                got, clean, trace = on_device(p, c, a, in_place)
                t_scan += time.time() - t0
                scans += 1
                what = "%s %s %s" % (tag, c.name, where)
                if got != want:
                    bad.append("%s: %s" % (what, differs(got, want, c)))
                if not clean:
                    bad.append("%s: written within 256 bytes of the output view" % what)
                lines, done = WINDOW.findall(trace), REDONE.findall(trace)
                lanes = (c.a + len(c.data) + B - 1) // B
                if lines != [(str(lanes), str(B), expect_form)]:
                    bad.append("%s: window lines %r, expected one of %d lanes of %d bytes, %s entries" % (what, lines, lanes, B, expect_form))
                if [int(m) for m, _ in done] != [len(c.redo)]:
                    bad.append("%s: redo lines %r, expected one of %d lanes" % (what, done, len(c.redo)))
                if where == "aligned":
                    redo[tag, c.name] = int(done[0][0]) if done else -1
                if len(bad) > 40:
                    break
        # the control: not congruent mod 16, so not the window kernel
        t0 = time.time()
        c = W.cases(B, 3, w.key)[0]
        want = oracle.scan(c.data)
        got, clean, trace = on_device(p, c, 0, False)
        t_scan += time.time() - t0
        if got != want or not clean:
            bad.append("%s control: %s%s" % (tag, differs(got, want, c), "" if clean else "; written outside the output view"))
        if WINDOW.findall(trace) or REDONE.findall(trace):
            bad.append("%s control: a window line in the trace of a scan whose buffers are not congruent mod 16" % tag)
        control.append(tag)
        print("%s: %s entries, delay %d: %d scans so far, %d complaint(s)" % (tag, expect_form, w.delay, scans, len(bad)), file=sys.stderr)
    print("RESULT " + repr({"programs": list(tags), "cases": list(W.NAMES), "redo": redo, "scans": scans, "control": control, "bad": bad[:12],
                             "seconds": tuple(round(t, 2) for t in (t_prep, t_scan, time.time() - t_job))}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
