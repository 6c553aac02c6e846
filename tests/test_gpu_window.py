"""The positional-window kernel (k_stream_lpw) on the GPU at lane, piece and wave edges that are PLACED (tests/window_cases.py),
against the oracle — and the trace says that the window kernel ran, on which form of its entries, and how many lanes it handed to the redo pass.

Before this file the window walk ran on a device only over random text (word soup, the fuzz, the 8 GiB runs): the edges were hit by chance, no
test told the window route from the direct walkers (a misaligned output silently takes another route), none counted the redone lanes (a kernel
that hands EVERY lane to the redo pass prints correct bytes), none looked at the bytes around the output although the kernel stores whole
16-byte blocks and 128-byte rows.  What runs here and nowhere on the host shim (tests/test_window_cases.py): the steady unconditional stores,
the wait counters, the direct-to-LDS loads, the swizzle against real LDS — and lanes of 16 KiB, what an 8 GiB headline uses.

GPU tier: one test per job, each ONE child (tests/gpu_window_check.py <job>; the switches are read once per process) under a time limit of its
own, its environment stripped of inherited TRRE_*; after a child that did not exit 0 nothing more is started on the GPU by this file.
    job          environment (on TRRE_TRACE=1)    what
    lanes2048                                     every case, every program (sixteen: narrow entries of delays 1 - 3 with and without the pair
                                                  form, wide ones of delays 4 - 7, both engines), lanes of 2 048 bytes (inputs of 1.2 MiB)
    lanes128     TRRE_LANE_BYTES=128              the same at lanes of 128 bytes (a workgroup is 32 KiB: 75 KiB cross two workgroup edges)
    lanes16k     TRRE_LANE_BYTES=16384            one narrow (pair) and one wide program at lanes of 16 KiB: 9.4 MiB, one workgroup edge crossed
    single       TRRE_NO_LPW_PAIR=1               the programs that have the pair form on their single (narrow) entries, at 2 048
Per case, program and placement (aligned, 5 and 15 bytes off, in place) the child compares the bytes, the 256 bytes on either side of the
output view and the two trace lines; see its docstring.  The redo counts it read from the device must be the host shim's for the same input
(lanes of 128 and 2 048; the shim has no 16 KiB geometry: there the count derived by hand in window_cases.expected_redo() stands alone)."""
import os
import subprocess
import sys
import time

import pytest

import gpu_window_check as G                   # (its tables; nothing in it touches a GPU before a job runs)
import window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_window_check.py")
BASE_ENV = {"TRRE_TRACE": "1"}
# job -> (seconds measured on an MI355X, process start to exit; the child's time limit)
TIMES = {"lanes2048": (4.5, 120), "lanes128": (3.6, 120), "lanes16k": (3.7, 120), "single": (3.3, 120)}
_failed = []

# ---- the documented programs and cases, written out (the child builds its tables from window_cases) ------------------------------------------------
_TAGS = ["swap2", "catdog", "zoo", "ther", "there", "abcdef", "abcdefg", "abcdefgh"]
_ALL = [t + "_" + e for t in _TAGS for e in ("nft", "dft")]
PROGRAMS = {"lanes2048": _ALL, "lanes128": _ALL, "lanes16k": ["catdog_nft", "abcdefg_nft"],
            "single": [t + "_" + e for t in ("swap2", "catdog", "ther") for e in ("nft", "dft")]}
CASES = ["main", "vend_0", "vend_1", "vend_16", "vend_63", "vend_64", "vend_65", "vend_191", "vend_192", "vend_193",
         "final_1", "final_64", "final_193", "final_long", "nul_lane_end", "nul_lane_start", "nul_skipped_head", "nul_last_piece"]


def shim_redo(tag, name, B, single=False):
    """the lanes the host shim redid for a case at the device's geometry (geo 0: lanes of 2 048 bytes; geo 2: of 128), input aligned"""
    import shim_lib
    import trre_amd
    w = W.program(tag)
    c = next(c for c in W.cases(B, 0, w.key) if c.name == name)
    fam = shim_lib.STREAM_LPW_PAIR if w.form == "pair" and not single else 8
    shim_lib.scan_like_runtime(trre_amd.Program(w.pat, w.eng), c.data, geo={2048: 0, 128: 2}[B], family=fam)
    return len(shim_lib.last_redo()), len(c.redo)


@pytest.mark.gpu
@pytest.mark.parametrize("job", list(G.JOBS))
def test_placed_edges_through_the_window_kernel_and_the_trace_says_so(job):
    assert not _failed, "the child of %r did not exit 0: nothing more is started" % _failed[0]
    env, B, tags, form = G.JOBS[job]
    e = {k: v for k, v in os.environ.items() if not k.startswith("TRRE_")}
    e.update(BASE_ENV)
    e.update(env)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(TIMES[job][1]), sys.executable, CHILD, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    wall = time.time() - t0
    err = r.stderr.decode("latin-1")
    print("\n".join(line for line in err.splitlines() if not line.startswith("trre: window kernel"))[-20000:])
    if r.returncode != 0:
        _failed.append(job)
    assert r.returncode == 0, "%s: exit status %d\n%s" % (job, r.returncode, err[-3000:])
    res = eval(r.stdout.decode().strip().splitlines()[-1][len("RESULT "):])
    print("%s: %d scans; seconds (cases and oracle, scans, the job) %r, the child from start to exit %.1f" % (job, res["scans"], res["seconds"], wall))
    assert res["bad"] == [], res["bad"]
    assert res["programs"] == PROGRAMS[job] == tags and res["cases"] == CASES and res["control"] == tags
    assert res["scans"] == len(tags) * len(CASES) * len(G.PLACEMENTS) and set(res["redo"]) == {(t, n) for t in tags for n in CASES}
    # every window line named the expected form and lane size (the child's complaint otherwise); the redo counts are the shim's
    if B in (128, 2048):
        for (tag, name), count in res["redo"].items():
            assert (count, count) == shim_redo(tag, name, B, job == "single"), (tag, name, count)
    # (lane 0 and the last lanes, always; of the 601 lanes of the main case those three and no more)
    assert all(count >= 2 for count in res["redo"].values()) and all(res["redo"][t, "main"] == 3 for t in tags), res["redo"]


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------

def test_the_jobs_are_the_documented_ones():
    """the child's job table and this file name the same programs and cases; every environment is a set of TRRE_* switches"""
    assert list(G.JOBS) == list(TIMES) == ["lanes2048", "lanes128", "lanes16k", "single"] and set(PROGRAMS) == set(TIMES)
    for job, (env, B, tags, form) in G.JOBS.items():
        assert tags == PROGRAMS[job], job
        assert all(k.startswith("TRRE_") for k in env) and not set(env) & set(BASE_ENV)
    assert [p.tag for p in W.PROGRAMS] == _ALL and W.NAMES == CASES
    assert [(G.JOBS[j][0], G.JOBS[j][1], G.JOBS[j][3]) for j in G.JOBS] == [
        ({}, 2048, None), ({"TRRE_LANE_BYTES": "128"}, 128, None), ({"TRRE_LANE_BYTES": "16384"}, 16384, None), ({"TRRE_NO_LPW_PAIR": "1"}, 2048, "narrow")]
    assert PROGRAMS["single"] == [p.tag for p in W.PROGRAMS if p.form == "pair"]
    assert [W.program(t).form for t in PROGRAMS["lanes16k"]] == ["pair", "wide"]
    assert [w for w, a, ip in G.PLACEMENTS] == ["aligned", "off_5", "off_15", "in_place"] and [a for w, a, ip in G.PLACEMENTS] == [0, 5, 15, 0]
    assert all(limit >= 120 and limit >= 10 * seconds for seconds, limit in TIMES.values())
