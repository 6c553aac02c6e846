"""The repair of the exact sub-ranges on the GPU: wrong state guesses made with ordinary patterns and ordinary bytes
(tests/repair_cases.py), against the oracle — and the trace says that the repair really ran.

Before this file the only thing that reached the repair code on a device was a NUL inside a long line (tests/test_gpu_round5.py, test_gpu_round6.py):
the SKIP shortcut, which passes lanes without walking them.  Here exact_repair(), exact_repair_backward() and exact_emit_again() (runtime.cpp),
the walking branch of the repair loop of k_stream_g16, k_rev_repair with rev_repair_lane on packed 4-bit symbols and on byte symbols, the early
returns of the forward passes on status[2] and status[3] and the capacity predicate of an emit pass that runs a second time all run, with 256
threads to a workgroup: what the host shim, which runs a launch's lanes one after the other, cannot show.

GPU tier: one test per job, each ONE child (tests/gpu_repair_check.py <job>; the switches are read once per process) under a time limit of its
own, its environment stripped of inherited TRRE_*; after a child that did not exit 0 nothing more is started on the GPU by this file.
    job          environment (on TRRE_TRACE=1 TRRE_MAPGEN=0)    what
    lanes2048                                                   every case at lanes of 2 048 bytes (inputs up to 1.6 MiB): bytes, the expectation on the trace
    lanes128     TRRE_LANE_BYTES=128                            every case at lanes of 128 bytes (a workgroup is 32 KiB, the look-back spans two lanes)
    old_way      TRRE_EXACT=0                                   the long run and the backward runs: the same bytes, no repair line in the trace
    one_walk     TRRE_ONE=1                                     long run, many runs, backward runs: the bytes alone (its look-back of 32 bytes misses these
                                                                constantly: tile repairs, void launches handed to the pair); the trace is printed
The forward rounds of a case whose input alone decides them (ONE lane is flagged per round: repair_cases.Case.single) must be the host shim's
for the same input and lane size, computed here — the order in which the threads run cannot change that —, and 1 + the workgroup edges crossed.
`long_run_aaa_dft` and `long_run_aaa_dft_guided` are NOT such cases: two lanes in three are flagged, every flagged lane stops the walk of the one
before it, a round settles one lane — 767 rounds on the shim —, and on the device the runtime gives up after n_chunks + 64 rounds and scans the
buffer the old way, in the stream family and in the guided one behind its backward pass (the bytes are the oracle's either way; the trace shows
n_chunks + 66 lines).  The many-runs cases stay under that bound whatever the order of the threads: repair_cases.max_flagged_lanes().

A repair that does less than it should still prints the oracle's bytes — the verification sees to that —: it shows in the ROUNDS, which is why
they are asserted wherever the input decides them.  The rounds measured on an MI355X are DESIGN.md 4.7's table; the children's wall times are in TIMES."""
import os
import subprocess
import sys
import time

import pytest

import gpu_repair_check as G                   # (its tables; nothing in it touches a GPU before a job runs)
import repair_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_repair_check.py")
BASE_ENV = {"TRRE_TRACE": "1", "TRRE_MAPGEN": "0"}
# job -> (seconds measured on an MI355X, process start to exit; the child's time limit)
TIMES = {"lanes2048": (6.5, 120), "lanes128": (3.1, 120), "old_way": (8.1, 120), "one_walk": (4.5, 120)}
_failed = []

# ---- the documented cases, written out (the child builds its table from repair_cases.cases()) ----------------------------------------------------
# (every forward program admits guided_gen: each of its cases runs as the family the library chooses and then with guided_gen forced)
_FWD = ["aa_nft", "aa_dft", "aa_a_nft"]
_BWD = ["star_nft", "star_dft", "plus_nft", "star_bytesym_nft"]


def _both(kind, tags):
    return [kind + t for t in tags] + [kind + t + "_guided" for t in tags]


_LONG = _both("long_run_", _FWD + ["aaa_dft"])
_MANY = _both("many_runs_", ["aa_nft", "aaa_dft"])
_BACK = ["backward_runs_" + t for t in _BWD]
DOCUMENTED = {
    "lanes2048": _LONG + _both("control_", _FWD) + _both("window_forward_", ["aa_nft", "aa_dft", "aaa_dft"])
    + _MANY + ["tail_%d_aa_%s" % (m, e) for m in (0, 5) for e in ("nft", "dft")] + _BACK + ["window_backward_" + t for t in _BWD],
    "old_way": _LONG + _BACK,
    "one_walk": _LONG + _MANY + _BACK,
}
DOCUMENTED["lanes128"] = DOCUMENTED["lanes2048"]


def shim_rounds(c, L):
    """repair rounds of a case on the host shim at the device's geometry (geo 0: lanes of 2 048 bytes; geo 2: of 128; workgroups of 256)"""
    import shim_lib
    import trre_amd
    p = trre_amd.Program(c.pat, c.eng)
    guided = c.family == "guided_gen" or p.info.kernel == trre_amd.KERNEL_GUIDED_GEN
    shim_lib.scan_like_runtime(p, c.data, geo={2048: 0, 128: 2}[L], family=shim_lib.GUIDED_GEN_EXACT if guided else shim_lib.STREAM_G16_EXACT)
    return shim_lib.last_rounds()


@pytest.mark.gpu
@pytest.mark.parametrize("job", list(G.JOBS))
def test_wrong_guesses_are_repaired_and_the_trace_says_so(job):
    assert not _failed, "the child of %r did not exit 0: nothing more is started" % _failed[0]
    env, L, names, trace = G.JOBS[job]
    e = {k: v for k, v in os.environ.items() if not k.startswith("TRRE_")}
    e.update(BASE_ENV)
    e.update(env)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(TIMES[job][1]), sys.executable, CHILD, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    wall = time.time() - t0
    err = r.stderr.decode("latin-1")
    print("\n".join(line for line in err.splitlines() if not line.startswith("trre: exact sub-ranges") or ": round 0," in line)[-20000:])
    if r.returncode != 0:
        _failed.append(job)
    assert r.returncode == 0, "%s: exit status %d\n%s" % (job, r.returncode, err[-3000:])
    res = eval(r.stdout.decode().strip().splitlines()[-1][len("RESULT "):])
    assert res["bad"] == [], res["bad"]
    assert res["cases"] == DOCUMENTED[job] == names
    assert res["extras"] == [(n, G.EXTRA_CHECKS) for n in G.EXTRAS]
    seen = dict(zip(res["cases"], res["rounds"]))
    print("%s: rounds (forward, backward): %r; column calls %r; seconds (oracle, scans, extras, the job) %r, the child from start to exit %.1f" %
          (job, {k: v[:2] for k, v in seen.items()}, res["column"], res["seconds"], wall))
    if trace == "quiet":
        assert all(v[:2] == (0, 0) for v in seen.values()) and res["column"][:2] == (0, 0), (seen, res["column"])
    if trace == "expect":
        # the column calls run this same scan on the markers' tables (guided_gen): a run of `a` from offset 1 over three lanes, the lanes whose
        # look-back begins inside it guess the parity wrong — in the size query and in the call that fills the arrays
        assert res["column"][0] >= 1 and res["column"][2] == "guided_gen", res["column"]
        cases = R.by_name(L)
        for name in names:
            c = cases[name]
            if c.single:                                       # one flagged lane per round: the shim's count, whatever the order of the threads
                assert seen[name][0] == shim_rounds(c, L) == R.forward_rounds(c.data, L), (name, seen[name])
        assert sum(v[0] > 0 for v in seen.values()) >= 10 and sum(v[1] > 0 for v in seen.values()) >= 4, seen


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------

def test_the_jobs_are_the_documented_ones():
    """the child's job table and this file name the same cases; every environment is a set of TRRE_* switches"""
    assert list(G.JOBS) == list(TIMES) == ["lanes2048", "lanes128", "old_way", "one_walk"] and set(DOCUMENTED) == set(TIMES)
    for job, (env, L, names, trace) in G.JOBS.items():
        assert names == DOCUMENTED[job], job
        assert all(k.startswith("TRRE_") for k in env) and not set(env) & set(BASE_ENV)
        assert [c.name for c in R.cases(128) if c.name in names] == names      # (the order of repair_cases.cases(), the same names for both lane sizes)
        assert set(G.EXTRAS) <= set(names)
    assert [c.name for c in R.cases(2048)] == [c.name for c in R.cases(128)] == DOCUMENTED["lanes2048"]
    assert [(G.JOBS[j][0], G.JOBS[j][1], G.JOBS[j][3]) for j in G.JOBS] == [({}, 2048, "expect"), ({"TRRE_LANE_BYTES": "128"}, 128, "expect"),
                                                                            ({"TRRE_EXACT": "0"}, 2048, "quiet"), ({"TRRE_ONE": "1"}, 2048, "print")]
    assert all(limit >= 120 and limit >= 10 * seconds for seconds, limit in TIMES.values())
