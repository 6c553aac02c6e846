"""GPU tier: the count / emit handshake (trre_amd/csrc/pass_block.hpp) at the caller's capacity, for every kernel that carries it.

The capacity predicate of the emit prologue has one owner, and this file is what guards it (the listing audits of tests/test_lds_audit.py pass
with the predicate negated).  For every case trre_scan_device is called twice through the C ABI, with need = len(the oracle's output):
    cap = need        rc 0, out_len == need and the bytes are the oracle's
    cap = need - 1    TRRE_E_CAPACITY and out_len == need
and in both calls the sentinel-filled 1 MiB behind `cap` comes back untouched.

Inputs: seeded word soup (tests/corpus.py) of exactly 130 KiB and 165 KiB, the last line without a newline.  Chunks of the workspace:
    direct families   TRRE_LANE_BYTES=128 x direct_block_threads() = 256 lanes: 32 KiB per chunk      5 and 6 chunks
                      (the grouped kernels' last workgroup has a dead group: 6 mod 4 for the 1024-thread count / mark kernels and 5 mod 2 for
                      the 512-thread emit / splice kernels)
    tile kernels      chunk_bytes(dft) = GeoDft::CHUNK = 32 KiB                                         5 and 6 chunks
    generator         kGenLaneBytes = 512 x 256 lanes: 128 KiB                                         2 and 2 chunks
    backtracking      kBtLaneBytes = 1024 x 256 lanes: 256 KiB (TRRE_LANE_BYTES does not apply)        1 and 1 chunk
    lazy tables       kLazyLaneBytes = 1024 x 256 lanes: 256 KiB                                       1 and 1 chunk
TRRE_MAPGEN=0 everywhere: left to itself `a:xyz` takes the memoryless one-pass kernel on a context's first scan, which has no handshake.

    case                 pattern / engine                          environment                         kernels
    axyz_tile            a:xyz dft, forced tile_gen                                                    k_scan_count / k_scan_emit
    axyz_g16             a:xyz dft                                                                     k_stream_g16<1> / <2>
    axyz_direct          a:xyz dft                                 TRRE_NO_G16=1                       k_stream_direct<1> / <2>
    dict_mark4_splice    the seeded 1000-entry dictionary, dft                                         k_fb_mark4 + k_fb_splice
    dict_mark            the same                                  TRRE_NO_FB_MARK4=1                  k_fb_mark + k_fb_splice
    dict_fb              the same                                  TRRE_NO_FB_COPY=1 TRRE_FB_EMIT=1    k_stream_fb<1> / <2>
    wide_fwd             a(a|b|c){9}c:x nft, forced guided_gen                                         k_wide_fwd<1> / <2>
    backtrack            a(a|b|c|d|e|f|g|h){12}c:x nft                                                 k_bt<1> / <2>
    lazy                 (a|b)*a(a|b){18}:x dft                                                        k_lazy<1> / <2>
    generate             [a-z ]*|.* nft, `-ma`                                                         k_gen<1> / <2>
The generator's emit pass writes into a buffer of the library's own, so k_gen's capacity predicate never sees the caller's capacity: there the host
compares the size with `cap` — the same two calls, the same assertions, answered by trre_scan_device itself.

The switches are read once per process: every environment is a child (tests/gpu_handshake_check.py <job>), one after the other, each under its own
timeout; after a child that did not exit 0 nothing more is started on the GPU by this file."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_handshake_check.py")
BASE_ENV = {"TRRE_LANE_BYTES": "128", "TRRE_MAPGEN": "0"}
JOBS = [("default", ["axyz_tile", "axyz_g16", "dict_mark4_splice", "wide_fwd", "backtrack", "lazy", "generate"]),
        ("no_g16", ["axyz_direct"]), ("no_mark4", ["dict_mark"]), ("fb_emit", ["dict_fb"])]
_failed = []


def _jobs():
    import gpu_handshake_check                 # (its tables; nothing in it touches a GPU before a job runs)
    return gpu_handshake_check.JOBS


@pytest.mark.gpu
@pytest.mark.parametrize("job,cases", JOBS, ids=[j for j, _ in JOBS])
def test_capacity_exact_and_one_byte_short(job, cases):
    assert not _failed, "the child of %r did not exit 0: nothing more is started" % _failed[0]
    e = {k: v for k, v in os.environ.items() if not k.startswith("TRRE_")}
    e.update(BASE_ENV)
    e.update(_jobs()[job][0])
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, CHILD, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    err = r.stderr.decode("latin-1")
    print(err[-6000:])
    if r.returncode != 0:
        _failed.append(job)
    assert r.returncode == 0, "%s: exit status %d\n%s" % (job, r.returncode, err[-3000:])
    res = eval(r.stdout.decode().strip().splitlines()[-1][len("RESULT "):])
    assert res["bad"] == [], res["bad"]
    assert res["cases"] == cases and res["calls"] == 4 * len(cases), res


def test_the_jobs_are_the_documented_ones():
    """(CPU tier) the child's table and this file's list name the same cases, and every environment is a set of TRRE_* switches"""
    jobs = _jobs()
    assert [(j, [c[0] for c in jobs[j][1]]) for j, _ in JOBS] == JOBS and len(jobs) == len(JOBS)
    assert all(k.startswith("TRRE_") for env, _ in jobs.values() for k in env)
