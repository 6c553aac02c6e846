"""GPU tier: the memoryless one-pass kernel (k_mapgen: trre_amd/csrc/map_kernels.hip, map_block.hpp) against the ORACLE — never against the count /
emit pair, never against another run of the engine.  Wall time on an MI355X: 3 min 40 s for the 15 GPU tests (measured: 219 s; the four edge
tests are 150 s of it, the window of 16 alone 65 s; the 256 MiB and 1 GiB oracle comparisons 15 s and 5 s — the oracle runs on 16 host threads).

TRRE_MAPGEN* are read once per process: every environment is a child (tests/gpu_mapgen_check.py <job>), each under its own timeout; a child that
exits non-zero fails its test and nothing more is started on the GPU in that test.  Every child runs with TRRE_MAPGEN_PROF=1 and TRRE_TRACE=1, and
the parent COUNTS: the kernel's phase-clock line once per scan of at least one byte, and "was void" never, wherever no input holds a NUL — not one
of those scans may have been answered by another kernel.  A program of its own wherever a context's history could change the route.

What the programs make the kernel do (gpu_mapgen_check.PROGRAMS; test_the_programs_are_memoryless_and_reach_every_instantiation reads it off the tables):
    k_mapgen<first_lookup, multi>   <0,0> '[aie]:' '[a-z]:' '.:'    <1,0> '(a:b|e:)'    <0,1> 'a:xyz' HTML escapes ':x' ..    <1,1> '(a:b|e:|c:xyz)'
    every text length 0..8 in one table                       '(a:|b:bb|..|h:hhhhhhhh)'
    tiles whose total is 0 (lines longer than a tile)          '[a-z]:' and '.:' on the corpus' long lines (of lowercase letters; of anything)
    8 x, 128 KiB per tile: four default windows, 8192 of 16    'e:12345678' on lines of mostly 'e'; '.:12345678'
    insertion at the empty string                              ':x' (NFT; the DFT program is a byte map)
The windows: the default (18 432), 16 384, 8 192 and 16 — the floor: runtime.cpp takes any TRRE_MAPGEN_WINDOW > 0 and rounds it up to a multiple
of 16; launch_mapgen has an upper limit only (the CU's LDS)."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_mapgen_check.py")
WINDOWS = [None, "16384", "8192", "16"]
_grid = {}


def child(job, env, timeout, grid=0, tmp=None):
    """one job in a process of its own; returns (its result, its stderr)"""
    e = dict(os.environ)
    for k in list(e):
        if k.startswith("TRRE_MAPGEN"):
            del e[k]
    e.update({"TRRE_MAPGEN": "1", "TRRE_MAPGEN_PROF": "1", "TRRE_TRACE": "1"})
    e.update({k: v for k, v in env.items() if v is not None})
    for k, v in env.items():
        if v is None:
            e.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, CHILD, job, str(grid)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    err = r.stderr.decode("latin-1")
    assert r.returncode == 0, "%s: exit status %d\n%s" % (job, r.returncode, err[-3000:])
    res = eval(r.stdout.decode().strip().splitlines()[-1][len("RESULT "):])
    print("%s %s: %d scans, %d on k_mapgen, %d void, %s" % (job, {k: v for k, v in env.items() if k != "TRRE_MAPGEN_DBG"}, res["scans"], err.count("memoryless kernel, shader clocks"),
                                                            err.count("was void"), {k: v for k, v in res.items() if k not in ("scans", "bad")}))
    return res, err


def on_mapgen(err):
    return err.count("memoryless kernel, shader clocks")


def all_on_mapgen(res, err):
    """the guard against a hollow pass: every scan was a launch of k_mapgen, none was void, and every output was the oracle's"""
    assert res["bad"] == [] and res["n_bad"] == 0, res["bad"]
    assert res["scans"] > 0 and on_mapgen(err) == res["scans"], (on_mapgen(err), res["scans"])
    assert "was void" not in err


def grid(window, tmp_path):
    """G, the workgroups of a launch at this window — from a launch (the kernel's own record of who took which tile), not from a CU count"""
    if window not in _grid:
        dbg = str(tmp_path / ("dbg_%s.bin" % window))
        res, _ = child("grid", {"TRRE_MAPGEN_WINDOW": window, "TRRE_MAPGEN_DBG": dbg}, 300)
        _grid[window] = res["grid"]
    return _grid[window]


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
def test_tile_and_grid_edges_against_the_oracle(window, tmp_path):
    """sizes k 16384 + d, k in {0, 1, 2, 3, G - 1, G, G + 1, 2 G + 1}, d in {-1, 0, 1, 15, 17}, input views at 0 / 1 / 7 / 8 / 15 and output views at
    0 / 1 / 15 of their allocations, final lines without '\\n', '\\n' alone, nothing: twenty programs on both engines, at every window"""
    G = grid(window, tmp_path)
    res, err = child("edges", {"TRRE_MAPGEN_WINDOW": window}, 900, G)
    all_on_mapgen(res, err)
    assert res["scans"] >= 20 * 40


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, "16"])
def test_golden_vectors_on_the_memoryless_kernel(window):
    """every golden vector whose program is memoryless, forced onto k_mapgen, against its recorded output.  Eleven golden inputs hold NULs: those
    launches are void and the general family answers — no other launch may be"""
    res, err = child("golden", {"TRRE_MAPGEN_WINDOW": window}, 600)
    assert res["bad"] == [], res["bad"]
    assert res["vectors"] > 0 and on_mapgen(err) == res["scans"], (res, on_mapgen(err))
    assert err.count("was void") <= res["with_nul"], (err.count("was void"), res["with_nul"])


@pytest.mark.gpu
@pytest.mark.parametrize("mib", [256, 1024])
def test_look_back_depth_against_the_oracle(mib):
    """one round trip of the look-back reaches 8 192 tiles back and the second poll the 64 groups before: 16 384 tiles for every program, 65 536 for
    '[aie]:' and 'a:xyz', on a corpus whose tiles' totals differ and trend (a tile placed with a neighbour's total moves bytes) — whole outputs"""
    res, err = child("depth", {"MAPGEN_CHECK_MIB": str(mib)}, 1100)
    all_on_mapgen(res, err)
    assert res["scans"] == (20 if mib == 256 else 2)


@pytest.mark.gpu
def test_nuls_void_the_launch_and_the_bytes_stay_the_oracles():
    res, err = child("nul", {}, 600)
    assert res["bad"] == [], res["bad"]
    assert res["scans"] == 3 * 10 and "memoryless kernel was void" in err


@pytest.mark.gpu
def test_default_routing_of_a_dense_program():
    """TRRE_MAPGEN unset, 'a:xyz' three times on one program: k_mapgen once, then the pair (mapgen_dense) — the oracle's bytes all three times"""
    res, err = child("default", {"TRRE_MAPGEN": None}, 300)
    assert res["bad"] == [] and res["scans"] == 3, res
    assert res["grew"] > 1.04 and on_mapgen(err) == 1 and "was void" not in err, (res["grew"], on_mapgen(err))


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, "16"])
def test_capacity_exact_and_one_byte_short(window):
    res, err = child("capacity", {"TRRE_MAPGEN_WINDOW": window}, 600)
    all_on_mapgen(res, err)


@pytest.mark.gpu
def test_alternating_programs_on_one_device(tmp_path):
    """The regression test of the staging race (tests/test_lds_audit.py proves the barrier): four programs whose length tables
    disagree on most lowercase letters, in turn, on G tiles — every tile is its workgroup's first, counted right after the tables were staged, and
    the LDS holds the tables of the program before.  64 rounds, compared on the device with the oracle's bytes."""
    G = grid(None, tmp_path)
    res, err = child("alternate", {}, 600, G)
    all_on_mapgen(res, err)
    assert res["rounds"] == 64 and res["scans"] == 64 * 4


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, "16"])
def test_random_memoryless_programs(window, tmp_path):
    """tools/gpu_fuzz.py's memoryless generator, seeds 11 / 12 / 13 with 30 patterns each (gpu_mapgen_check.FUZZ_SEEDS), 1..5 tiles and G + 1,
    random alignment; at most a quarter of the patterns skipped, at least 50 run"""
    res, err = child("fuzz", {"TRRE_MAPGEN_WINDOW": window}, 600, grid(window, tmp_path))
    all_on_mapgen(res, err)
    assert res["drawn"] == 90 and res["skipped"] * 4 <= res["drawn"] and res["drawn"] - res["skipped"] >= 50, res


# ---- CPU tier: the lists above are what they say ---------------------------------------------------------------------------------------

def _tables(pat, eng):
    import shim_lib
    import trre_amd
    p = trre_amd.Program(pat, eng)
    assert shim_lib.has_mapgen(p), (pat, eng)
    assert {v: k for k, v in trre_amd.KERNEL_NAMES.items()}["stream_gen"] in p.allowed_kernels(), (pat, eng)
    blob = p.export_stream_tables()
    h = struct.unpack_from("<48I", blob, 0)
    t = struct.unpack_from("<1024I", blob, h[45])
    # launch_mapgen's choice: (first_lookup: some byte prints ONE byte that is not itself; multi: the longest text has two bytes or more)
    first = any((t[4 * c + 2] & (15 | 0x80)) == 1 and (t[4 * c] & 0xff) != c for c in range(256))
    return (first, h[46] > 1), [t[4 * c + 2] & 15 for c in range(256)], t


def _child_lists():
    import gpu_mapgen_check                    # (its lists; nothing in it touches a GPU before a job runs)
    return gpu_mapgen_check.PROGRAMS, gpu_mapgen_check.ALTERNATING


def test_the_programs_are_memoryless_and_reach_every_instantiation():
    """every program of the GPU lists carries the memoryless form (the lists can never quietly test something else), the four instantiations of
    k_mapgen are all reached, one table holds every text length 0..8, the two engines' tables of a pattern are the same tables, and the alternating
    programs' length tables disagree on most lowercase letters"""
    programs, alternating = _child_lists()
    where, by_pat = {}, {}
    for pat, eng in programs:
        inst, lens, t = _tables(pat, eng)
        where.setdefault(inst, []).append((pat, eng))
        by_pat.setdefault(pat, []).append(t)
    print({k: [p for p, _ in v] for k, v in where.items()})
    assert set(where) == {(False, False), (True, False), (False, True), (True, True)}, where
    assert any(set(_tables(pat, eng)[1]) >= set(range(9)) for pat, eng in programs)
    assert all(ts[0] == ts[1] for ts in by_pat.values() if len(ts) == 2)
    lens = [_tables(pat, eng)[1] for pat, eng in alternating]
    assert len(lens) >= 3
    low = range(ord("a"), ord("z") + 1)
    assert sum(lens[0][c] != lens[1][c] for c in low) >= 24
    for i in range(len(lens)):
        for j in range(i):
            assert sum(lens[i][c] != lens[j][c] for c in low) >= 8, (i, j)


def test_the_fuzz_seeds_stay_inside_the_cap():
    """the seeds of test_random_memoryless_programs, with Oracle() and the tables alone: at most a quarter of the drawn patterns are refused or
    not memoryless, at least 50 are left"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_fuzz
    drawn = skipped = 0
    for seed in (11, 12, 13):
        plan = gpu_fuzz.memoryless_plan(seed, 30)
        drawn += len(plan)
        skipped += sum(1 for _, progs in plan if not progs)
    print("drawn %d, skipped %d" % (drawn, skipped))
    assert drawn == 90 and skipped * 4 <= drawn and drawn - skipped >= 50
