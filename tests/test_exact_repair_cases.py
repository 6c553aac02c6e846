"""CPU tier of the repair of the exact sub-ranges: every case of tests/repair_cases.py through the kernels' bodies on the host shim
at the PRODUCTION look-back (families STREAM_G16_EXACT / GUIDED_GEN_EXACT, not the _MISS families with their 4-byte look-back), against the
oracle — and the repair rounds each case needs there (shim_lib.last_rounds()).  That is what keeps tests/test_gpu_exact_repair.py from passing
without testing anything: a provoking case provokes, a control does not, for the reference model alone and without a GPU.

Geometries: geo 0, lanes of 2 048 bytes in workgroups of 256, runs cases(2048) with their expectations and cases(128) for the bytes alone; geo 2,
lanes of 128 bytes in workgroups of 256 (what TRRE_LANE_BYTES=128 runs on the device), runs cases(128) with their expectations.

Repair rounds on the shim (forward + backward; the shim runs a launch's lanes one after the other):
    case                                        L = 2048    L = 128
    long_run_*  aa:x, (aa:x|a:y), also guided   4           4          1 + three workgroup edges
    long_run_aaa_dft, also guided               767         773        (one lane settled per round)
    control_*                                   0           0
    window_forward_*  aa:x / aaa:xy             1 / 3       1 / 2
    many_runs_*       aa:x / aaa:xy             1 / 4       2 / 67
    tail_*                                      2           2          1 + one workgroup edge
    backward_runs_*, window_backward_*          1           1          (backward rounds)"""
import re
import struct

import pytest

import repair_cases as R
import shim_lib
import trre_amd
from oracle_lib import Oracle

_progs, _wants = {}, {}


def prog(pat, eng):
    if (pat, eng) not in _progs:
        _progs[pat, eng] = trre_amd.Program(pat, eng)
    return _progs[pat, eng]


def want_of(c):
    """the oracle's bytes, computed once per (program, input)"""
    key = (c.pat, c.eng, c.data)
    if key not in _wants:
        _wants[key] = Oracle(c.pat, c.eng).scan(c.data)
    return _wants[key]


def guided(c):
    return c.family == "guided_gen" or prog(c.pat, c.eng).info.kernel == trre_amd.KERNEL_GUIDED_GEN


def on_the_shim(c, geo):
    """(bytes, repair rounds) of a case through the exact family of its tables"""
    fam = shim_lib.GUIDED_GEN_EXACT if guided(c) else shim_lib.STREAM_G16_EXACT
    got = shim_lib.scan_like_runtime(prog(c.pat, c.eng), c.data, geo=geo, family=fam)
    return got, shim_lib.last_rounds()


def check_expectation(c, rounds, L):
    if c.expect is None:
        return
    if c.expect[0] == "none":
        assert rounds == 0, (c.name, L, rounds)
    else:
        assert rounds >= c.expect[1], (c.name, L, rounds)
    if c.expect[0] == "backward":                 # (one round settles every run, see repair_cases.Case; the forward pass of these patterns forgets)
        assert rounds == 1, (c.name, L, rounds)
    if c.single:
        assert rounds == R.forward_rounds(c.data, L), (c.name, L, rounds)
    if c.expect[0] == "forward":                  # (no order of execution needs more rounds than the longest run has lanes that can guess wrong)
        assert rounds <= R.max_flagged_lanes(c.data, L), (c.name, L, rounds)


@pytest.mark.parametrize("L,geo", [(2048, 0), (128, 2), (128, 0)], ids=["lanes2048", "lanes128", "lanes128_inputs_on_2048"])
def test_every_case_on_the_shim_at_the_production_look_back(L, geo):
    seen = []
    for c in R.cases(L):
        got, rounds = on_the_shim(c, geo)
        want = want_of(c)
        print("%s L=%d geo %d: n=%d, %d bytes out, %d round(s)" % (c.name, L, geo, len(c.data), len(want), rounds))
        assert got == want, (c.name, L, geo)
        if (L, geo) != (128, 0):                     # (the inputs built for 128-byte lanes on lanes of 2 048: the bytes alone)
            check_expectation(c, rounds, L)
        seen.append(c.expect and c.expect[0])
    assert seen.count("forward") >= 10 and seen.count("backward") >= 4 and seen.count("none") >= 5


def test_the_greedy_reference_agrees_with_the_oracle():
    """aa:x, (aa:x|a:y), aaa:xy: a left-to-right greedy replace per line, written in repair_cases.py — a second reference, no regex engine"""
    n = 0
    for L in (2048, 128):
        for c in R.cases(L):
            if c.pat in R.GREEDY:
                assert R.greedy(c.pat, c.data) == want_of(c), (c.name, L)
                n += 1
    assert n >= 40
    assert R.greedy("aa:x", b"baaa\nxaaaa") == b"bxa\nxxa\n" and R.greedy("(aa:x|a:y)", b"aaa\n") == b"xy\n" and R.greedy("aaa:xy", b"aaaaa b\n") == b"xyaa b\n"


def test_the_programs_are_what_the_cases_say():
    """the families the cases run, and the symbols of the backward pass: 4 bits (kNib, sym_mode 2) and 8 (sym_mode 1)"""
    for pat, eng in R.PARITY + [R.THIRDS]:
        p = prog(pat, eng)
        assert p.info.kernel == trre_amd.KERNEL_STREAM_GEN and shim_lib.has_g16(p.export_stream_tables()), (pat, eng)
    # guided_gen is forced for EVERY forward program that admits it, no more and no fewer
    assert R.GUIDED == [k for k in R.PARITY + [R.THIRDS] if trre_amd.KERNEL_GUIDED_GEN in prog(*k).allowed_kernels()]
    for L in (2048, 128):
        names = {c.name for c in R.cases(L)}
        for c in R.cases(L):
            if c.family is None and (c.pat, c.eng) in R.GUIDED and c.name.startswith(("long_run_", "control_", "window_forward_", "many_runs_")):
                assert c.name + "_guided" in names, c.name
    for pat, eng in R.GUIDED:
        assert shim_lib.has_g16(prog(pat, eng).export_guided_tables()[1]), (pat, eng)
    bits = {}
    for pat, eng in R.BACKWARD + [R.BYTE_SYMBOLS] + R.GUIDED:
        p = prog(pat, eng)
        rblob, gblob = p.export_guided_tables()
        assert shim_lib.has_g16(gblob) and 0 < p.info.guided_rev_states <= 256, (pat, eng)
        bits[pat, eng] = struct.unpack_from("<8I", rblob, 0)[7]          # (device_blob.hpp: RevBlobHeader::sym_bits)
    for pat, eng in R.BACKWARD + [R.BYTE_SYMBOLS]:
        assert prog(pat, eng).info.kernel == trre_amd.KERNEL_GUIDED_GEN, (pat, eng)
    assert all(bits[k] == 4 for k in R.BACKWARD + R.GUIDED) and bits[R.BYTE_SYMBOLS] == 8, bits


@pytest.mark.parametrize("L", [2048, 128])
def test_the_inputs_are_what_their_names_say(L):
    G = 256 * L
    c = R.by_name(L)
    run, control = c["long_run_aa_nft"].data, c["control_aa_nft"].data
    assert run.index(b"aa") == 1 and control.index(b"aa") == 2 and run.count(b"a" * (3 * G + 1001)) == 1 and b"a" * (3 * G + 1002) not in run
    assert R.forward_rounds(run, L) == 4 and R.forward_rounds(control, L) == 0
    assert len(run) <= 1600 * 1024 and run.endswith(b"c\n" + R.SHORT)
    # the window edges: a run of 3 L + 1 whose first byte is d in front of a lane start, five far from a line start and five after a '\n'
    wf = c["window_forward_aa_nft"].data
    starts = [i for i in range(1, len(wf)) if wf[i:i + 300] == b"a" * 300 and wf[i - 1] != 0x61]
    assert [-s % L for s in starts] == [d % L for d in (0, 1, 255, 256, 257)] * 2
    assert [wf[s - 1] == 0x0A for s in starts] == [False] * 5 + [True] * 5 and all(b"\n" not in wf[s - 599:s - 1] for s in starts)
    assert all(wf[s:s + 3 * L + 2] == b"a" * (3 * L + 1) + b"b" for s in starts)
    mr = c["many_runs_aa_nft"].data
    runs = [len(m.group()) for m in re.finditer(rb"a{100,}", mr)]
    assert len(runs) == 40 and min(runs) >= 300 and max(runs) <= 9000
    # the runtime gives up after n_chunks + 64 rounds: whatever the order of the threads, the forty runs stay under that (the GPU tier asserts it)
    assert R.max_flagged_lanes(mr, L) <= (len(mr) + G - 1) // G + 64, (L, R.max_flagged_lanes(mr, L))
    for more in (0, 5):
        t = c["tail_%d_aa_nft" % more].data
        assert t[-1:] == b"a" and len(t) % L and b"\n" not in t and R.forward_rounds(t, L) == 2
    assert len(c["tail_5_aa_nft"].data) == len(c["tail_0_aa_nft"].data) + 5
    # backward: runs of [ab] of 300 and more, under 30 000; their ends; one across a multiple of G; one over a lane edge with a `c` far behind it
    br = c["backward_runs_star_nft"].data
    found, i = [], 0
    while i < len(br):
        j = i
        while j < len(br) and br[j] in b"ab":
            j += 1
        if j - i >= 300:
            found.append((i, j, br[j:j + 1]))
        i = j + 1
    assert len(found) == 32 and all(300 <= j - i < 30000 for i, j, _ in found)
    assert {e for _, _, e in found} == {b"c", b"d", b"\n", b" "} and any(br[j:j + 2] == b"c\n" for _, j, _ in found)
    assert any(i < k * G < j and e == b"c" for i, j, e in found for k in (1, 2, 3))
    assert any(e == b"c" and (i // L + 1) * L + R.LOOK < j and j - i > 2 * L for i, j, e in found)
    wb = c["window_backward_star_nft"].data
    found = [(m.start(), m.end()) for m in re.finditer(rb"[ab]{300,}", wb)]
    assert [e % L for _, e in found] == [d % L for d in (255, 256, 257)] * 2 and [wb[e] for _, e in found] == [0x63] * 3 + [0x0A] * 3
    assert all(e - s > L + R.LOOK for s, e in found)
