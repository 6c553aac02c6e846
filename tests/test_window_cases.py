"""CPU tier of the window kernel's placed edges (tests/window_cases.py): every case's claims hold in its bytes; every case through the lane and
mover code of k_stream_lpw on the host shim (families 8 and STREAM_LPW_PAIR, lanes of 128 and 2 048 bytes, input and output 0 and 5 bytes off
16-byte alignment) against the oracle; and the lanes the shim handed to the redo pass are the ones window_cases.expected_redo() derives by hand.
That is what keeps tests/test_gpu_window.py from passing without testing anything: an edge that is named is there, for the reference model alone
and without a GPU.

Sharpness.  Four mutations of scan_block.hpp, one at a time, on a copy of the tree; test_every_case_on_the_shim against the mutated copy:
    mutation                                                 the placed edges of `main` that catch it (catdog_nft; lanes of 128 and of 2 048 alike)
    `rend <= rv + kWtPiece - 16` -> `<= rv + kWtPiece`       tail:hi-1, hi+48, hi+49, hi+63, hi+B-1; head:residue_0, 63, 64, 127, at_B-1, nl_at_B-1, nl_at_-1_and_0
    `>=` -> `>` in WtMover::stores                           head:residue_112 (and tail:hi+47)
    the head loop of WtLane::emit from `rfs - r0 + 1`        head:lane_1_behind_the_redone_lane, one byte: everywhere else the lane in front writes those bytes too
    `hit` without `(p1 >= rhi)`                              every head and tail edge
Every mutation also fails the vend_*, final_* and nul_* cases of several programs, in their soup; the redo list of `main` stays right under all four.

What the shim cannot run — the steady unconditional stores, the wait counters, the direct-to-LDS loads, the swizzle against real LDS — is the GPU
tier's."""
import struct

import pytest

import shim_lib
import trre_amd
import window_cases as W
from oracle_lib import Oracle

NL = 0x0A
_progs, _wants = {}, {}


def prog(p):
    if p.tag not in _progs:
        _progs[p.tag] = trre_amd.Program(p.pat, p.eng)
    return _progs[p.tag]


def want_of(p, c):
    """the oracle's bytes, computed once per (program, input)"""
    key = (p.pat, p.eng, c.name, c.B, c.a)
    if key not in _wants:
        _wants[key] = Oracle(p.pat, p.eng).scan(c.data)
    return _wants[key]


def form_of(p):
    """the table form the launcher chooses, from the stream tables' header (device_blob.hpp: lpw_bytes, lpw_delay, lpw2_bytes): (form, delay)"""
    h = struct.unpack_from("<36I", prog(p).export_stream_tables(), 0)
    if h[12] == 0:
        return None, 0
    assert h[12] <= 32768, (p.tag, h[12])            # (build_window_form's bound = the kernel's LDS room: entries are never read from global memory)
    return ("wide" if h[13] > 3 else "pair" if 0 < h[35] <= 32768 else "narrow"), h[13]


def test_the_programs_have_the_forms_the_table_says():
    forms = {}
    for p in W.PROGRAMS:
        assert prog(p).info.kernel == trre_amd.KERNEL_STREAM_LP, p.tag
        form, delay = form_of(p)
        if form is None:
            assert (p.pat, p.eng) in W.NO_WINDOW_FORM, p.tag
            continue
        assert (p.pat, p.eng) not in W.NO_WINDOW_FORM and (form, delay) == (p.form, p.delay), (p.tag, form, delay)
        forms.setdefault((form, delay), set()).add(p.eng)
    # narrow entries of delays 1, 2, 3, wide ones of 4, 5, 6, 7, the pair form and a narrow program without it; both engines everywhere
    assert {d for f, d in forms if f in ("pair", "narrow")} == {1, 2, 3} and {d for f, d in forms if f == "wide"} == {4, 5, 6, 7}
    assert ("narrow", 2) in forms and ("pair", 2) in forms and all(e == {"nft", "dft"} for e in forms.values())
    assert all(W.program(t).form == f for t, f in zip(W.BIG_PROGRAMS, ("pair", "wide")))


# ---- the claims ----------------------------------------------------------------------------------------------------------------------------------

def first_line_start(v, lo, hi):
    """the first offset in [lo, hi) with a '\\n' right before it; None: none"""
    if v[lo - 1] == NL:
        return lo
    p = v.find(b"\n", lo, hi - 1)
    return None if p < 0 else p + 1


def check_claims(c, key):
    B, a, K = c.B, c.a, len(key)
    v = b"\xaa" * a + c.data
    vend = len(v)
    assert vend == a + len(c.data) and (b"\0" in c.data) == c.nul
    assert max(len(ln) for ln in c.data.split(b"\n")) < W.LONG
    kinds = set()
    for name, X in c.edges:
        kind, _, what = name.partition(":")
        kinds.add(kind)
        lo = X // B * B
        if kind not in ("end", "final", "first") and name != "nul:last_piece":        # outside the redo zones
            assert a + 64 <= X < vend - 3 * 64 - B, (c.name, name, X)
        if kind == "head":
            assert first_line_start(v, lo, lo + B) == X and X // B not in c.redo, (c.name, name, X)
            if what.startswith("residue_"):
                assert X % 128 == int(what[8:]), (c.name, name, X)
            if what == "last_piece":
                assert B - 64 <= X - lo < B
            if what == "at_B-1":
                assert X - lo == B - 1
            if what.startswith("nl_at_B-1"):
                assert X == lo and X // B - 1 in c.no_start and v.count(b"\n", lo - B - 1, lo) == 1
            if what == "nl_at_-1_and_0":
                assert X == lo and v[X - 1] == v[X] == NL
        elif kind == "tail":
            d = W.tails(B)[what]
            hi = X - d
            assert hi % B == 0 and v[X] == NL and b"\n" not in v[hi - 1:X], (c.name, name, X)
            start = v.rfind(b"\n", 0, max(hi - 1, 0) if d >= 0 else X) + 1
            assert hi - B <= start < hi and (hi // B - 1) not in c.redo, (c.name, name, X, start)      # the line starts in that lane: its last one
        elif kind == "inline":
            s, e = v.rfind(b"\n", 0, X) + 1, v.find(b"\n", X)
            assert X % B == 0 and v[X - K:X + K] == key + key and (X - s >= B or e - X >= B), (c.name, name, X)
        elif kind == "split":
            edge, i = what.split(":")
            i = int(i)
            assert W.SPLIT_KINDS[edge](X, B) and v[X - i:X - i + K] == key and (i < K or v[X:X + K] == key), (c.name, name, X)
        elif kind == "run":
            n = int(what.split("_")[0])
            assert v[X:X + n] == b"\n" * n and X // B != (X + n - 1) // B and v[X - 1] != NL and v[X + n] != NL
        elif kind == "end":
            assert X == vend and X - W.END_LANES * B == int(what.split("_")[1])
        elif kind == "final":
            n = vend - X
            assert v[X - 1] == NL and b"\n" not in v[X:] and (n == int(what) if what != "long" else n >= B + 256)
            if what == "long":                                  # the lane the line starts in is handed over mid-walk, not at init
                assert X // B in c.redo and (X // B + 1) * B + 192 <= vend and first_line_start(v, lo, lo + B) is not None
        elif kind == "first":
            assert X == a and v[a:a + K] == key
        elif kind == "nul":
            assert v[X] == 0 and v.count(b"\0") == 1
            assert {"lane_end": X % B == B - 1, "lane_start": X % B == 0, "skipped_head": lo <= X < first_line_start(v, lo, lo + B),
                    "last_piece": vend - 64 <= X}[what], (c.name, name, X)
        else:
            raise AssertionError("an edge of an unknown kind: %r" % (name,))
    for L in c.no_start:
        assert first_line_start(v, L * B, L * B + B) is None and L not in c.redo, (c.name, L)
    assert 0 in c.redo and c.redo == tuple(sorted(c.redo)) and (vend - 1) // B in c.redo
    return kinds


def check_keys(c, want):
    """the oracle's output differs from the input inside the 16 bytes before and after every placed key edge (length-preserving programs: without
    a NUL the output lies where the input lies)"""
    assert len(want) == len(c.data)
    n = 0
    for name, X in c.edges:
        if name.split(":")[0] in ("head", "tail", "inline", "split"):
            i = X - c.a
            assert want[i - 16:i] != c.data[i - 16:i] and want[i:i + 16] != c.data[i:i + 16], (c.name, name, X)
            n += 1
    return n


@pytest.mark.parametrize("B,mis,tags", [(128, (0, 5, 15), None), (2048, (0, 5, 15), None), (16384, (0, 5), W.BIG_PROGRAMS)],
                         ids=["lanes128", "lanes2048", "lanes16k"])
def test_every_claim_holds_in_the_bytes(B, mis, tags):
    progs = [p for p in W.PROGRAMS if tags is None or p.tag in tags]
    for a in mis:
        seen, keyed = set(), 0
        for key in sorted({p.key for p in progs}):
            cs = W.cases(B, a, key)
            assert [c.name for c in cs] == W.NAMES
            for c in cs:
                assert (c.a, c.B) == (a, B)
                seen |= {(c.name, k) for k in check_claims(c, key)}
                if not c.nul:
                    for p in progs:
                        if p.key == key:
                            keyed += check_keys(c, want_of(p, c))
        names = {e.name for c in W.cases(B, a, progs[0].key) for e in c.edges}
        # every group of the issue is there: ten residues and four more heads, twelve tails, lanes without a start, splits over seven kinds of
        # edge at every inner position, the ends, the NULs
        assert {"head:residue_%d" % r for r in W.HEAD_RESIDUES} | {"head:last_piece", "head:at_B-1", "head:nl_at_-1_and_0", "run:300_empty_lines",
                "head:nl_at_B-1_next_lane_starts_at_0"} <= names
        assert {"tail:" + t for t in W.tails(B)} <= names and len(W.tails(B)) == 12
        K = len(progs[0].key)
        assert {"split:%s:%d" % (k, i) for k in ("dword", "block", "piece", "row", "lane") for i in range(1, K + 1)} <= names
        every = [e.name for c in W.cases(B, a, progs[0].key) for e in c.edges]
        assert sum(n.startswith("split:wave:") for n in every) == 3 and sum(n.startswith("split:workgroup:") for n in every) == 1
        assert any(n.startswith("inline:across_workgroup_edge") for n in names) and any(n.startswith("inline:1_lane:") for n in names)
        if B <= 2048:
            assert any(n.startswith("inline:2_lanes:") for n in names) and any(n.startswith("inline:3_lanes:") for n in names)
        main = W.cases(B, a, progs[0].key)[0]
        if B == 128:                                            # a whole wave without an active lane
            assert any(n.startswith("inline:whole_wave") for n in names) and set(range(320, 384)) <= set(main.no_start)
        assert len(main.data) + a == W.MAIN_LANES * B + 100 and keyed >= 100


# ---- the shim --------------------------------------------------------------------------------------------------------------------------------

def on_the_shim(p, c, geo, fam):
    got = shim_lib.scan_like_runtime(prog(p), c.data, geo=geo, family=fam, in_mis=c.a, out_mis=c.a)
    return got, shim_lib.last_redo()


@pytest.mark.parametrize("B,geo", [(128, 2), (2048, 0)], ids=["lanes128", "lanes2048"])
@pytest.mark.parametrize("a", [0, 5])
def test_every_case_on_the_shim(B, geo, a):
    ran, left_out = 0, []
    for p in W.PROGRAMS:
        if form_of(p)[0] is None:
            left_out.append((p.pat, p.eng))
            continue
        fams = [8] + ([shim_lib.STREAM_LPW_PAIR] if p.form == "pair" else [])     # (the pair family exists for the tables that have the form)
        for c in W.cases(B, a, p.key):
            want = want_of(p, c)
            for fam in fams:
                got, redo = on_the_shim(p, c, geo, fam)
                assert got == want, (p.tag, c.name, B, a, fam, next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want))))
                assert tuple(redo) == c.redo, (p.tag, c.name, B, a, fam, redo, c.redo)
            ran += 1
    assert sorted(left_out) == sorted(W.NO_WINDOW_FORM) and ran == (len(W.PROGRAMS) - len(left_out)) * len(W.NAMES)
