"""Scans in place (d_in == d_out) against the oracle.

The C ABI lets the output buffer be the input buffer (include/trre_mi355x.h, trre_scan_device): every family and mode must
then print, byte for byte, what separate buffers give — also where a launch is void and the scan runs again (a NUL, an
overflowing fold, a mask scratch), where the output grows or shrinks, after TRRE_E_CAPACITY (the input is still there for
the retry) and over a batch of split-form enqueues.  Any other overlap is refused.  Every in-place call gets a fresh copy of
its input; every case names the family it runs, so that a change of routing cannot take it off the path it is meant for."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import golden_lib
import trre_amd
from oracle_lib import Oracle, scan_mt
from trre_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAM = {v: k for k, v in trre_amd.KERNEL_NAMES.items()}
SENTINEL = 0xA5
PAD = 4 << 20               # bytes behind the capacity the scan is given: they must come back untouched


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev())


def inplace(p, src, off, cap=None):
    """a fresh buffer of off + cap + PAD bytes holding `src` (bytes or a device tensor) at `off`; the scan in place
    (scan_tensor(t[off:off+n], out=t[off:off+cap])).  Returns (output bytes or the TrreError, the buffer)."""
    import torch
    n = len(src) if isinstance(src, (bytes, bytearray)) else src.numel()
    cap = cap if cap is not None else n + 64
    t = torch.full((off + cap + PAD,), SENTINEL, dtype=torch.uint8, device=dev())
    if n:
        t[off:off + n] = to_dev(src) if isinstance(src, (bytes, bytearray)) else src
    try:
        got = p.scan_tensor(t[off:off + n], out=t[off:off + cap]).cpu().numpy().tobytes()
    except trre_amd.TrreError as e:
        got = e
    assert bool((t[off + cap:] == SENTINEL).all()), "written beyond the capacity"
    if off:
        assert bool((t[:off] == SENTINEL).all()), "written before the output"
    return got, t


def check(p, data, want, off, what, cap=None):
    got, _ = inplace(p, data, off, cap if cap is not None else max(len(data), len(want)) + 64)
    if isinstance(got, trre_amd.TrreError):
        raise AssertionError("%r: %s" % (what, got))
    if got != want:
        i = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
        raise AssertionError("%r: %d bytes, want %d; first difference at %d" % (what, len(got), len(want), i))


def families(p):
    return [trre_amd.KERNEL_AUTO] + p.allowed_kernels()


# ---- a. the golden vectors, in place -----------------------------------------------------------------------------------

def test_golden_vectors_in_place():
    """every scan vector on both engines, AUTO and then every family the program allows, at offsets 0 and 3 of a buffer
    of max(n, len(expected)) + 64 bytes (eleven inputs hold NULs: the relaunches of a void launch at small sizes)"""
    import torch
    n_ok = n_fail = n_fam = 0
    progs = {}
    for pat, name, data, engine, exp in golden_lib.cases():
        key = (pat, engine)
        if key not in progs:
            progs[key] = trre_amd.Program(pat, engine)
        p = progs[key]
        fams = families(p)
        if exp is None:
            fams = [f for f in fams if f in (trre_amd.KERNEL_AUTO, trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_GUIDED_GEN)]
        for fam in fams:
            p.set_kernel(fam)
            for off in (0, 3):
                size = max(len(data), len(exp or b"")) + 64
                t = torch.full((off + size,), SENTINEL, dtype=torch.uint8, device=dev())
                if data:
                    t[off:off + len(data)] = to_dev(data)
                try:
                    got = p.scan_tensor(t[off:off + len(data)], out=t[off:]).cpu().numpy().tobytes()
                except trre_amd.TrreError as e:
                    got = e
                if exp is None:
                    assert isinstance(got, trre_amd.TrreError) and got.code == api.E_DIVERGES, (pat, name, engine, fam, off)
                else:
                    assert got == exp, (pat, name, engine, trre_amd.KERNEL_NAMES[fam], off)
                if off:
                    assert int(t[0]) == SENTINEL and int(t[1]) == SENTINEL and int(t[2]) == SENTINEL
        p.set_kernel(trre_amd.KERNEL_AUTO)
        if exp is None:
            n_fail += 1
        else:
            n_ok += 1
            n_fam += len(fams) - 1
    assert n_ok == 902 and n_fail == 28 and n_fam > 4900, (n_ok, n_fail, n_fam)


def test_match_and_generator_vectors_in_place():
    """`trre -m` vectors (AUTO and every family), and the generator modes' vectors (they copy their input to the host
    first), in place"""
    import torch
    n = 0
    progs = {}
    for pat, name, data, exp in golden_lib.match_cases():
        if pat not in progs:
            progs[pat] = trre_amd.Program(pat, "nft", mode="match")
        p = progs[pat]
        for fam in (families(p) if exp is not None else [trre_amd.KERNEL_AUTO]):
            p.set_kernel(fam)
            for off in (0, 3):
                got, _ = inplace(p, data, off, max(len(data), len(exp or b"")) + 64)
                if exp is None:
                    assert isinstance(got, trre_amd.TrreError) and got.code == api.E_DIVERGES, (pat, name, fam, off)
                else:
                    assert got == exp, (pat, name, trre_amd.KERNEL_NAMES[fam], off)
        p.set_kernel(trre_amd.KERNEL_AUTO)
        n += 1
    assert n > 100
    m = 0
    for pat, flags, name, data, exp, printed in golden_lib.all_cases():
        if exp is None or not data:
            continue
        p = trre_amd.Program(pat, "nft", mode="match_all" if "m" in flags else "scan_all")
        assert trre_amd.KERNEL_NAMES[p.info.kernel] == "generate"
        for off in (0, 3):
            got, _ = inplace(p, data, off, max(len(data), len(exp)) + 64)
            assert got == exp, (pat, flags, name, off)
        m += 1
    assert m >= 150
    del torch


# ---- b. slabs at real sizes --------------------------------------------------------------------------------------------

_inputs = {}


def slab(name):
    """device inputs: 64 MiB of printable lines (cfg 2), 64 MiB of the cat / dog soup (cfg 4), 8 MiB of lines of 400 KB"""
    if name not in _inputs:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import corpora
        if name == "printable":
            _inputs[name] = corpora.printable_lines(64 << 20, corpora.SEED0 + 2, dev())
        elif name == "printable8":
            _inputs[name] = corpora.printable_lines(8 << 20, corpora.SEED0 + 3, dev())
        elif name == "catdog":
            _inputs[name] = corpora.cat_dog_soup(64 << 20, corpora.SEED0 + 4, dev())
        elif name == "long":
            _inputs[name] = corpora.long_lines(8 << 20, corpora.SEED0 + 5, dev(), 400000)
    return _inputs[name]


def variants(x, which="all"):
    """(name, device tensor): no NUL; a NUL at byte 0; NULs at 16384 k - 1 and 16384 k (k_mapgen's tile edge); a NUL inside
    the longest line; a NUL on the byte before the final '\\n'; no final newline"""
    n = x.numel()
    out = [("plain", x)]
    if which == "plain":
        return out
    y = x.clone()
    y[0] = 0
    out.append(("nul0", y))
    if which == "nul":
        return out
    y = x.clone()
    for k in sorted({k for k in (1, 2, 777, n // 16384 - 1) if 0 < 16384 * k < n}):
        y[16384 * k - 1] = 0
        y[16384 * k] = 0
    out.append(("nul_tile_edge", y))
    ends = (x == 10).nonzero().flatten().cpu()
    gaps = ends[1:] - ends[:-1]
    i = int(gaps.argmax())
    y = x.clone()
    y[int(ends[i]) + int(gaps[i]) // 2] = 0
    out.append(("nul_in_longest_line", y))
    y = x.clone()
    y[n - 2] = 0
    out.append(("nul_before_last_nl", y))
    y = x.clone()
    y[n - 1] = ord("q")
    out.append(("no_final_nl", y))
    return out


# (label, pattern, engine, mode, forced family or None, the family it must run as, input, variants)
SLAB_CASES = [
    ("caesar", "[a:b-y:zz:a]", "dft", "scan", None, "bytemap", "printable", "all"),     # not idempotent: a rerun from its own output shows
    ("caesar_long", "[a:b-y:zz:a]", "dft", "scan", None, "bytemap", "long", "all"),
    ("catdog_stream_lp", "(cat:dog|dog:cat)", "nft", "scan", None, "stream_lp", "catdog", "all"),
    ("catdog_stream_lp_long", "(cat:dog|dog:cat)", "nft", "scan", None, "stream_lp", "long", "all"),
    ("guided_lp_long", "(a:x)*b", "nft", "scan", "guided_lp", "guided_lp", "long", "nul"),
    ("tile_lp_long", "(a:x)*b", "nft", "scan", "tile_lp", "tile_lp", "long", "nul"),
    ("expand", "a:xyz", "dft", "scan", None, "stream_gen", "printable", "all"),
    ("delete", "[aie]:", "nft", "scan", None, "stream_gen", "printable", "all"),
    ("html", "(<:&lt;|>:&gt;|&:&amp;)", "nft", "scan", None, "stream_gen", "printable", "nul"),
    ("ing", "[a-z]+ing:X", "dft", "scan", None, "guided_gen", "printable", "nul"),
    ("lazy", "((a:x)*b)|((a:y)*c)", "dft", "scan", None, "dft_lazy", "printable8", "nul"),
    ("lp_dft_lazy", "a(a|b|c|d|e|f|g|h){12}(c:x)", "dft", "scan", None, "dft_lazy", "printable8", "nul"),
    ("backtrack", "a(a|b|c|d|e|f|g|h){12}c:x", "nft", "scan", None, "backtrack", "printable8", "nul"),
    ("tile_gen", "(cat:dog|dog:cat)", "nft", "scan", "tile_gen", "tile_gen", "catdog", "nul"),
    ("match", "(a|b)*c", "nft", "match", None, "guided_gen", "printable8", "nul"),
]

_want = {}


def oracle_out(pat, eng, mode, data):
    key = (pat, eng, mode, hash(data), len(data))
    if key not in _want:
        _want[key] = Oracle(pat, eng).match(data) if mode == "match" else scan_mt(pat, eng, 16, data)
    return _want[key]


@pytest.mark.parametrize("case", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_slabs_in_place(case):
    label, pat, eng, mode, forced, runs, inp, which = case
    p = trre_amd.Program(pat, eng, mode=mode)
    if forced is None:
        assert trre_amd.KERNEL_NAMES[p.info.kernel] == runs, (label, trre_amd.KERNEL_NAMES[p.info.kernel])
    else:
        assert FAM[forced] in p.allowed_kernels(), label
        p.set_kernel(FAM[forced])
    if label == "lp_dft_lazy":
        assert p.info.flags & trre_amd.api.FLAG_LENGTH_PRESERVING        # AUTO sends this length-preserving pattern to the lazy family
    for vname, x in variants(slab(inp), which):
        data = x.cpu().numpy().tobytes()
        want = oracle_out(pat, eng, mode, data)
        for off in (0, 5):
            check(p, x, want, off, (label, vname, off))


MAPGEN_SCRIPT = r'''
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, trre_amd
from oracle_lib import scan_mt
import test_gpu_inplace as T
res = {}
for pat, eng in (("a:xyz", "dft"), ("[aie]:", "nft")):
    p = trre_amd.Program(pat, eng)
    assert trre_amd.KERNEL_NAMES[p.info.kernel] == "stream_gen"
    for vname, x in T.variants(T.slab("printable")):
        want = scan_mt(pat, eng, 16, x.cpu().numpy().tobytes())
        for off in (0, 5):
            try:
                T.check(p, x, want, off, (pat, vname, off))
                res["%%s %%s %%d" %% (pat, vname, off)] = "ok"
            except AssertionError as e:
                res["%%s %%s %%d" %% (pat, vname, off)] = str(e)
print("RESULT " + json.dumps(res))
'''


def test_memoryless_expansions_in_place_through_the_pair():
    """'a:xyz' and '[aie]:' in place through the count / emit pair (TRRE_MAPGEN=0: not the memoryless one-pass kernel, which
    test_slabs_in_place runs by default), in a child process of its own"""
    e = dict(os.environ)
    e["TRRE_MAPGEN"] = "0"
    r = subprocess.run([sys.executable, "-c", MAPGEN_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=e, timeout=900)
    assert r.returncode == 0, r.stderr.decode("latin-1")[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    assert len(res) == 24 and all(v == "ok" for v in res.values()), {k: v for k, v in res.items() if v != "ok"}


# ---- c. TRRE_E_CAPACITY in place ---------------------------------------------------------------------------------------

def test_capacity_in_place_leaves_the_input():
    """'a:xyz' in place with one byte too few: TRRE_E_CAPACITY with the size needed, the input still in the first n bytes —
    and scan_tensor's retry (a fresh output) from the same buffer prints the oracle's bytes"""
    import torch
    data = slab("printable8")[:3 << 20].cpu().numpy().tobytes()
    want = scan_mt("a:xyz", "dft", 16, data)
    n, need = len(data), len(want)
    assert need > n + 1000
    p = trre_amd.Program("a:xyz", "dft")
    for fam in families(p):
        p.set_kernel(fam)
        t = torch.full((need - 1 + PAD,), SENTINEL, dtype=torch.uint8, device=dev())
        t[:n] = to_dev(data)
        m = ctypes.c_size_t()
        s = torch.cuda.current_stream().cuda_stream
        rc = api.lib().trre_scan_device(p._h, t.data_ptr(), n, t.data_ptr(), need - 1, ctypes.byref(m), s)
        torch.cuda.synchronize()
        assert rc == api.E_CAPACITY and m.value == need, (trre_amd.KERNEL_NAMES[fam], rc, m.value)
        assert t[:n].cpu().numpy().tobytes() == data, trre_amd.KERNEL_NAMES[fam]
        assert bool((t[need - 1:] == SENTINEL).all()), trre_amd.KERNEL_NAMES[fam]
        small = torch.empty(16, dtype=torch.uint8, device=dev())
        assert p.scan_tensor(t[:n], out=small).cpu().numpy().tobytes() == want, trre_amd.KERNEL_NAMES[fam]
        # the idiom itself: in place first, room asked for, the retry reads the buffer again
        t[:n] = to_dev(data)
        assert p.scan_tensor(t[:n], out=t[:need - 1]).cpu().numpy().tobytes() == want, trre_amd.KERNEL_NAMES[fam]
    p.set_kernel(trre_amd.KERNEL_AUTO)


# ---- d. the split form -------------------------------------------------------------------------------------------------

def test_split_form_in_place():
    """an aliased enqueue + finish; then several enqueues of the same aliased scan before one finish (a benchmark loop):
    every launch reads the input as it was at the first enqueue"""
    import torch
    data = slab("printable8").cpu().numpy().tobytes()
    for pat, eng in (("[a:b-y:zz:a]", "dft"), ("a:xyz", "dft"), ("(cat:dog|dog:cat)", "nft"), ("[aie]:", "nft")):
        want = scan_mt(pat, eng, 16, data)
        p = trre_amd.Program(pat, eng)
        cap = max(len(data), len(want)) + 64
        for reps in (1, 3):
            for off in (0, 5):
                t = torch.full((off + cap + PAD,), SENTINEL, dtype=torch.uint8, device=dev())
                t[off:off + len(data)] = to_dev(data)
                for _ in range(reps):
                    p.enqueue(t[off:off + len(data)], t[off:off + cap])
                m = p.finish()
                torch.cuda.synchronize()
                assert t[off:off + m].cpu().numpy().tobytes() == want, (pat, reps, off)
                assert bool((t[off + cap:] == SENTINEL).all()), (pat, reps, off)


# ---- e. partial overlap ------------------------------------------------------------------------------------------------

def test_partial_overlap_is_refused_on_the_device():
    """d_out = d_in +- {1, 15, 16, 4096}, and d_out + cap == d_in + 1: TRRE_E_ARG from trre_scan_device and trre_scan_enqueue,
    nothing written"""
    import torch
    n = 16384
    data = slab("printable8")[:n].cpu().numpy().tobytes()
    base = 3 * n
    t = torch.full((7 * n,), SENTINEL, dtype=torch.uint8, device=dev())
    t[base:base + n] = to_dev(data)
    before = t.cpu().numpy().tobytes()
    s = torch.cuda.current_stream().cuda_stream
    m = ctypes.c_size_t()
    for pat, eng in (("[a:b-y:zz:a]", "dft"), ("a:xyz", "dft"), ("(cat:dog|dog:cat)", "nft")):
        p = trre_amd.Program(pat, eng)
        d_in = t.data_ptr() + base
        for d_out, cap in [(d_in + d, n) for d in (1, 15, 16, 4096, -1, -15, -16, -4096)] + [(d_in + 1 - n, n), (d_in + 1 - 64, 64)]:
            assert api.lib().trre_scan_device(p._h, d_in, n, d_out, cap, ctypes.byref(m), s) == api.E_ARG, (pat, d_out - d_in, cap)
            assert api.lib().trre_scan_enqueue(p._h, d_in, n, d_out, cap, s) == api.E_ARG, (pat, d_out - d_in, cap)
        torch.cuda.synchronize()
        assert t.cpu().numpy().tobytes() == before, pat
        # the neighbours that do not overlap are scans like any other
        assert p.scan_tensor(t[base:base + n], out=t[base + n:base + 3 * n]).cpu().numpy().tobytes() == scan_mt(pat, eng, 1, data)
        t[base + n:] = SENTINEL
