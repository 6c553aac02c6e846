"""Packed strings on the GPU (include/trre_mi355x.h: trre_scan_device_strings; Program.scan_strings / map_strings) against the
oracle: string i is the content of one line, its output is R(string_i + b"\\n") without the last byte, out_offsets[i] where it
starts."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import golden_lib
import trre_amd
from gpu_column_lib import dev, off_dev, pack, to_dev
from oracle_lib import Oracle, OracleError, scan_mt
from trre_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SENTINEL = 0xA5
THREADS = 16


def run(p, values, offsets):
    out, oo = p.scan_strings(values, offsets)
    return out.cpu().numpy().tobytes(), oo.cpu().numpy().tolist()


def expect(o, recs):
    """the specification: the oracle on each string as one line, the framing newline dropped; the deterministic engine's
    tables grow with what it has seen, so every string gets a fresh one there, as a fresh process of the reference would"""
    fresh = o.engine == 1
    return pack([(Oracle(o.pattern, "dft") if fresh else o).scan(r + b"\n")[:-1] for r in recs])


def random_offsets(rng, data):
    n = len(data)
    cuts = [rng.randrange(n + 1) for _ in range(rng.randrange(0, 12))]
    nls = [i + 1 for i, c in enumerate(data) if c == 10]
    if nls:
        cuts += rng.sample(nls, min(len(nls), rng.randrange(0, 4)))
    if cuts and rng.random() < 0.4:
        cuts += [rng.choice(cuts)] * 2
    return [0] + sorted(cuts) + [n]


def test_golden_vectors_every_family():
    """every golden scan vector cut into strings, AUTO and every family the program allows: bytes and offsets equal the
    per-string oracle; a string the reference does not survive gives TRRE_E_DIVERGES with out_len = 0; a program that prints
    a '\\n' of its own is refused"""
    rng = random.Random(707)
    n_cases = compared = diverged = newline_printing = n_fam = 0
    progs = {}
    for pat, name, data, engine, exp in golden_lib.cases():
        n_cases += 1
        key = (pat, engine)
        if key not in progs:
            progs[key] = (trre_amd.Program(pat, engine), Oracle(pat, engine))
        p, o = progs[key]
        off = random_offsets(rng, data)
        recs = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        values, offsets = to_dev(data), off_dev(off)
        try:
            want = expect(o, recs)
        except OracleError:
            want = None
        refused = False
        for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
            if want is None and fam not in (trre_amd.KERNEL_AUTO, trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_GUIDED_GEN):
                continue
            p.set_kernel(fam)
            try:
                got = run(p, values, offsets)
            except trre_amd.TrreError as e:
                if e.code == api.E_UNSUPPORTED and "newline" in e.message:
                    refused = True
                    break
                assert want is None and e.code == api.E_DIVERGES and e.partial is None, (pat, name, engine, trre_amd.KERNEL_NAMES[fam], e)
                continue
            assert want is not None, (pat, name, engine, trre_amd.KERNEL_NAMES[fam], "diverges in the reference")
            assert got[0] == want[0], (pat, name, engine, trre_amd.KERNEL_NAMES[fam], off)
            assert got[1] == want[1], (pat, name, engine, trre_amd.KERNEL_NAMES[fam], off)
            n_fam += fam != trre_amd.KERNEL_AUTO
        p.set_kernel(trre_amd.KERNEL_AUTO)
        if refused:
            newline_printing += 1
        elif want is None:
            # through the C ABI: out_len is 0 on TRRE_E_DIVERGES
            import torch
            out = torch.empty(len(data) + 4096, dtype=torch.uint8, device=dev())
            oo = torch.empty(len(off), dtype=torch.int64, device=dev())
            m = ctypes.c_size_t(77)
            rc = api.lib().trre_scan_device_strings(p._h, values.data_ptr(), len(data), offsets.data_ptr(), len(off) - 1, out.data_ptr(),
                                                     out.numel(), oo.data_ptr(), ctypes.byref(m), None)
            assert rc == api.E_DIVERGES and m.value == 0, (pat, name, engine, rc, m.value)
            diverged += 1
        else:
            compared += 1
    assert compared + diverged + newline_printing == n_cases == 930, (compared, diverged, newline_printing, n_cases)
    assert compared > 700 and n_fam > 4000 and diverged > 0, (compared, n_fam, diverged, newline_printing)


def test_one_string_per_line_equals_scan_tensor():
    """one string per line of a 300 KB text: the bytes of scan_tensor of the text without its newlines, the output offsets its
    newline positions minus the index"""
    rng = random.Random(1)
    data = bytes(rng.choice(b"the cat sat on a dog\n\0") for _ in range(300000)) + b"\n"
    arr = np.frombuffer(data, dtype=np.uint8)
    nls = np.flatnonzero(arr == 10)
    off = np.concatenate([[0], nls + 1 - np.arange(1, len(nls) + 1)])
    values = to_dev(arr[arr != 10].tobytes())
    for pat, eng in (("[a:A-z:Z]", "dft"), ("(cat:dog|dog:cat)", "nft"), ("a:xyz", "dft"), ("[aie]:", "nft")):
        p = trre_amd.Program(pat, eng)
        got, oo = run(p, values, off_dev(off))
        want = np.frombuffer(p.scan_tensor(to_dev(data)).cpu().numpy().tobytes(), dtype=np.uint8)
        assert got == want[want != 10].tobytes(), pat
        onl = np.flatnonzero(want == 10)
        assert oo == [0] + (onl - np.arange(len(onl))).tolist(), pat


def test_in_place_and_capacity():
    """out = values (at offsets 0 and 5 of a buffer): equal to separate buffers, sentinels intact; cap = 0 and cap = needed - 1
    give E_CAPACITY with the exact unframed size and touch neither the input nor the sentinels; the retry with room works"""
    import torch
    rng = random.Random(2)
    data = bytes(rng.choice(b"abcxyz \n") for _ in range(100000))
    off = sorted(rng.randrange(len(data) + 1) for _ in range(300))
    off = [0] + off + [len(data)]
    recs = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    f = api.lib().trre_scan_device_strings
    for pat, eng in (("a:xyz", "dft"), ("[aie]:", "nft"), ("[a:A-z:Z]", "dft"), ("(cat:dog|dog:cat)", "nft")):
        p = trre_amd.Program(pat, eng)
        want = expect(Oracle(pat, eng), recs)
        need = len(want[0])
        for base in (0, 5):
            cap = max(len(data), need) + 64
            t = torch.full((base + cap + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
            t[base:base + len(data)] = to_dev(data)
            v = t[base:base + len(data)]
            out, oo = p.scan_strings(v, off_dev(off), out=t[base:base + cap])
            assert out.data_ptr() == v.data_ptr()
            assert out.cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1], (pat, base)
            assert bool((t[base + max(need, len(data)):] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())
            # the capacity query, in place: nothing of the caller's data is written
            for small in (0, need - 1):
                t = torch.full((base + cap + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
                t[base:base + len(data)] = to_dev(data)
                offs, oo = off_dev(off), torch.full((len(off),), -7, dtype=torch.int64, device=dev())
                m = ctypes.c_size_t()
                args = (p._h, t.data_ptr() + base, len(data), offs.data_ptr(), len(off) - 1, t.data_ptr() + base)
                if small < len(data):
                    # (in place the buffer is at least the input: a smaller cap is asked for with separate buffers)
                    o2 = torch.full((small + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
                    rc = f(*args[:5], o2.data_ptr(), small, oo.data_ptr(), ctypes.byref(m), None)
                    assert bool((o2 == SENTINEL).all()), (pat, small)
                else:
                    rc = f(*args, small, oo.data_ptr(), ctypes.byref(m), None)
                assert rc == api.E_CAPACITY and m.value == need, (pat, base, small, rc, m.value)
                assert t[base:base + len(data)].cpu().numpy().tobytes() == data, pat
                assert bool((t[base + len(data):] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())
                rc = f(*args, cap, oo.data_ptr(), ctypes.byref(m), None)
                assert rc == 0 and m.value == need, (pat, rc)
                assert t[base:base + need].cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1], pat
                assert bool((t[base + max(need, len(data)):] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())


def test_bad_offsets_touch_nothing():
    import torch
    p = trre_amd.Program("[a:A-z:Z]", "dft")
    data = b"hello\nworld\n" * 100
    x = to_dev(data)
    n = len(data)
    for off in ([1, n], [0, n - 1], [0, 50, 40, n], [0, n + 1, n], [-1, 0, n], [0, 10, 10, 9, n]):
        out = torch.full((2 * n,), SENTINEL, dtype=torch.uint8, device=dev())
        oo = torch.full((len(off),), -5, dtype=torch.int64, device=dev())
        offs = off_dev(off)
        m = ctypes.c_size_t(77)
        rc = api.lib().trre_scan_device_strings(p._h, x.data_ptr(), n, offs.data_ptr(), len(off) - 1, out.data_ptr(), out.numel(),
                                                 oo.data_ptr(), ctypes.byref(m), None)
        assert rc == api.E_ARG and m.value == 0, off
        assert bool((out == SENTINEL).all()) and bool((oo == -5).all()), off


def test_map_strings_literals_and_empty_inputs():
    import torch
    p = trre_amd.Program("[a:A-z:Z]", "dft")
    assert p.map_strings([b"", b"cat", b"a\nb", b"a\0b"]) == [b"", b"CAT", b"A\nB", b"A"]
    assert p.scan_list([b"cat"]) == [b"CA\n"]                     # (the records call keeps the reference's file framing)
    assert p.map_strings([]) == []
    e = torch.empty(0, dtype=torch.uint8, device=dev())
    out, oo = p.scan_strings(e, off_dev([0]))
    assert out.numel() == 0 and oo.cpu().tolist() == [0]
    out, oo = p.scan_strings(e, off_dev([0, 0, 0, 0]))
    assert out.numel() == 0 and oo.cpu().tolist() == [0, 0, 0, 0]


def test_empty_line_output_is_seen():
    """':x' under the non-deterministic engine prints x for every line, the empty one too: an empty string has a non-empty
    output.  The reference's deterministic engine prints nothing for an empty line, whatever the program (':x' gives b"\\n" for
    b"\\n" and b"ab\\n" for b"ab\\n" there), so for it the same strings are held against the oracle's empty outputs"""
    for eng in ("nft", "dft"):
        p = trre_amd.Program(":x", eng)
        want = [Oracle(":x", eng).scan(r + b"\n")[:-1] for r in (b"", b"ab", b"")]
        assert want == ([b"x", b"xaxbx", b"x"] if eng == "nft" else [b"", b"ab", b""])
        assert p.map_strings([b"", b"ab", b""]) == want
        import torch
        out, oo = p.scan_strings(torch.empty(0, dtype=torch.uint8, device=dev()), off_dev([0] * 1001))
        assert out.cpu().numpy().tobytes() == want[0] * 1000 and oo.cpu().tolist() == [len(want[0]) * i for i in range(1001)]


def test_million_one_byte_strings():
    import torch
    rng = np.random.default_rng(3)
    n = 1 << 20
    data = rng.choice(np.frombuffer(b"ab\n\0z", dtype=np.uint8), n).astype(np.uint8)
    x = torch.from_numpy(data).to(dev())
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev())
    table = {"[a:A-z:Z]": {97: b"A", 98: b"B", 10: b"\n", 0: b"", 122: b"Z"},
             "a:xyz": {97: b"xyz", 98: b"b", 10: b"\n", 0: b"", 122: b"z"},
             "(cat:dog|dog:cat)": {97: b"a", 98: b"b", 10: b"\n", 0: b"", 122: b"z"}}
    for pat, eng in (("[a:A-z:Z]", "dft"), ("a:xyz", "dft"), ("(cat:dog|dog:cat)", "nft")):
        for c, w in table[pat].items():                          # (the table is the oracle's)
            assert Oracle(pat, eng).scan(bytes([c]) + b"\n")[:-1] == w, (pat, c)
        lens = np.zeros(256, np.int64)
        for c, w in table[pat].items():
            lens[c] = len(w)
        out, oo = trre_amd.Program(pat, eng).scan_strings(x, offs)
        assert out.cpu().numpy().tobytes() == b"".join(table[pat][c] for c in data.tolist()), pat
        assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], np.cumsum(lens[data])])), pat


def test_one_gib_strings():
    """1 GiB of the dictionary corpus, one string per line, the line ends stripped on the device, against the 16-thread oracle"""
    import dictgen
    import torch
    keys, vals = dictgen.make_dictionary(1000)
    data = dictgen.corpus_fast(keys, 1 << 30, seed=9)
    data = data[:data.rfind(b"\n") + 1]
    x = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev())
    nl = x == 10
    ends = torch.nonzero(nl).flatten()
    offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev()), ends + 1 - torch.arange(1, ends.numel() + 1, device=dev())])
    values = x[~nl]
    del x, nl, ends
    for pat, eng in (("[a:A-z:Z]", "dft"), ("a:xyz", "dft"), ("[aie]:", "nft"), (dictgen.pattern(keys, vals), "dft")):
        want = np.frombuffer(scan_mt(pat, eng, THREADS, data), dtype=np.uint8)
        onl = np.flatnonzero(want == 10)
        out, oo = trre_amd.Program(pat, eng).scan_strings(values, offs)
        assert out.numel() == len(want) - len(onl), pat[:20]
        assert np.array_equal(out.cpu().numpy(), want[want != 10]), pat[:20]
        assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], onl - np.arange(len(onl))])), pat[:20]
        del out, oo, want, onl
        torch.cuda.empty_cache()
