"""Ragged records on the GPU (include/trre_mi355x.h: trre_scan_device_records; Program.scan_records / scan_list) against the
oracle: record i's output is what the reference prints for record i alone, out_offsets[i] where it starts."""
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
    out, oo = p.scan_records(values, offsets)
    return out.cpu().numpy().tobytes(), oo.cpu().numpy().tolist()


def expect(o, recs):
    """the oracle on each record alone; the deterministic engine's tables grow with what it has seen (an epsilon cycle met
    or not), so every record gets a fresh one there, as a fresh process of the reference would"""
    fresh = o.engine == 1
    outs = [(Oracle(o.pattern, "dft") if fresh else o).scan(r) for r in recs]
    return pack(outs)


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
    """every golden scan vector cut at random points, AUTO and every family the program allows: bytes and offsets equal the
    per-record oracle; a record the reference does not survive gives TRRE_E_DIVERGES; a program that prints a '\\n' of its
    own is refused"""
    rng = random.Random(606)
    n_ok = n_fam = n_div = n_refused = 0
    progs = {}
    for pat, name, data, engine, exp in golden_lib.cases():
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
        for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
            if want is None and fam not in (trre_amd.KERNEL_AUTO, trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_GUIDED_GEN):
                continue
            p.set_kernel(fam)
            try:
                got = run(p, values, offsets)
            except trre_amd.TrreError as e:
                if e.code == api.E_UNSUPPORTED and "newline" in e.message:
                    n_refused += 1
                    break
                assert want is None and e.code == api.E_DIVERGES, (pat, name, engine, trre_amd.KERNEL_NAMES[fam], e)
                n_div += 1
                continue
            assert want is not None, (pat, name, engine, trre_amd.KERNEL_NAMES[fam], "diverges in the reference")
            assert got[0] == want[0], (pat, name, engine, trre_amd.KERNEL_NAMES[fam], off)
            assert got[1] == want[1], (pat, name, engine, trre_amd.KERNEL_NAMES[fam], off)
            n_fam += fam != trre_amd.KERNEL_AUTO
        p.set_kernel(trre_amd.KERNEL_AUTO)
        n_ok += 1
    assert n_ok == 930 and n_fam > 4000 and n_div > 0, (n_ok, n_fam, n_div, n_refused)


def test_records_equal_lines_same_bytes_as_scan_tensor():
    rng = random.Random(1)
    data = bytes(rng.choice(b"the cat sat on a dog\n\0") for _ in range(300000)) + b"\n"
    nls = [i + 1 for i, c in enumerate(data) if c == 10]
    for pat, eng in (("[a:A-z:Z]", "dft"), ("(cat:dog|dog:cat)", "nft"), ("a:xyz", "dft"), ("[aie]:", "nft")):
        p = trre_amd.Program(pat, eng)
        x = to_dev(data)
        got, oo = run(p, x, off_dev([0] + nls))
        want = p.scan_tensor(x).cpu().numpy().tobytes()
        assert got == want, pat
        onl = [i + 1 for i, c in enumerate(want) if c == 10]
        assert oo == [0] + onl, pat


def test_in_place_and_capacity_retry():
    """out = values (at offsets 0 and 5 of a buffer): equal to separate buffers; a capacity too small gives E_CAPACITY with
    the size needed and the input back in place, and the retry with room works"""
    import torch
    rng = random.Random(2)
    data = bytes(rng.choice(b"abcxyz \n") for _ in range(100000))
    off = sorted(rng.randrange(len(data) + 1) for _ in range(300))
    off = [0] + off + [len(data)]
    recs = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    for pat, eng in (("a:xyz", "dft"), ("[aie]:", "nft"), ("[a:A-z:Z]", "dft"), ("(cat:dog|dog:cat)", "nft")):
        p = trre_amd.Program(pat, eng)
        want = expect(Oracle(pat, eng), recs)
        for base in (0, 5):
            cap = max(len(data), len(want[0])) + 64
            t = torch.full((base + cap + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
            t[base:base + len(data)] = to_dev(data)
            v = t[base:base + len(data)]
            out, oo = p.scan_records(v, off_dev(off), out=t[base:base + cap])
            assert out.data_ptr() == v.data_ptr()
            assert out.cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1], (pat, base)
            assert bool((t[base + cap:] == SENTINEL).all()) and bool((t[:base] == SENTINEL).all())
        if len(want[0]) <= len(data):
            continue
        # capacity: in place with cap = n, through the C ABI
        t = torch.full((len(data) + 4096,), SENTINEL, dtype=torch.uint8, device=dev())
        t[:len(data)] = to_dev(data)
        offs, oo = off_dev(off), torch.full((len(off),), -7, dtype=torch.int64, device=dev())
        m = ctypes.c_size_t()
        args = (p._h, t.data_ptr(), len(data), offs.data_ptr(), len(off) - 1)
        rc = api.lib().trre_scan_device_records(*args, t.data_ptr(), len(data), oo.data_ptr(), ctypes.byref(m), None)
        assert rc == api.E_CAPACITY and m.value == len(want[0]), (pat, rc, m.value)
        assert t[:len(data)].cpu().numpy().tobytes() == data, pat
        assert bool((t[len(data):] == SENTINEL).all())
        big = torch.empty(m.value + 4096, dtype=torch.uint8, device=dev())
        big[:len(data)] = t[:len(data)]
        rc = api.lib().trre_scan_device_records(p._h, big.data_ptr(), len(data), offs.data_ptr(), len(off) - 1, big.data_ptr(),
                                                 big.numel(), oo.data_ptr(), ctypes.byref(m), None)
        assert rc == 0 and big[:m.value].cpu().numpy().tobytes() == want[0] and oo.cpu().numpy().tolist() == want[1], pat
        # separate buffers: the size query and the retry with the same arguments but room
        out = torch.empty(16, dtype=torch.uint8, device=dev())
        rc = api.lib().trre_scan_device_records(*args, out.data_ptr(), 16, oo.data_ptr(), ctypes.byref(m), None)
        assert rc == api.E_CAPACITY and m.value == len(want[0])


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
        rc = api.lib().trre_scan_device_records(p._h, x.data_ptr(), n, offs.data_ptr(), len(off) - 1, out.data_ptr(), out.numel(),
                                                 oo.data_ptr(), ctypes.byref(m), None)
        assert rc == api.E_ARG, off
        assert bool((out == SENTINEL).all()) and bool((oo == -5).all()), off


def test_empty_inputs():
    import torch
    p = trre_amd.Program("[a:A-z:Z]", "dft")
    e = torch.empty(0, dtype=torch.uint8, device=dev())
    out, oo = p.scan_records(e, off_dev([0]))
    assert out.numel() == 0 and oo.cpu().tolist() == [0]
    out, oo = p.scan_records(e, off_dev([0, 0, 0, 0]))
    assert out.numel() == 0 and oo.cpu().tolist() == [0, 0, 0, 0]
    assert p.scan_list([]) == []
    assert p.scan_list([b"", b"abc", b"", b"x\ny", b"q\n", b"a\0b\n"]) == [b"", b"AB\n", b"", b"X\n\n", b"Q\n", b"A\n"]


def test_million_one_byte_records():
    rng = np.random.default_rng(3)
    n = 1 << 20
    data = rng.choice(np.frombuffer(b"ab\n\0z", dtype=np.uint8), n).astype(np.uint8)
    import torch
    x = torch.from_numpy(data).to(dev())
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev())
    for pat, eng in (("[a:A-z:Z]", "dft"), ("a:xyz", "dft"), ("(cat:dog|dog:cat)", "nft")):
        out, oo = trre_amd.Program(pat, eng).scan_records(x, offs)
        assert out.cpu().numpy().tobytes() == b"\n" * n, pat       # a one-byte record is an empty line
        assert bool((oo == offs).all()), pat


def corpus_1g():
    import dictgen
    keys, vals = dictgen.make_dictionary(1000)
    data = dictgen.corpus_fast(keys, 1 << 30, seed=9)
    return data, dictgen.pattern(keys, vals)


def test_one_gib_records():
    """1 GiB in 3 records (cut inside lines) and in one record per line, against the 16-thread oracle"""
    import torch
    data, dict_pat = corpus_1g()
    n = len(data)
    arr = np.frombuffer(data, dtype=np.uint8)
    nls = np.flatnonzero(arr == 10) + 1
    x = torch.from_numpy(arr.copy()).to(dev())
    cuts = [0, n // 3 + 17, 2 * n // 3 + 5, n]
    recs3 = [data[cuts[i]:cuts[i + 1]] for i in range(3)]
    for pat, eng in (("[a:A-z:Z]", "dft"), ("a:xyz", "dft"), ("[aie]:", "nft"), (dict_pat, "dft")):
        p = trre_amd.Program(pat, eng)
        # one record per line: the scan's output, cut at its newlines
        want = scan_mt(pat, eng, THREADS, data)
        out, oo = p.scan_records(x, torch.from_numpy(np.concatenate([[0], nls]).astype(np.int64)).to(dev()))
        assert out.numel() == len(want) and out.cpu().numpy().tobytes() == want, pat[:20]
        onl = np.flatnonzero(np.frombuffer(want, dtype=np.uint8) == 10) + 1
        assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], onl])), pat[:20]
        del out, oo, want
        # three records
        parts = [scan_mt(pat, eng, THREADS, r) for r in recs3]
        out, oo = p.scan_records(x, off_dev(cuts))
        assert out.cpu().numpy().tobytes() == b"".join(parts), pat[:20]
        assert oo.cpu().tolist() == [0, len(parts[0]), len(parts[0]) + len(parts[1]), sum(map(len, parts))], pat[:20]
        del out, oo, parts
        torch.cuda.empty_cache()


def test_diverging_record():
    """' +: ' on a run of 70 000 spaces in record 2: E_DIVERGES with records 0-1 and the reference's partial line"""
    recs = [b"a  b   c\n", b"x  y", b"p q " + b" " * 70000 + b"z\n", b"after  it\n"]
    o = Oracle(" +: ", "nft")
    head = o.scan(recs[0]) + o.scan(recs[1])
    with pytest.raises(OracleError) as ei:
        o.scan(recs[2])
    data, off = pack(recs)
    p = trre_amd.Program(" +: ", "nft")
    with pytest.raises(trre_amd.TrreError) as ej:
        p.scan_records(to_dev(data), off_dev(off))
    assert ej.value.code == api.E_DIVERGES
    assert ej.value.partial.cpu().numpy().tobytes() == head + ei.value.partial
