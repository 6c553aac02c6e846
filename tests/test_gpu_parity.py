"""GPU parity tests proper: the HIP path, called through the C ABI, against the
golden vectors (outputs of the compiled reference), the oracle and — when the
prebuilt binaries travelled along — the reference itself.  Bit-exact: this is
byte/integer work, the tolerance is zero."""
import random

import pytest

import corpus
import golden_lib
import trre_amd
from conftest import have_gpu
from oracle_lib import Oracle, ref_available, ref_scan

pytestmark = pytest.mark.gpu

_progs = {}


def prog(pat, eng):
    key = (pat, eng)
    if key not in _progs:
        try:
            _progs[key] = trre_amd.Program(pat, eng)
        except trre_amd.TrreError as e:
            _progs[key] = e
    return _progs[key]


def gpu_scan(p, data, family=None):
    import torch
    p.set_kernel(family or trre_amd.KERNEL_AUTO)
    try:
        if not data:
            return p.scan(data)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        return p.scan_tensor(t).cpu().numpy().tobytes()
    finally:
        p.set_kernel(trre_amd.KERNEL_AUTO)


def test_gpu_present_and_native_library_loaded():
    import torch
    assert have_gpu(), "the -m gpu tier needs a GPU"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    assert trre_amd.api.lib() is not None
    with open("/proc/self/maps") as f:
        assert "libtrre_mi355x.so" in f.read()


# golden (pattern, engine) pairs the product may refuse: none.  All 912 vectors generated from the compiled
# reference run on the GPU (round 1 refused 60 of its 870: NFT patterns with '.' or wide ranges); 18 of them are
# runs on which the reference itself exits 1 (an epsilon cycle entered) and the scan reports TRRE_E_DIVERGES.
REFUSED_GOLDEN = set()


def test_golden_vectors_on_gpu():
    n = n_fail = 0
    n_guided = {"nft": 0, "dft": 0}
    guided = (trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_GUIDED_GEN)
    for pat, name, data, engine, exp in golden_lib.cases():
        p = prog(pat, engine)
        if isinstance(p, trre_amd.TrreError):
            assert (pat, engine) in REFUSED_GOLDEN, (pat, engine, p)
            continue
        if exp is None:                     # the reference exits 1 here (epsilon cycle entered): so must the scan
            for fam in [None] + [f for f in guided if f in allowed(p)]:
                with pytest.raises(trre_amd.TrreError) as e:
                    gpu_scan(p, data, fam)
                assert e.value.code == trre_amd.api.E_DIVERGES, (pat, name, engine, fam)
            n_fail += 1
            continue
        assert gpu_scan(p, data) == exp, (pat, name, engine)
        n += 1
        # the guided families run every NFT pattern and (round 4) every DFT pattern that is not a byte map: check them
        # too, not only where AUTO picks them
        for fam in guided:
            if fam in allowed(p):
                assert gpu_scan(p, data, fam) == exp, (pat, name, engine, fam)
                n_guided[engine] += 1
    assert n == 902 and n_fail == 28 and n_guided["nft"] > 500 and n_guided["dft"] > 350, (n, n_fail, n_guided)


_allowed = {}


def allowed(p):
    if id(p) not in _allowed:
        _allowed[id(p)] = p.allowed_kernels()
    return _allowed[id(p)]


def test_reference_scan_rows_with_dot_on_gpu():
    """test.sh:114,115,129-132 (expected outputs from the reference's own test table) with the NFT engine"""
    for pat, data, want in [("(.:x)*.*", b"abc\n", b"xxx\n"), ("(.:x)*?.*", b"abc\n", b"abc\n"), ("<(.:)*>", b"<abc>\n", b"<>\n"),
                            ("<(.:)*?>", b"<abc>\n", b"<>\n"), ("<(.:)+>", b"<abc>\n", b"<>\n"), ("<(.:)+?>", b"<abc>\n", b"<>\n")]:
        p = prog(pat, "nft")
        assert Oracle(pat, "nft").scan(data) == want
        for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
            assert gpu_scan(p, data, fam) == want, (pat, fam)
            assert gpu_scan(p, data * 5000, fam) == want * 5000, (pat, fam)


def test_epsilon_cycle_reports_diverges_on_gpu():
    """'a:*' on a line with an 'a': the reference exits 1 with 'stack max capacity reached'"""
    p = prog("a:*", "nft")
    assert gpu_scan(p, b"b\nccc\n") == b"b\nccc\n"
    with pytest.raises(trre_amd.TrreError) as e:
        gpu_scan(p, b"b\nca\n")
    assert e.value.code == trre_amd.api.E_DIVERGES


def test_divergence_leaves_what_the_reference_had_printed():
    """NFT engine: the reference exits 1 with the lines before the bad one and the bad line's output up to the failing
    attempt on stdout (exit() flushes).  The scan returns TRRE_E_DIVERGES with exactly those bytes: golden vectors, every
    family that runs the pattern, device and host paths, and a bad line deep inside a large buffer (many lanes and
    chunks before it, more bad lines after it)."""
    n = 0
    for pat, name, data, printed in golden_lib.fail_cases():
        p = prog(pat, "nft")
        for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
            with pytest.raises(trre_amd.TrreError) as e:
                gpu_scan(p, data, fam)
            assert e.value.code == trre_amd.api.E_DIVERGES
            assert e.value.partial.cpu().numpy().tobytes() == printed, (pat, name, fam)
        with pytest.raises(trre_amd.TrreError) as e:
            p.scan(data)
        assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial == printed, (pat, name, "host")
        n += 1
    assert n >= 13
    rng = random.Random(77)
    head = corpus.word_soup(rng, 3 << 20).replace(b"a", b"e")          # no 'a': 'a:*' never enters its cycle here
    bad = b"cat dog cat xyz cat a cat\n"
    data = head + bad + corpus.word_soup(rng, 1 << 20) + bad
    for pat in ("cat:dog|a:*", "cat:doggy|a(:y)*"):
        want = Oracle(pat, "nft").scan(head) + Oracle(pat, "nft").scan(b"cat dog cat xyz cat \n")[:-1]
        p = prog(pat, "nft")
        with pytest.raises(trre_amd.TrreError) as e:
            gpu_scan(p, data)
        assert e.value.partial.cpu().numpy().tobytes() == want, pat
        o_head = Oracle(pat, "nft").scan(head)
        for kw in ({}, {"device_mask": 0}):
            with pytest.raises(trre_amd.TrreError) as e:
                p.scan(data * 12, **kw)                                    # ~50 MiB: the bad line sits in the first chunk of several
            assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial == want, (pat, kw)
            with pytest.raises(trre_amd.TrreError) as e:
                p.scan(head * 11 + data, **kw)                             # ... and in the second chunk (33 MiB of clean lines first)
            assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial == o_head * 11 + want, (pat, kw, "second chunk")


def test_stack_limit_of_the_reference_search():
    """The reference's backtracking stack holds at most 65 536 live alternatives (trre_nft.c:35-36,548-556): a greedy loop over a
    run of 65 536 bytes exits 1 ("stack max capacity reached") with what it had printed, although the search would succeed.
    Rounds 1-3 printed the match (a documented deviation); the stack guard (guard_block.hpp) finds the lines long enough for
    that, runs the reference's search on them and answers like the reference: every family, device and host buffers, in place."""
    import torch
    from oracle_lib import OracleError
    for pat, run, close in [(" +: ", b" ", b"y"), ("(a|b)*c:x", b"ab", b"c"), ("[a-z]+ing:X", b"q", b"ing")]:
        o = Oracle(pat, "nft")
        p = prog(pat, "nft")
        rng = random.Random(5)
        head = corpus.word_soup(rng, 200000)
        short = head + b"x" + run * (30000 // len(run)) + close + b"\n" + head
        assert gpu_scan(p, short) == o.scan(short), pat
        long_ = head + b"x" + run * (70000 // len(run)) + close + b"\nmore lines\n" + b"x" + run * (80000 // len(run)) + close + b"\n" + head
        with pytest.raises(OracleError) as oe:              # the oracle models the limit (and so does the reference binary)
            o.scan(long_)
        want = oe.value.partial
        assert want.startswith(o.scan(head)) and len(want) < len(head) + 200000
        for fam in [trre_amd.KERNEL_AUTO] + [f for f in p.allowed_kernels() if f != trre_amd.KERNEL_BACKTRACK]:
            with pytest.raises(trre_amd.TrreError) as e:
                gpu_scan(p, long_, fam)
            assert e.value.code == trre_amd.api.E_DIVERGES and "stack max capacity reached" in e.value.message, (pat, fam)
            assert e.value.partial.cpu().numpy().tobytes() == want, (pat, fam)
        for kw in ({}, {"device_mask": 0}):                  # host buffers, chunks and shards
            with pytest.raises(trre_amd.TrreError) as e:
                p.scan(long_, **kw)
            assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial == want, (pat, kw)
            if pat != " +: ":
                continue
            with pytest.raises(trre_amd.TrreError) as e:
                p.scan(head * 200 + long_, **kw)             # the bad line in a later chunk (40 MB of clean lines first)
            assert e.value.partial == o.scan(head) * 200 + want, (pat, kw)
        if ref_available() and pat == " +: ":
            import subprocess
            import os
            from oracle_lib import REF_DIR
            r = subprocess.run([os.path.join(REF_DIR, "trre"), pat], input=long_, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 1 and r.stderr.startswith(b"error: stack max capacity reached") and r.stdout == want
    # in place (a length-preserving pattern with a loop): the guard looks before the launch, the lines before the bad one are
    # scanned in place, the bad line's part follows them
    pat = "(a:x)*b"
    p = prog(pat, "nft")
    data = b"aab ab\n" * 1000 + b"a" * 70000 + b"b\n" + b"tail\n"
    with pytest.raises(OracleError) as oe:
        Oracle(pat, "nft").scan(data)
    if trre_amd.KERNEL_STREAM_LP in p.allowed_kernels() or trre_amd.KERNEL_GUIDED_LP in p.allowed_kernels():
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        with pytest.raises(trre_amd.TrreError) as e:
            p.scan_tensor(t, out=t)
        assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial.cpu().numpy().tobytes() == oe.value.partial
    with pytest.raises(trre_amd.TrreError) as e:
        gpu_scan(p, data)
    assert e.value.partial.cpu().numpy().tobytes() == oe.value.partial
    # match mode (trre -m) runs the same search: one attempt per line
    pat = "(a|b)*c"
    pm = trre_amd.Program(pat, "nft", mode="match")
    data = b"abc\nxx\nbbac\n" * 500 + b"ab" * 35000 + b"c\nabc\n"
    with pytest.raises(OracleError) as oe:
        Oracle(pat, "nft").match(data)
    assert oe.value.partial == b"abc\nbbac\n" * 500
    with pytest.raises(trre_amd.TrreError) as e:
        gpu_scan(pm, data)
    assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial.cpu().numpy().tobytes() == oe.value.partial
    ok = b"abc\nxx\nbbac\n" * 500 + b"ab" * 15000 + b"c\nabc\n"
    assert gpu_scan(pm, ok) == Oracle(pat, "nft").match(ok)


def test_every_kernel_family_agrees_on_gpu():
    rng = random.Random(5)
    data = corpus.word_soup(rng, 300000) + corpus.printable_lines(rng, 300000) + b"tail without newline"
    for pat, eng in [("[a:A-z:Z]", "dft"), ("[a:b-y:zz:a]", "dft"), ("(cat:dog|dog:cat)", "dft"),
                     ("(cat:dog|dog:cat)", "nft"), ("cat:dog", "nft"), ("cat:dog", "dft"), ("a:xyz", "dft"),
                     ("[aie]:", "nft"), ("abc:2|ab:1", "nft"), ("abc:2|ab:1", "dft")]:
        p = prog(pat, eng)
        want = Oracle(pat, eng).scan(data)
        for fam in p.allowed_kernels():
            assert gpu_scan(p, data, fam) == want, (pat, eng, fam)


def test_unaligned_device_buffers():
    import torch
    rng = random.Random(9)
    data = corpus.word_soup(rng, 100000)
    for pat, eng in [("[a:A-z:Z]", "dft"), ("(cat:dog|dog:cat)", "nft"), ("cat:dog", "dft"), ("a:xyz", "dft")]:
        p = prog(pat, eng)
        want = Oracle(pat, eng).scan(data)
        for in_mis, out_mis in [(1, 1), (5, 5), (3, 0), (0, 7), (9, 12)]:
            src = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
            src[in_mis:in_mis + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            dst = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
            got = p.scan_tensor(src[in_mis:in_mis + len(data)], out=dst[out_mis:])
            assert got.cpu().numpy().tobytes() == want, (pat, eng, in_mis, out_mis)


def test_long_lines_on_gpu():
    base = b"cat dog ca do " * 400           # 5.6 kB lines: longer than the tile halo
    data = (b"short cat\n" + base + b"\n" + b"dog\n" + base * 3 + b"\nend cat\n") * 30
    for pat, eng in [("(cat:dog|dog:cat)", "dft"), ("(cat:dog|dog:cat)", "nft"), ("a:xyz", "dft"), ("[aie]:", "nft"), ("[a:A-z:Z]", "dft")]:
        p = prog(pat, eng)
        want = Oracle(pat, eng).scan(data)
        for fam in p.allowed_kernels():
            assert gpu_scan(p, data, fam) == want, (pat, eng, fam)
    one = b"cat " * 300000                     # a single 1.2 MB line without a newline
    assert gpu_scan(prog("(cat:dog|dog:cat)", "dft"), one) == Oracle("(cat:dog|dog:cat)", "dft").scan(one)


def test_very_long_lines_through_the_guided_families():
    """The backward pass bounds its look-ahead (64 KiB): inside a longer line one lane becomes the line's walker and carries
    the state through the lanes that stand back (every lane used to rescan the rest of the line — quadratic, an
    8 MiB line took minutes).  Lines of 100 kB .. 6 MB between ordinary ones, every guided family, against the oracle."""
    import time
    rng = random.Random(31)
    long1 = (b"abcab xyz " * 10000)[:100000]
    long2 = bytes(rng.choice(b"abcxyz 0123") for _ in range(700000))
    long3 = (b"abx cat 7" * 700000)                           # 6 MB (loops stay short: the reference's stack holds 65 536 items)
    data = corpus.word_soup(rng, 50000) + long1 + b"\n" + b"short abc\n" + long2 + b"c\n" + corpus.word_soup(rng, 30000) + long3 + b"\nabc\n" + long1
    for pat in ("(a|b)*c:x", "[0-9]+:N", "(cat:dog|dog:cat)"):
        p = prog(pat, "nft")
        want = Oracle(pat, "nft").scan(data)
        for fam in (trre_amd.KERNEL_GUIDED_LP, trre_amd.KERNEL_GUIDED_GEN):
            if fam in p.allowed_kernels():
                t0 = time.time()
                assert gpu_scan(p, data, fam) == want, (pat, fam)
                assert time.time() - t0 < 20, (pat, fam, "the backward pass must not be quadratic in the line length")


@pytest.mark.parametrize("env", [{"TRRE_LANE_BYTES": "256"}, {"TRRE_LANE_BYTES": "4096"}, {"TRRE_LANE_BYTES": "1024"},
                                 {"TRRE_NO_G16": "1"}, {"TRRE_NO_FB": "1"}, {"TRRE_FB_EMIT": "1"}, {"TRRE_NO_FB_COPY": "1"}, {"TRRE_NO_LPW_PAIR": "1"}])
def test_alternative_stream_implementations(env):
    """the stream families at other lane sizes, on the 8-byte entries only, large tables without their
    fallback form / with both passes on it / without its copy form, the window walk one byte per step (selected by environment, which the library reads once per process)"""
    import os
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_impl_check.py")
    r = subprocess.run([sys.executable, script], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode("latin-1")[-2000:]


def test_mask_scratch_grows_with_the_input():
    """NFT tile kernels need a mask scratch for lines longer than the LDS tile; one left by a smaller
    scan must not be reused for a larger one (found by tools/gpu_fuzz.py)"""
    p = prog("c", "nft")
    o = Oracle("c", "nft")
    for n_lines in (3, 40):
        data = b"".join(b"abcxy" * 9000 + b"\n" + b"cab\n" for _ in range(n_lines))
        for fam in (trre_amd.KERNEL_TILE_LP, trre_amd.KERNEL_TILE_GEN):
            assert gpu_scan(p, data, fam) == o.scan(data), (n_lines, fam)


def test_host_path_redownloads_after_a_relaunch():
    """trre_scan_host queues an early download behind the first launch of a length-preserving chunk; when finish()
    has to run the chunk again (here: mask scratch for 45 kB lines on the NFT tile kernels) the bytes fetched early
    are stale and must be fetched again (silently wrong output through trre_scan_host / the CLI)"""
    p = prog("c", "nft")
    o = Oracle("c", "nft")
    data = b"".join(b"abcxy" * 9000 + b"\n" + b"cab\n" for _ in range(12))
    p.set_kernel(trre_amd.KERNEL_TILE_LP)
    try:
        assert p.scan(data) == o.scan(data)
        assert p.scan(data, device_mask=0) == o.scan(data)
    finally:
        p.set_kernel(trre_amd.KERNEL_AUTO)
    # the same through a bounded fold that overflows (stream_lp -> general family) and through a NUL
    for pat, eng, d in [("a+:b", "nft", b"x" + b"a" * 200 + b"y\n" + b"caab\n" * 3000), ("(cat:dog|dog:cat)", "nft", b"cat\0dog\n" + b"a cat\n" * 5000)]:
        pp = prog(pat, eng)
        assert pp.scan(d) == Oracle(pat, eng).scan(d), (pat, eng)


def test_capacity_error_reports_needed_size():
    import ctypes
    import torch
    p = prog("a:xyz", "dft")
    data = b"banana\n" * 1000
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    small = torch.empty(100, dtype=torch.uint8, device="cuda")
    m = ctypes.c_size_t()
    rc = trre_amd.api.lib().trre_scan_device(p._h, t.data_ptr(), t.numel(), small.data_ptr(), small.numel(),
                                             ctypes.byref(m), None)
    assert rc == trre_amd.api.E_CAPACITY and m.value == len(Oracle("a:xyz", "dft").scan(data))


def test_against_the_compiled_reference_binary():
    """4 MiB of seeded text against the digests of the compiled reference's outputs (tests/golden/fresh.json), and against the
    binary itself when oracle/_ref travelled along"""
    for pat, eng, data, want in golden_lib.fresh_cases("gpu"):
        got = gpu_scan(prog(pat, eng), data)
        assert golden_lib.digest(got) == want, (pat, eng)
        if ref_available():
            assert got == ref_scan(pat, eng, data, timeout=600), (pat, eng)


def test_full_size_properties_1gib_uppercase():
    """BASELINE config 2 at full size through a size-independent property: the
    output must equal the input with a-z shifted to A-Z (computed independently
    with torch on the device), and an oracle-checked 8 MiB slice."""
    import torch
    n = 1 << 30
    g = torch.Generator(device="cuda").manual_seed(1234)
    data = torch.randint(0x20, 0x7f, (n,), dtype=torch.uint8, device="cuda", generator=g)
    ends = torch.cumsum(torch.randint(33, 162, (n // 90,), device="cuda", generator=g), 0)
    data[ends[ends < n]] = 10
    data[-1] = 10
    p = prog("[a:A-z:Z]", "dft")
    for fam in [trre_amd.KERNEL_AUTO] + p.allowed_kernels():
        p.set_kernel(fam)
        out = p.scan_tensor(data)
        p.set_kernel(trre_amd.KERNEL_AUTO)
        lower = (data >= 97) & (data <= 122)
        assert out.numel() == n
        assert torch.equal(out, torch.where(lower, data - 32, data)), fam
        del lower
    cut = int((data[: 8 << 20] == 10).nonzero()[-1]) + 1
    host = data[:cut].cpu().numpy().tobytes()
    assert out[:cut].cpu().numpy().tobytes() == Oracle("[a:A-z:Z]", "dft").scan(host)


def test_dictionary_config_on_gpu():
    """BASELINE config 5 shape: the seeded 1000-entry key:value dictionary, both engines (the NFT
    engine has 5555 CONS states and runs through the folded stream table)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import dictgen
    keys, vals = dictgen.make_dictionary(1000)
    pat = dictgen.pattern(keys, vals)
    data = dictgen.corpus_fast(keys, 3 << 20)
    for eng in ("dft", "nft"):
        p = prog(pat, eng)
        want = Oracle(pat, eng).scan(data[: 1 << 18] if eng == "nft" else data)   # the NFT oracle is ~0.2 MB/s here
        got = gpu_scan(p, data[: 1 << 18] if eng == "nft" else data)
        assert got == want, eng


def test_a_positional_launch_void_by_a_nul_reports_nothing_else():
    """(tests/test_front_shim.py, the same name) through the library: every family, no TRRE_E_DIVERGES"""
    for pat, data in [(b"c|(\\\\c)?((a:.*[c:a-y:a]):x.)|(a).[b:y-y:y]", b"x\x00axa\nx\n"),
                      (b"y|[ba](\\([c-y]|c[aa]*?:([b-y]a{2})+?)", b"xzx<>xcyz\nbxcabay\nc\x00cbyacbycacy\nxxxcxbbxcy\n\ny\n")]:
        p = prog(pat, "dft")
        want = Oracle(pat, "dft").scan(data)
        for fam in p.allowed_kernels():
            assert gpu_scan(p, data, fam) == want, (pat, fam)


def test_byte_map_repairs_its_output_after_nul_bytes():
    """A NUL cuts its line short (Q2): the byte map's positional launch is void, the library maps the stretches between
    the cut lines again to where they belong (runtime.cpp, repair_bytemap_nuls) — NULs at every place of a line, several in
    one line, in the last line with and without a newline, as the first and the last byte, misaligned buffers; more NULs
    or cut lines than the repair takes (the general family runs instead); against the oracle."""
    import torch
    rng = random.Random(5)
    p = prog("[a:A-z:Z]", "dft")
    assert p.info.kernel == trre_amd.KERNEL_BYTEMAP
    o = Oracle("[a:A-z:Z]", "dft")
    base = corpus.word_soup(rng, 300000)
    cases = [b"ab\0cd\nef\n", b"ab\0cd", b"\0", b"\0\n", b"a\0", b"\0a\n\0\nb\n", b"x\0y\0z\nq\n", b"abc\n\0", b"abc\n\0\n"]
    for k in (1, 3, 40, 200, 300, 1500):
        buf = bytearray(base)
        for _ in range(k):
            buf[rng.randrange(len(buf))] = 0
        cases.append(bytes(buf))
    one = bytearray(base)
    one[len(one) // 2] = 0
    cases += [bytes(one) + b"tail without newline", b"\0" + bytes(one), bytes(one) + b"\0",
              b"ab\0" + b"x" * (5 << 20) + b"\nend\n"]               # (a line of megabytes behind a NUL: not repaired, run again)
    for data in cases:
        want = o.scan(data)
        for skip_in, skip_out in ((0, 0), (3, 3), (5, 0)):
            t = torch.frombuffer(bytearray(b"x" * skip_in + data), dtype=torch.uint8).cuda()[skip_in:]
            out = torch.empty(len(data) + 64 + skip_out, dtype=torch.uint8, device="cuda")[skip_out:]
            got = p.scan_tensor(t, out=out).cpu().numpy().tobytes()
            assert got == want, (len(data), data[:20], skip_in, skip_out)


def test_random_dictionaries_on_gpu():
    """Seeded dictionaries large enough for the fallback form of their tables — prefix-free or keys inside keys, texts of
    0..8 bytes, partial keys, key upon key, lines of kilobytes, sparse and dense — both engines against the oracle: the copy
    form where the tables have it (most of these), the count / emit pair where they do not or where a launch declares itself
    void (texts every three bytes)."""
    rng = random.Random(4242)
    checked = 0
    for it in range(8):
        letters = "abcdefgh"[:rng.randint(6, 8)]
        keys = set()
        while len(keys) < rng.choice([300, 450, 600]):
            keys.add("".join(rng.choice(letters) for _ in range(rng.randint(2, 7))))
        keys = sorted(keys)
        if it % 2:
            keys = [k for k in keys if not any(o != k and k.startswith(o) for o in keys)]
        rng.shuffle(keys)
        lo = 0 if it == 5 else 1
        vals = ["".join(rng.choice("XYZxyz01") for _ in range(rng.randint(lo, 8))) for _ in keys]
        pat = "|".join("%s:%s" % kv for kv in zip(keys, vals))
        density = [0.05, 0.15, 0.3, 0.6][it % 4]
        toks = []
        size = 0
        while size < 400000:
            r = rng.random()
            if r < density:
                t = rng.choice(keys)
            elif r < density + 0.1:
                t = rng.choice(keys)[:rng.randint(1, 6)] + rng.choice(letters)
            elif r < density + 0.15:
                t = rng.choice(keys) + rng.choice(keys) + rng.choice(keys)
            else:
                t = "".join(rng.choice(letters + "xyz") for _ in range(rng.randint(1, 9)))
            t += rng.choice([" ", " ", "\n", ",", "", ""]) if it != 3 else rng.choice([" ", ",", ""])
            toks.append(t)
            size += len(t)
        data = "".join(toks).encode() + rng.choice([b"\n", b""])
        for eng in ("dft", "nft"):
            try:
                p = prog(pat, eng)
            except trre_amd.TrreError:
                continue
            buf = data if eng == "dft" else data[: 1 << 16]           # (the NFT oracle is slow on these)
            assert gpu_scan(p, buf) == Oracle(pat, eng).scan(buf), (it, eng)
            checked += 1
    assert checked >= 12


def test_a_program_stops_trying_its_bounded_table_after_an_overflow():
    """round 4: the count pass of a bounded fold that meets a run it was not built for voids the launch (the emit pass leaves at
    once), finish() runs the buffer on the guided kernels — and the scans after it go there directly"""
    p = trre_amd.Program(" +: ", "nft")
    o = Oracle(" +: ", "nft")
    assert p.info.kernel == trre_amd.KERNEL_STREAM_GEN
    short = b"a  b   c\n" * 20000
    assert gpu_scan(p, short) == o.scan(short) and p.info.kernel == trre_amd.KERNEL_STREAM_GEN
    long_run = short + b"x" + b" " * 300 + b"y\n" + short
    assert gpu_scan(p, long_run) == o.scan(long_run)
    assert p.info.kernel == trre_amd.KERNEL_GUIDED_GEN                     # (what a scan launches from now on)
    assert gpu_scan(p, short) == o.scan(short) and gpu_scan(p, long_run) == o.scan(long_run)
    assert gpu_scan(p, short, trre_amd.KERNEL_STREAM_GEN) == o.scan(short)  # (forcing the family still works)


def test_bounded_fold_falls_back_to_the_tile_kernels():
    """greedy loops fold into stream tables for runs of up to 64 bytes; a longer run voids the launch
    (overflow mark) and the tile kernels produce the result"""
    rng = random.Random(12)
    base = corpus.word_soup(rng, 200000).replace(b" ", b"  ")
    long_run = base + b"p" + b" " * 300 + b"q aaaa" + b"a" * 150 + b"b\n" + base
    for pat in (" +: ", "a+:b", "a*b:x", " *, *:,"):
        for eng in ("nft", "dft"):
            p = prog(pat, eng)
            o = Oracle(pat, eng)
            for data in (base, long_run):
                assert gpu_scan(p, data) == o.scan(data), (pat, eng, len(data))


def test_host_buffers_in_chunks():
    """trre_scan_host pipelines inputs larger than 64 MiB in line-aligned chunks; a too small output
    buffer reports the size needed"""
    import ctypes
    rng = random.Random(77)
    block = corpus.word_soup(rng, 3 << 20) + b"a line without cats\n"
    data = block * 50                                        # ~150 MiB, three chunks
    for pat, eng in [("(cat:dog|dog:cat)", "nft"), ("a:xyz", "dft"), ("[a:A-z:Z]", "dft")]:
        p = prog(pat, eng)
        want_block = Oracle(pat, eng).scan(block)
        got = p.scan(data)
        assert len(got) == len(want_block) * 50, (pat, eng)
        assert got[:len(want_block)] == want_block and got[-len(want_block):] == want_block, (pat, eng)
        assert got == want_block * 50, (pat, eng)
    p = prog("a:xyz", "dft")
    small = ctypes.create_string_buffer(1 << 20)
    m = ctypes.c_size_t()
    rc = trre_amd.api.lib().trre_scan_host(p._h, data, len(data), small, len(small), ctypes.byref(m), 0)
    assert rc == trre_amd.api.E_CAPACITY and m.value == len(Oracle("a:xyz", "dft").scan(block)) * 50


def test_random_patterns_against_the_oracle():
    """a short run of the differential fuzz (tools/gpu_fuzz.py): random patterns and inputs, every kernel
    family each pattern admits, misaligned buffers"""
    import os
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gpu_fuzz.py")
    # (the backtracking fallback is among the families of every NFT pattern: a small step budget keeps the cases on which the
    # reference's search is exponential — errors there, skipped by the fuzz — from taking ten seconds each)
    # (... and the stack guard searches the fuzz's 70 KB lines of loop bytes, quadratic ones up to its budget: a smaller budget
    # leaves them undecided sooner — the scan's output stands, which is what the oracle says wherever it answers at all)
    env = dict(os.environ, TRRE_BT_BUDGET="1000000", TRRE_GUARD_BUDGET="2000000")
    r = subprocess.run([sys.executable, script, "--seconds", "30", "--seed", "20250926"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=420, env=env)
    out = r.stdout.decode("latin-1")
    assert r.returncode == 0 and "0 mismatches" in out, out[-2000:]


def test_wide_guided_tables_on_gpu():
    """patterns whose backward DFA has more than 256 states (round 2: TRRE_E_UNSUPPORTED beyond 64 nodes): 16-bit symbols,
    both tables through L1 / L2.  Scan mode (automatic choice and forced), match mode, a divergence's partial output."""
    rng = random.Random(6)
    data = b"".join(bytes(rng.choice(b"abcdefghxyz ") for _ in range(rng.randint(0, 300))) + b"\n" for _ in range(20000)) + b"xabcdefghy tail"
    for pat in ("a(a|b|c|d|e|f|g|h){9}c:x", "x.{8}y:z", "a(a|b|c){9}c:x"):
        p = prog(pat, "nft")
        assert p.info.guided_rev_states > 256
        want = Oracle(pat, "nft").scan(data)
        assert gpu_scan(p, data) == want, pat
        assert gpu_scan(p, data, trre_amd.KERNEL_GUIDED_GEN) == want, (pat, "wide")
    pat = "[a-h]{8}(a|b)[a-z ]*"
    assert gpu_scan(trre_amd.Program(pat, "nft", mode="match"), data) == Oracle(pat, "nft").match(data)
    p = prog("x.{8}y:z|q:*", "nft")
    with pytest.raises(trre_amd.TrreError) as e:
        gpu_scan(p, b"x12345678y a\nx12345678y q b\nnever\n")
    assert e.value.code == trre_amd.api.E_DIVERGES and e.value.partial.cpu().numpy().tobytes() == b"z a\nz "


def test_match_mode_on_gpu():
    """`trre -m` through the C ABI (trre_compile_mode, TRRE_MODE_MATCH): golden vectors of the compiled reference,
    and a larger buffer against the oracle's match mode"""
    progs = {}
    n = 0
    for pat, name, data, exp in golden_lib.match_cases():
        if pat not in progs:
            progs[pat] = trre_amd.Program(pat, "nft", mode="match")
        if exp is None:
            with pytest.raises(trre_amd.TrreError) as e:
                gpu_scan(progs[pat], data)
            assert e.value.code == trre_amd.api.E_DIVERGES
        else:
            assert gpu_scan(progs[pat], data) == exp, (pat, name)
        n += 1
    assert n > 100
    rng = random.Random(3)
    data = corpus.word_soup(rng, 2 << 20, max_len=30) + b"cat\ndog\n\nlast cat"
    for pat in ("(cat:dog|dog:cat| |[a-z]|[A-Z])*", "[a-z ]*", ".*(cat:dog).*"):
        assert gpu_scan(trre_amd.Program(pat, "nft", mode="match"), data) == Oracle(pat, "nft").match(data), pat


def test_backtracking_fallback_on_gpu():
    """family 9 (round 4): the reference's depth-first search, a lane per KiB with its own stack — every NFT golden vector, and a
    pattern beyond every table form (round 3: TRRE_E_UNSUPPORTED) on 32 MiB against the oracle"""
    n = 0
    for pat, name, data, engine, exp in golden_lib.cases():
        if engine != "nft" or exp is None or len(data) > 20000:
            continue
        p = prog(pat, engine)
        assert gpu_scan(p, data, trre_amd.KERNEL_BACKTRACK) == exp, (pat, name)
        n += 1
    assert n > 430, n
    pat = "a(a|b|c|d|e|f|g|h){12}c:x"
    p = prog(pat, "nft")
    assert p.info.kernel == trre_amd.KERNEL_BACKTRACK
    rng = random.Random(3)
    block = bytearray(corpus.printable_lines(rng, 1 << 20))
    for _ in range(3000):
        at = rng.randrange(len(block) - 20)
        if b"\n" not in block[at:at + 14]:
            block[at:at + 14] = b"a" + bytes(rng.choice(b"abcdefgh") for _ in range(12)) + b"c"
    data = bytes(block) * 32
    want = Oracle(pat, "nft").scan(bytes(block))
    assert want != bytes(block)
    assert gpu_scan(p, data) == want * 32
    assert p.scan(bytes(block)) == want                                # host buffers
    # beyond its limits: an error, not a hang and not a wrong answer
    q = prog("(a|aa)*b:x", "nft")
    with pytest.raises(trre_amd.TrreError) as e:
        gpu_scan(q, b"a" * 60 + b"\n" + b"aab\n" * 100, trre_amd.KERNEL_BACKTRACK)
    assert e.value.code == trre_amd.api.E_UNSUPPORTED
    assert gpu_scan(q, b"a" * 12 + b"\n" + b"aab\n" * 100, trre_amd.KERNEL_BACKTRACK) == b"a" * 12 + b"\n" + b"x\n" * 100
