"""The children of tests/test_gpu_mapgen_oracle.py: one job per process (TRRE_MAPGEN* are read once per process), every output compared byte
for byte with the oracle.  Prints `RESULT <repr of a dict>` as its last line: "scans" (launches on inputs of at least one byte), "bad" (the
first mismatches; empty: all equal) and what the job adds.      python tests/gpu_mapgen_check.py <job> [grid]"""
import ctypes
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE, os.path.join(ROOT, "tools")):
    sys.path.insert(0, d)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import corpora  # noqa: E402
import golden_lib  # noqa: E402
import trre_amd  # noqa: E402
from oracle_lib import Oracle, scan_mt  # noqa: E402
from trre_amd import api  # noqa: E402

TILE = 16384
SENTINEL = 0xA5
PAD = 1 << 20
DEV = torch.device("cuda", 0)
GEN = {v: k for k, v in trre_amd.KERNEL_NAMES.items()}["stream_gen"]
LENS8 = "(a:|b:bb|c:ccc|d:dddd|e:eeeee|f:ffffff|g:ggggggg|h:hhhhhhhh)"
HTML = "(<:&lt;|>:&gt;|&:&amp;)"
UPPER = "(n:nn|o:ooo|p:pppp|q:qqqqq|r:rrrrrr|s:sssssss|t:tttttttt|u:uu|v:vvv|w:wwww|x:xxxxx|y:yyyyyy|z:zzzzzzz)"
# what each makes the kernel do: test_gpu_mapgen_oracle.py's docstring; test_the_programs_are_memoryless_and_reach_every_instantiation (CPU
# tier) shows from the tables that every one carries the memoryless form and that the list reaches all four instantiations
PROGRAMS = [("[aie]:", "nft"), ("[aie]:", "dft"), ("(a:b|e:)", "nft"), ("(a:b|e:)", "dft"), ("a:xyz", "nft"), ("a:xyz", "dft"), (HTML, "nft"), (HTML, "dft"),
            ("(a:b|e:|c:xyz)", "nft"), ("(a:b|e:|c:xyz)", "dft"), (LENS8, "nft"), (LENS8, "dft"), ("[a-z]:", "nft"), ("[a-z]:", "dft"), (".:", "nft"), (".:", "dft"),
            ("e:12345678", "nft"), ("e:12345678", "dft"), (".:12345678", "dft"), (":x", "nft")]
ALTERNATING = [("[a-m]:", "dft"), (UPPER, "dft"), ("[aie]:", "nft"), (LENS8, "nft")]
bad = []
scans = 0


def program(pat, eng):
    p = trre_amd.Program(pat, eng)
    p.set_kernel(GEN)                                  # (the family whose one-pass form k_mapgen is: a change of routing cannot take a case elsewhere)
    return p


def lens_of(p):
    """the program's length table (StreamBlobHeader::off_mg): for the tile index of a mismatch only"""
    blob = p.export_stream_tables()
    off = struct.unpack_from("<48I", blob, 0)[45]
    return np.array(struct.unpack_from("<1024I", blob, off)[2::4], dtype=np.int64) & 15


def corpus(n, seed):
    """n bytes whose tiles' totals differ and trend along the buffer: printable lines | token soups whose weights drift | lines longer than
    several tiles | long lines of lowercase letters, mostly 'e' (a tile of them: nothing left by '[a-z]:', 8 x by 'e:12345678')"""
    a, b, c = n * 3 // 8, n // 4, n // 4
    d = n - a - b - c
    parts = [corpora.printable_lines(a, seed, DEV)] if a else []
    vocab = ["the", "a", "e", "eee", "<b>", "&", "<<>>", "abcdefgh", "hhhh", "ing", "x", "aaaa", "&&&&", "zebra"]
    for k in range(4):
        nb = b // 4 if k < 3 else b - 3 * (b // 4)
        if nb:
            parts.append(corpora.token_soup(nb, seed + 10 + k, DEV, vocab, [1.0 + ((j * 7 + k * 5) % 14) * (k + 1) for j in range(len(vocab))], block_tokens=1 << 22))
    if c:
        parts.append(corpora.long_lines(c, seed + 1, DEV, 70000))
    if d:
        g = torch.Generator(device=DEV).manual_seed(seed + 2)
        low = torch.randint(97, 123, (d,), dtype=torch.uint8, device=DEV, generator=g)
        low[torch.rand(d, device=DEV, generator=g) < 0.8] = ord("e")
        low[50000::50001] = 10
        low[d - 1] = 10
        parts.append(low)
    return torch.cat(parts)


def run(p, src, want, in_off, out_off, what, cap=None):
    """one scan of src (a device tensor) from offset in_off of an allocation into offset out_off of another, cap bytes (default: what is needed
    + 64); the output against `want` on the device; the bytes before and behind the output view stay as they were"""
    global scans
    n = src.numel()
    cap = len(want) + 64 if cap is None else cap
    ibuf = torch.full((in_off + n + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    ibuf[in_off:in_off + n] = src
    obuf = torch.full((out_off + cap + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    try:
        p.enqueue(ibuf[in_off:in_off + n], obuf[out_off:out_off + cap])
        m = p.finish()
    except trre_amd.TrreError as e:
        scans += n > 0
        bad.append("%s: %s" % (what, e))
        return False
    scans += n > 0
    w = torch.frombuffer(bytearray(want), dtype=torch.uint8).to(DEV) if want else torch.empty(0, dtype=torch.uint8, device=DEV)
    ok = m == len(want) and torch.equal(obuf[out_off:out_off + m], w)
    if not ok:
        k = min(m, len(want))
        ne = (obuf[out_off:out_off + k] != w[:k]).nonzero()
        at = int(ne[0]) if ne.numel() else k
        cum = np.cumsum(lens_of(p)[src.cpu().numpy()]) if n else np.zeros(1)
        bad.append("%s: %d bytes, want %d; first difference at output offset %d, input tile %d" % (what, m, len(want), at, int(np.searchsorted(cum, at, side="right")) // TILE))
    if not bool((obuf[out_off + cap:] == SENTINEL).all()) or not bool((obuf[:out_off] == SENTINEL).all()):
        bad.append("%s: written outside the output view" % what)
        ok = False
    return ok


def oracle(pat, eng, t):
    data = t.cpu().numpy().tobytes()
    return scan_mt(pat, eng, 16, data) if len(data) > (1 << 20) else Oracle(pat, eng).scan(data)


def job_grid(_):
    """the grid of a launch, from the launch: TRRE_MAPGEN_DBG leaves every tile's workgroup (k_mapgen: dbg[16 tile + 10] = blockIdx.x)"""
    p = program("[aie]:", "nft")
    n_tiles = 16384
    p.scan_tensor(corpora.printable_lines(n_tiles * TILE, 5, DEV))
    d = np.fromfile(os.environ["TRRE_MAPGEN_DBG"], dtype=np.uint64).reshape(-1, 16)[:n_tiles, 10].astype(np.int64)
    G = int(d.max()) + 1
    assert G < n_tiles // 2 and bool((d == np.arange(n_tiles) % G).all()), G       # (workgroup w takes the tiles w, w + G, ..)
    return {"grid": G}


def job_edges(G):
    """sizes k 16384 + d around the tile edges and the grid's, input views at 0 / 1 / 7 / 8 / 15 of an allocation, output views at 0 / 1 / 15 (every
    pair of the two is met: they cycle with coprime periods over the 40 sizes and 20 programs); the ends: no final newline, '\\n' alone, nothing"""
    ks = sorted({0, 1, 2, 3, G - 1, G, G + 1, 2 * G + 1})
    sizes = [k * TILE + d for k in ks for d in (-1, 0, 1, 15, 17) if k * TILE + d >= 0]
    base = corpus((2 * G + 1) * TILE + 64, 77)
    case = 0
    for j, (pat, eng) in enumerate(PROGRAMS):
        p = program(pat, eng)
        for i, n in enumerate(sizes):
            src = base[(i * 29) % 61:][:n].clone()
            if n and i % 3 != 1:
                src[n - 1] = 10                        # (two sizes in three end with a line end; the others end where the corpus is cut)
            in_off, out_off = (0, 1, 7, 8, 15)[case % 5], (0, 1, 15)[case % 3]
            case += 1
            run(p, src, oracle(pat, eng, src), in_off, out_off, "%r/%s n=%d in+%d out+%d" % (pat, eng, n, in_off, out_off))
        for data in (b"\n", b"x", b"ae<\n\n\nee", b"\n" * 70000, b"e" * 40000):
            src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
            run(p, src, Oracle(pat, eng).scan(data), 1, 15, "%r/%s %r.." % (pat, eng, data[:8]))
        run(p, torch.empty(0, dtype=torch.uint8, device=DEV), Oracle(pat, eng).scan(b""), 0, 0, "%r/%s empty" % (pat, eng))
    return {}


def job_golden(_):
    """every golden vector whose program is memoryless, a program of its own each (an input with a NUL voids the launch: two of those would
    retire the kernel for the program), against the vector's recorded output"""
    n = nul = 0
    for pat, name, data, eng, exp in golden_lib.cases():
        if exp is None:
            continue
        try:
            p = trre_amd.Program(pat, eng)
        except trre_amd.TrreError:
            continue
        blob = p.export_stream_tables()
        if not blob or len(blob) < 192 or struct.unpack_from("<48I", blob, 0)[46] == 0 or GEN not in p.allowed_kernels():
            continue
        p.set_kernel(GEN)
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV) if data else torch.empty(0, dtype=torch.uint8, device=DEV)
        run(p, src, exp, (0, 3)[n % 2], (0, 1, 15)[n % 3], "golden %r/%s on %s" % (pat, eng, name), cap=max(len(exp), len(data)) + 64)
        n += 1
        nul += bool(data) and b"\0" in data
    return {"vectors": n, "with_nul": nul}


def job_depth(_):
    """the look-back's reach: MAPGEN_CHECK_MIB of the drifting corpus (256: 16 384 tiles, every program; 1024: 65 536 tiles, '[aie]:' and
    'a:xyz'), whole outputs against the 16-thread oracle"""
    mib = int(os.environ["MAPGEN_CHECK_MIB"])
    progs = PROGRAMS if mib <= 256 else [("[aie]:", "nft"), ("a:xyz", "dft")]
    inp = corpus(mib << 20, 91)
    data = inp.cpu().numpy().tobytes()
    for k, (pat, eng) in enumerate(progs):
        want = scan_mt(pat, eng, 16, data)
        run(program(pat, eng), inp, want, 0, (0, 1, 15)[k % 3], "%r/%s on %d MiB" % (pat, eng, mib))
        del want
    return {}


def job_nul(_):
    """a NUL at byte 0, at 16384 k - 1 and 16384 k, inside a long line: the launch is void, the general family answers; then, on ONE program, three
    buffers with a NUL and a clean one: the void count may retire the kernel, the bytes stay the oracle's"""
    base = corpora.long_lines(9 * TILE + 100, 13, DEV, 40000)
    for pat, eng in [("a:xyz", "dft"), ("[aie]:", "nft"), (LENS8, "dft")]:
        for at in (0, TILE - 1, TILE, 3 * TILE - 1, 3 * TILE, 5 * TILE + 777):
            src = base.clone()
            src[at] = 0
            run(program(pat, eng), src, oracle(pat, eng, src), 0, 1, "%r/%s NUL at %d" % (pat, eng, at))
        p = program(pat, eng)
        for at in (100, 2 * TILE, 8 * TILE, None):
            src = base.clone()
            if at is not None:
                src[at] = 0
            run(p, src, oracle(pat, eng, src), 7, 0, "%r/%s one program, NUL at %s" % (pat, eng, at))
    return {}


def job_default(_):
    """TRRE_MAPGEN unset: 'a:xyz' three times on one program (its own choice of family): the first scan on k_mapgen, the later ones on the pair
    (the output was 4 % longer than the input: mapgen_dense)"""
    inp = corpora.printable_lines(8 << 20, 3, DEV)
    p = trre_amd.Program("a:xyz", "dft")
    want = oracle("a:xyz", "dft", inp)
    for k in range(3):
        run(p, inp, want, 0, 0, "'a:xyz' by default, scan %d" % k)
    return {"grew": len(want) / inp.numel()}


def job_capacity(_):
    """an output view of exactly the m bytes needed: the oracle's bytes; of m - 1: TRRE_E_CAPACITY, the size needed reported; nothing written
    behind the view either way"""
    L = api.lib()
    for pat, eng in [("a:xyz", "dft"), ("[aie]:", "nft"), ("e:12345678", "dft"), (LENS8, "nft")]:
        for n in (70000, 3 * TILE + 5, 40 * TILE):
            src = corpus(n, 5)
            want = oracle(pat, eng, src)
            for out_off in (0, 1, 15):
                run(program(pat, eng), src, want, 8, out_off, "%r/%s n=%d exact capacity out+%d" % (pat, eng, n, out_off), cap=len(want))
                global scans
                cap = len(want) - 1
                obuf = torch.full((out_off + cap + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
                m = ctypes.c_size_t()
                p = program(pat, eng)
                rc = L.trre_scan_device(p._h, src.data_ptr(), n, obuf[out_off:].data_ptr(), cap, ctypes.byref(m), torch.cuda.current_stream(DEV).cuda_stream)
                torch.cuda.synchronize()
                scans += 1
                if rc != api.E_CAPACITY or m.value != len(want):
                    bad.append("%r/%s n=%d one byte short: rc %d, %d reported, %d needed" % (pat, eng, n, rc, m.value, len(want)))
                if not bool((obuf[out_off + cap:] == SENTINEL).all()) or not bool((obuf[:out_off] == SENTINEL).all()):
                    bad.append("%r/%s n=%d one byte short: written outside the output view" % (pat, eng, n))
    return {}


def job_alternate(G):
    """programs whose length tables disagree on most lowercase letters, in turn on inputs of exactly G tiles — every tile is its workgroup's first,
    the one tile counted right after the tables were staged —: 64 rounds, the first mismatch ends it"""
    global scans
    inp = corpus(G * TILE, 31)
    low = torch.randint(97, 123, (G * TILE,), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    inp = torch.where(inp == 10, inp, torch.where(torch.arange(G * TILE, device=DEV) % 3 == 0, inp, low))     # (two bytes in three: lowercase letters)
    inp[-1] = 10
    progs = [(pat, eng, program(pat, eng)) for pat, eng in ALTERNATING]
    wants = [torch.frombuffer(bytearray(oracle(pat, eng, inp)), dtype=torch.uint8).to(DEV) for pat, eng, _ in progs]
    out = torch.empty(8 * inp.numel() + 4096, dtype=torch.uint8, device=DEV)
    for rnd in range(64):
        for (pat, eng, p), w in zip(progs, wants):
            p.enqueue(inp, out)
            m = p.finish()
            scans += 1
            if m != w.numel() or not torch.equal(out[:m], w):
                k = min(m, w.numel())
                ne = (out[:k] != w[:k]).nonzero()
                at = int(ne[0]) if ne.numel() else k
                cum = np.cumsum(lens_of(p)[inp.cpu().numpy()])
                bad.append("round %d, %r/%s: %d bytes, want %d; first difference at output offset %d, tile %d" % (rnd, pat, eng, m, w.numel(), at, int(np.searchsorted(cum, at, side="right")) // TILE))
                return {"rounds": rnd}
    return {"rounds": 64}


FUZZ_SEEDS, FUZZ_CASES = (11, 12, 13), 30


def job_fuzz(G):
    global scans
    import gpu_fuzz
    drawn = skipped = 0
    for seed in FUZZ_SEEDS:
        d, s, r, b = gpu_fuzz.run_memoryless(seed, FUZZ_CASES, G)
        drawn += d
        skipped += s
        scans += r
        bad.extend(b)
    return {"drawn": drawn, "skipped": skipped}


if __name__ == "__main__":
    extra = globals()["job_" + sys.argv[1]](int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    print("%s: %d scans of at least one byte, %d mismatches" % (sys.argv[1], scans, len(bad)), file=sys.stderr)
    print("RESULT " + repr(dict(extra, scans=scans, n_bad=len(bad), bad=bad[:8])))
