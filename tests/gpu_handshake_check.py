"""The child of tests/test_gpu_handshake.py: the cases of ONE environment (the switches are read once per process), each through the C ABI at a
capacity of exactly the oracle's size and of one byte less.  Prints `RESULT <repr of a dict>` as its last line: "cases" (the names of the cases
that ran, in order), "calls" (trre_scan_device calls made) and "bad" (what was wrong; empty: nothing).
    python tests/gpu_handshake_check.py <job>"""
import ctypes
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE, os.path.join(ROOT, "tools")):
    sys.path.insert(0, d)
import torch  # noqa: E402

import corpus  # noqa: E402
import trre_amd  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from trre_amd import api  # noqa: E402

FAM = {v: k for k, v in trre_amd.KERNEL_NAMES.items()}
SENTINEL = 0xA5
PAD = 1 << 20               # bytes behind the capacity the scan is given: they must come back untouched
SIZES = (130 * 1024, 165 * 1024)
AXYZ, WIDE, BT, LAZY, GEN = "a:xyz", "a(a|b|c){9}c:x", "a(a|b|c|d|e|f|g|h){12}c:x", "(a|b)*a(a|b){18}:x", "[a-z ]*|.*"


def dictionary():
    import dictgen
    keys, vals = dictgen.make_dictionary(1000)
    return dictgen.pattern(keys, vals)


# job -> (the environment on top of test_gpu_handshake.BASE_ENV, [(case, pattern, engine, mode, family forced or None, family expected)])
JOBS = {
    "default": ({}, [("axyz_tile", AXYZ, "dft", "scan", "tile_gen", "tile_gen"),
                     ("axyz_g16", AXYZ, "dft", "scan", None, "stream_gen"),
                     ("dict_mark4_splice", None, "dft", "scan", None, "stream_gen"),
                     ("wide_fwd", WIDE, "nft", "scan", "guided_gen", "guided_gen"),
                     ("backtrack", BT, "nft", "scan", None, "backtrack"),
                     ("lazy", LAZY, "dft", "scan", None, "dft_lazy"),
                     ("generate", GEN, "nft", "match_all", None, "generate")]),
    "no_g16": ({"TRRE_NO_G16": "1"}, [("axyz_direct", AXYZ, "dft", "scan", None, "stream_gen")]),
    "no_mark4": ({"TRRE_NO_FB_MARK4": "1"}, [("dict_mark", None, "dft", "scan", None, "stream_gen")]),
    "fb_emit": ({"TRRE_NO_FB_COPY": "1", "TRRE_FB_EMIT": "1"}, [("dict_fb", None, "dft", "scan", None, "stream_gen")]),
}


def inputs():
    """seeded word soup (tests/corpus.py) of exactly SIZES bytes, the last line without a newline"""
    out = []
    for k, n in enumerate(SIZES):
        d = bytearray(corpus.word_soup(random.Random(41 + k), n + 256)[:n])
        if d[-1] == 0x0A:
            d[-1] = ord("x")
        out.append(bytes(d))
    return out


def oracle(pat, eng, mode, data):
    if mode == "match_all":
        return Oracle(pat, "nft", all_outputs=True).match(data)
    return Oracle(pat, eng).scan(data)


def call(p, src, need, cap):
    """one trre_scan_device call into a sentinel-filled buffer of cap + PAD bytes: (rc, out_len, the first cap bytes, the pad is untouched)"""
    buf = torch.full((cap + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    m = ctypes.c_size_t()
    rc = api.lib().trre_scan_device(p._h, src.data_ptr(), src.numel(), buf.data_ptr(), cap, ctypes.byref(m), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    clean = bool((buf[cap:] == SENTINEL).all())
    return rc, m.value, buf[:min(cap, need)].cpu().numpy().tobytes(), clean


def main(job):
    bad, cases, calls = [], [], 0
    data = inputs()
    for name, pat, eng, mode, forced, expect in JOBS[job][1]:
        pat = pat if pat is not None else dictionary()
        p = trre_amd.Program(pat, eng, mode=mode)
        if forced:
            p.set_kernel(FAM[forced])
        if trre_amd.KERNEL_NAMES[p.info.kernel] != expect:
            bad.append("%s: family %s, not %s" % (name, trre_amd.KERNEL_NAMES[p.info.kernel], expect))
        for d in data:
            want = oracle(pat, eng, mode, d)
            need = len(want)
            src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
            rc, m, got, clean = call(p, src, need, need)
            calls += 1
            print("%s n=%d need=%d: cap=need rc %d out_len %d" % (name, len(d), need, rc, m), file=sys.stderr)
            if rc != 0 or m != need or got != want:
                bad.append("%s n=%d cap=need: rc %d, out_len %d, need %d, bytes equal: %s" % (name, len(d), rc, m, need, got == want))
            if not clean:
                bad.append("%s n=%d cap=need: written behind the capacity" % (name, len(d)))
            rc, m, _, clean = call(p, src, need, need - 1)
            calls += 1
            print("%s n=%d need=%d: cap=need-1 rc %d out_len %d" % (name, len(d), need, rc, m), file=sys.stderr)
            if rc != api.E_CAPACITY or m != need:
                bad.append("%s n=%d cap=need-1: rc %d, out_len %d, need %d" % (name, len(d), rc, m, need))
            if not clean:
                bad.append("%s n=%d cap=need-1: written behind the capacity" % (name, len(d)))
        cases.append(name)
    print("RESULT " + repr({"cases": cases, "calls": calls, "bad": bad[:12]}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
