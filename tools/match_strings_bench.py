"""Matched strings against the plain match scan and the strings call, 8 GiB resident (include/trre_mi355x.h: trre_match_device_strings).

On printable lines, with one string per line and with 4 KiB strings, prints one JSON line per form, all calls from the same
process: the plain match scan of the newline-joined text (trre_scan_device, match mode), the new call on the strings
themselves, and — the yardstick — the plain scan and the strings call (trre_scan_device_strings) under a scan-mode program of
the same guided family on the same strings.  ms per call (median of --steps after --warmup), GB/s of input, and what each of
the two string calls adds to its plain scan.  The time of each added pass: run this under
`rocprofv3 --kernel-trace --stats -- python tools/match_strings_bench.py` (a run of its own, no counters in it) and read the
k_match_* rows next to k_str_stage's.

    python tools/match_strings_bench.py [--gib 8] [--steps 5] [--warmup 1] [--forms line,4KiB] [--pattern '[a:A-m:M].*']
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import column_bench  # noqa: E402
import trre_amd  # noqa: E402
from column_bench import timed  # noqa: E402
from trre_amd import api  # noqa: E402


def main():
    ap = column_bench.parser(gib=8.0)
    ap.add_argument("--pattern", default="[a:A-m:M].*")      # accepts the lines that start with a..m: about a third of the printable ones
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    x, stripped, s_off = column_bench.line_column(n, dev)
    pm = trre_amd.Program(args.pattern, "nft", "match")
    ps = trre_amd.Program(args.pattern, "nft")
    ps.set_kernel(trre_amd.KERNEL_GUIDED_GEN)                # the family match mode runs on
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for label in args.forms.split(","):
        values, offs = column_bench.form(label, stripped, s_off)
        nrec = offs.numel() - 1
        if label == "line":
            joined = x
        else:
            joined = torch.cat([values.view(nrec, 4096), torch.full((nrec, 1), 10, dtype=torch.uint8, device=dev)], dim=1).flatten()
        cap = joined.numel() + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        oo = torch.empty_like(offs)
        valid = torch.zeros((nrec + 63) // 64, dtype=torch.int64, device=dev)
        res = {}

        def plain(p):
            rc = lib.trre_scan_device(p._h, joined.data_ptr(), joined.numel(), out.data_ptr(), cap, ctypes.byref(m), stream)
            assert rc == 0, rc

        def strings():
            rc = lib.trre_scan_device_strings(ps._h, values.data_ptr(), values.numel(), offs.data_ptr(), nrec, out.data_ptr(), cap, oo.data_ptr(),
                                              ctypes.byref(m), stream)
            assert rc == 0, rc

        def match():
            rc = lib.trre_match_device_strings(pm._h, values.data_ptr(), values.numel(), offs.data_ptr(), nrec, out.data_ptr(), cap, oo.data_ptr(),
                                               valid.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
            assert rc == 0, rc
        res["plain_match"] = timed(lambda: plain(pm), args.steps, args.warmup)
        res["match_strings"] = timed(match, args.steps, args.warmup)
        m_match, n_matched = m.value, k.value
        res["plain_scan"] = timed(lambda: plain(ps), args.steps, args.warmup)
        res["scan_strings"] = timed(strings, args.steps, args.warmup)
        nb = values.numel()
        print(json.dumps({"pattern": args.pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matched": n_matched, "out_bytes": m_match,
                          "plain_match_ms": round(res["plain_match"], 3), "match_strings_ms": round(res["match_strings"], 3),
                          "plain_scan_ms": round(res["plain_scan"], 3), "scan_strings_ms": round(res["scan_strings"], 3),
                          "match_adds_ms": round(res["match_strings"] - res["plain_match"], 3),
                          "strings_adds_ms": round(res["scan_strings"] - res["plain_scan"], 3),
                          "plain_match_GBps": round(joined.numel() / res["plain_match"] / 1e6, 1),
                          "match_strings_GBps": round(nb / res["match_strings"] / 1e6, 1),
                          "scan_strings_GBps": round(nb / res["scan_strings"] / 1e6, 1)}), flush=True)
        del out, oo, valid, joined
    pm.close()
    ps.close()


if __name__ == "__main__":
    main()
