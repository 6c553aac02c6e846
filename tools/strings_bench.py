"""Packed strings against the plain scan and the records call, 8 GiB resident (include/trre_mi355x.h: trre_scan_device_strings).

For '[a:A-z:Z]' on printable lines, 'a:xyz' on printable lines and the 1000-entry dictionary on its soup (DFT engine), with
one string per line and with 4 KiB strings, prints one JSON line per case, all three from the same process: the plain scan
of the newline-terminated text (trre_scan_device), the records call on that same text (the existing path, the yardstick) and
the strings call on the strings themselves (one per line: the text without its newlines; 4 KiB: the text cut every 4096
bytes) — ms per call (median of --steps after --warmup) and GB/s of input.  The time of each added pass: run this under
`rocprofv3 --kernel-trace --stats -- python tools/strings_bench.py` and read the k_str_* rows next to k_rec_stage's.

    python tools/strings_bench.py [--gib 8] [--steps 5] [--warmup 1] [--cases rot,xyz,dict] [--forms line,4KiB]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import corpora  # noqa: E402
import dictgen  # noqa: E402
import trre_amd  # noqa: E402
from column_bench import timed  # noqa: E402
from trre_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="rot,xyz,dict")
    ap.add_argument("--forms", default="line,4KiB")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    keys, vals = dictgen.make_dictionary(1000)
    cases = {"rot": ("[a:A-z:Z]", "printable"), "xyz": ("a:xyz", "printable"), "dict": (dictgen.pattern(keys, vals), "dict1000")}
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    corpus_name = None
    for key in args.cases.split(","):
        pat, cname = cases[key]
        if cname != corpus_name:
            x = forms = None
            torch.cuda.empty_cache()
            x = corpora.by_name(cname, n, corpora.SEED0 + 7, dev)
            corpus_name = cname
            step = 1 << 30                           # (nonzero over the whole buffer at once is beyond torch's index range)
            ends = torch.cat([(x[lo:lo + step] == 10).nonzero().flatten() + (lo + 1) for lo in range(0, n, step)])
            if ends.numel() == 0 or int(ends[-1]) != n:
                ends = torch.cat([ends, torch.tensor([n], dtype=torch.int64, device=dev)])
            zero = torch.zeros(1, dtype=torch.int64, device=dev)
            stripped = torch.cat([x[lo:lo + step][x[lo:lo + step] != 10] for lo in range(0, n, step)])
            nl_before = torch.cat([(x[lo:lo + step] == 10).sum().reshape(1) for lo in range(0, n, step)]).sum()
            assert stripped.numel() == n - int(nl_before)
            # string i's end in the stripped text: its line's end minus the newlines up to it (a last line without one counts none)
            idx = torch.arange(1, ends.numel() + 1, dtype=torch.int64, device=dev)
            s_ends = ends - torch.minimum(idx, nl_before)
            per_4k = torch.cat([torch.arange(0, n, 4096, dtype=torch.int64, device=dev), torch.tensor([n], dtype=torch.int64, device=dev)])
            # label: (records input, records offsets, strings input, strings offsets)
            forms = {"line": (x, torch.cat([zero, ends]), stripped, torch.cat([zero, s_ends])), "4KiB": (x, per_4k, x, per_4k)}
            del ends, idx, s_ends
        p = trre_amd.Program(pat, "dft")
        m = ctypes.c_size_t()
        cap = p.scan_tensor(x).numel() + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)

        def plain():
            rc = lib.trre_scan_device(p._h, x.data_ptr(), n, out.data_ptr(), cap, ctypes.byref(m), stream)
            assert rc == 0, rc
        ms_plain = timed(plain, args.steps, args.warmup)
        for label in args.forms.split(","):
            rin, roff, sin, soff = forms[label]
            oo = torch.empty_like(roff)
            res = {}
            for name, f, vin, voff in (("records", lib.trre_scan_device_records, rin, roff), ("strings", lib.trre_scan_device_strings, sin, soff)):
                call_args = (p._h, vin.data_ptr(), vin.numel(), voff.data_ptr(), voff.numel() - 1)
                rc = f(*call_args, out.data_ptr(), cap, oo.data_ptr(), ctypes.byref(m), stream)
                if rc == api.E_CAPACITY:             # records cut inside lines print more than the plain scan
                    del out
                    cap = m.value + 64
                    out = torch.empty(cap, dtype=torch.uint8, device=dev)

                def call():
                    rc = f(*call_args, out.data_ptr(), cap, oo.data_ptr(), ctypes.byref(m), stream)
                    assert rc == 0, rc
                res[name] = (timed(call, args.steps, args.warmup), vin.numel(), m.value)
            (ms_rec, n_rec, _), (ms_str, n_str, m_str) = res["records"], res["strings"]
            print(json.dumps({"case": key, "strings": label, "nrec": roff.numel() - 1, "bytes": n, "string_bytes": n_str, "out_bytes": m_str,
                              "kernel": trre_amd.KERNEL_NAMES[p.info.kernel],
                              "plain_ms": round(ms_plain, 3), "records_ms": round(ms_rec, 3), "strings_ms": round(ms_str, 3),
                              "strings_over_records": round(ms_str / ms_rec, 3),
                              "plain_GBps": round(n / ms_plain / 1e6, 1), "records_GBps": round(n_rec / ms_rec / 1e6, 1),
                              "strings_GBps": round(n_str / ms_str / 1e6, 1)}), flush=True)
            del oo
        del out
        p.close()


if __name__ == "__main__":
    main()
