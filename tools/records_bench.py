"""Ragged records against the plain scan, 8 GiB resident (include/trre_mi355x.h: trre_scan_device_records).

For '[a:A-z:Z]' on printable lines, 'a:xyz' on printable lines and the 1000-entry dictionary on its soup (DFT engine), with
one record per line and with 4 KiB records, prints one JSON line per case: the plain scan (trre_scan_device) and the records
call on the same buffer, in ms per call (median of --steps after --warmup) and in GB/s of input, and what the records call
adds.  The time of each added pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/records_bench.py` and
read the k_rec_* rows (and k_chunk_scan's extra calls).

    python tools/records_bench.py [--gib 8] [--steps 5] [--warmup 1] [--cases rot,xyz,dict]
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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    keys, vals = dictgen.make_dictionary(1000)
    cases = {"rot": ("[a:A-z:Z]", "printable"), "xyz": ("a:xyz", "printable"), "dict": (dictgen.pattern(keys, vals), "dict1000")}
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    corpus_name, x = None, None
    for key in args.cases.split(","):
        pat, cname = cases[key]
        if cname != corpus_name:
            x = None
            torch.cuda.empty_cache()
            x = corpora.by_name(cname, n, corpora.SEED0 + 7, dev)
            corpus_name = cname
            step = 1 << 30                           # (nonzero over the whole buffer at once is beyond torch's index range)
            per_line = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev)] +
                                 [(x[lo:lo + step] == 10).nonzero().flatten() + (lo + 1) for lo in range(0, n, step)])
            if int(per_line[-1]) != n:
                per_line = torch.cat([per_line, torch.tensor([n], dtype=torch.int64, device=dev)])
            per_4k = torch.cat([torch.arange(0, n, 4096, dtype=torch.int64, device=dev), torch.tensor([n], dtype=torch.int64, device=dev)])
        p = trre_amd.Program(pat, "dft")
        m = ctypes.c_size_t()
        plain_out = p.scan_tensor(x)
        cap = plain_out.numel() + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        del plain_out

        def plain():
            rc = lib.trre_scan_device(p._h, x.data_ptr(), n, out.data_ptr(), cap, ctypes.byref(m), stream)
            assert rc == 0, rc
        ms_plain = timed(plain, args.steps, args.warmup)
        for label, offs in (("line", per_line), ("4KiB", per_4k)):
            oo = torch.empty_like(offs)
            rc = lib.trre_scan_device_records(p._h, x.data_ptr(), n, offs.data_ptr(), offs.numel() - 1, out.data_ptr(), cap,
                                              oo.data_ptr(), ctypes.byref(m), stream)
            if rc == api.E_CAPACITY:                 # records cut inside lines print more than the plain scan
                del out
                cap = m.value + 64
                out = torch.empty(cap, dtype=torch.uint8, device=dev)

            def rec():
                rc = lib.trre_scan_device_records(p._h, x.data_ptr(), n, offs.data_ptr(), offs.numel() - 1, out.data_ptr(), cap,
                                                  oo.data_ptr(), ctypes.byref(m), stream)
                assert rc == 0, rc
            ms_rec = timed(rec, args.steps, args.warmup)
            print(json.dumps({"case": key, "records": label, "nrec": offs.numel() - 1, "bytes": n, "out_bytes": m.value,
                              "kernel": trre_amd.KERNEL_NAMES[p.info.kernel],
                              "plain_ms": round(ms_plain, 3), "records_ms": round(ms_rec, 3), "added_ms": round(ms_rec - ms_plain, 3),
                              "plain_GBps": round(n / ms_plain / 1e6, 1), "records_GBps": round(n / ms_rec / 1e6, 1)}), flush=True)
            del oo
        del out
        p.close()


if __name__ == "__main__":
    main()
