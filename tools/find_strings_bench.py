"""Found strings against the strings call (include/trre_mi355x.h: trre_find_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per form, both calls from
the same process: scan_strings (trre_scan_device_strings under a scan-mode program of the same pattern, forced to the general
guided family: the family both scans of the find call run on) and find_strings — the filling call with room, as the second
call of Program.find_strings.  ms per call (median of --steps after --warmup), GB/s of input, and the ratio.  From the code the
find call costs about two general guided scans plus the compaction.  The time of each pass: run this under
`rocprofv3 --kernel-trace --stats -- python tools/find_strings_bench.py` (a run of its own, no counters in it) and read the
k_find_unframe row next to k_str_unframe's.

    python tools/find_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--pattern '[0-9]+']
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
    ap = column_bench.parser()
    ap.add_argument("--pattern", default="[0-9]+")           # every number of the line
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    stripped, s_off = column_bench.line_column(n, dev)[1:]
    pf = trre_amd.Program(args.pattern, "nft", "find")
    ps = trre_amd.Program(args.pattern, "nft")
    ps.set_kernel(trre_amd.KERNEL_GUIDED_GEN)
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for label in args.forms.split(","):
        values, offs = column_bench.form(label, stripped, s_off)
        nrec, nb = offs.numel() - 1, values.numel()
        cap = nb + nrec + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        oo = torch.empty_like(offs)
        lo = torch.empty_like(offs)
        rc = lib.trre_find_device_strings(pf._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
        assert rc in (0, api.E_CAPACITY), rc
        need, found = m.value, k.value
        assert need <= cap
        mo = torch.empty(found + 1, dtype=torch.int64, device=dev)

        def strings():
            rc = lib.trre_scan_device_strings(ps._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), cap, oo.data_ptr(), ctypes.byref(m), stream)
            assert rc == 0, rc

        def find():
            rc = lib.trre_find_device_strings(pf._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), cap, mo.data_ptr(), found, lo.data_ptr(),
                                              ctypes.byref(k), ctypes.byref(m), stream)
            assert rc == 0, rc
        t_scan = timed(strings, args.steps, args.warmup)
        t_find = timed(find, args.steps, args.warmup)
        print(json.dumps({"pattern": args.pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "out_bytes": need,
                          "scan_strings_ms": round(t_scan, 3), "find_strings_ms": round(t_find, 3), "find_over_scan": round(t_find / t_scan, 2),
                          "scan_strings_GBps": round(nb / t_scan / 1e6, 1), "find_strings_GBps": round(nb / t_find / 1e6, 1)}), flush=True)
        del out, oo, lo, mo
    pf.close()
    ps.close()


if __name__ == "__main__":
    main()
