"""Match spans against found strings (include/trre_mi355x.h: trre_span_device_strings, trre_find_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per form, both calls from
the same process under the same pattern: find_strings and span_strings — each the filling call with room, as the second call of
Program.find_strings / span_strings — and the spans' size query (count_strings: no span is stored).  ms per call (median of
--steps after --warmup), GB/s of input, and the ratio.  The span call costs one general guided scan and two streaming passes
over the framed text, the find call two scans, an unframing and a compaction; DESIGN.md 4.9d has what was measured (the two
cost about the same) and where the time goes.  The time of each pass: run this under
`rocprofv3 --kernel-trace --stats -- python tools/span_strings_bench.py` (a run of its own, no counters in it) and read the
k_span_count and k_span_emit rows.

    python tools/span_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--pattern '[0-9]+']
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
    pp = trre_amd.Program(args.pattern, "nft", "spans")
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for label in args.forms.split(","):
        values, offs = column_bench.form(label, stripped, s_off)
        nrec, nb = offs.numel() - 1, values.numel()
        lo = torch.empty_like(offs)
        rc = lib.trre_find_device_strings(pf._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
        assert rc in (0, api.E_CAPACITY), rc
        need, found = m.value, k.value
        rc = lib.trre_span_device_strings(pp._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
        assert rc in (0, api.E_CAPACITY) and k.value == found, (rc, k.value, found)
        out = torch.empty(need + 64, dtype=torch.uint8, device=dev)
        mo = torch.empty(found + 1, dtype=torch.int64, device=dev)
        st = torch.empty(found + 1, dtype=torch.int64, device=dev)
        en = torch.empty(found + 1, dtype=torch.int64, device=dev)

        def find():
            rc = lib.trre_find_device_strings(pf._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), need, mo.data_ptr(), found, lo.data_ptr(),
                                              ctypes.byref(k), ctypes.byref(m), stream)
            assert rc == 0, rc

        def span():
            rc = lib.trre_span_device_strings(pp._h, values.data_ptr(), nb, offs.data_ptr(), nrec, st.data_ptr(), en.data_ptr(), found, lo.data_ptr(),
                                              ctypes.byref(k), stream)
            assert rc == 0, rc

        def count():
            rc = lib.trre_span_device_strings(pp._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
            assert rc in (0, api.E_CAPACITY), rc
        t_find = timed(find, args.steps, args.warmup)
        t_span = timed(span, args.steps, args.warmup)
        t_count = timed(count, args.steps, args.warmup)
        print(json.dumps({"pattern": args.pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found,
                          "find_strings_ms": round(t_find, 3), "span_strings_ms": round(t_span, 3), "count_strings_ms": round(t_count, 3),
                          "span_over_find": round(t_span / t_find, 2), "find_strings_GBps": round(nb / t_find / 1e6, 1),
                          "span_strings_GBps": round(nb / t_span / 1e6, 1), "count_strings_GBps": round(nb / t_count / 1e6, 1)}), flush=True)
        del out, lo, mo, st, en
    pf.close()
    pp.close()


if __name__ == "__main__":
    main()
