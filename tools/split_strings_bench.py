"""Split strings against match spans (include/trre_mi355x.h: trre_split_device_strings, trre_span_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process under the same spans program: span_strings and split_strings — each the filling call with room, as
the second call of Program.span_strings / split_strings — and the split's size query (null pointers: the list offsets alone).
ms per call (median of --steps after --warmup, host clock around the synchronous call), GB/s of input, and the ratio.  The split
call is the span call's passes up to the totals, one more read of the framed text (k_split_count) and a compaction that writes
the kept bytes (k_split_emit) where the span call stores two words per match; DESIGN.md 4.9f has what was measured.  The time of
each pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/split_strings_bench.py` (a run of its own, no
counters in it) and read the k_split_count and k_split_emit rows.

    python tools/split_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns '[0-9]+' ',']
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
    ap.add_argument("--patterns", nargs="+", default=["[0-9]+", ","])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    stripped, s_off = column_bench.line_column(n, dev)[1:]
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for pattern in args.patterns:
        p = trre_amd.Program(pattern, "nft", "spans")
        for label in args.forms.split(","):
            values, offs = column_bench.form(label, stripped, s_off)
            nrec, nb = offs.numel() - 1, values.numel()
            lo = torch.empty_like(offs)

            def query():
                rc = lib.trre_split_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k),
                                                   ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            need, pieces = m.value, k.value
            found = pieces - nrec
            out = torch.empty(need + 64, dtype=torch.uint8, device=dev)
            po = torch.empty(pieces + 1, dtype=torch.int64, device=dev)
            st = torch.empty(found + 1, dtype=torch.int64, device=dev)
            en = torch.empty(found + 1, dtype=torch.int64, device=dev)

            def span():
                rc = lib.trre_span_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, st.data_ptr(), en.data_ptr(), found, lo.data_ptr(),
                                                  ctypes.byref(k), stream)
                assert rc == 0 and k.value == found, (rc, k.value, found)

            def split():
                rc = lib.trre_split_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), need, po.data_ptr(), pieces,
                                                   lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (pieces, need), (rc, k.value, m.value)
            t_span = timed(span, args.steps, args.warmup)
            t_split = timed(split, args.steps, args.warmup)
            t_query = timed(query, args.steps, args.warmup)
            # the kept bytes are the input minus the matched ones
            assert need == nb - int((en[:found] - st[:found]).sum().item()), (need, nb)
            print(json.dumps({"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "n_pieces": pieces,
                              "out_bytes": need, "span_strings_ms": round(t_span, 3), "split_strings_ms": round(t_split, 3),
                              "split_query_ms": round(t_query, 3), "split_over_span": round(t_split / t_span, 2),
                              "span_strings_GBps": round(nb / t_span / 1e6, 1), "split_strings_GBps": round(nb / t_split / 1e6, 1),
                              "split_query_GBps": round(nb / t_query / 1e6, 1)}), flush=True)
            del out, lo, po, st, en
        p.close()


if __name__ == "__main__":
    main()
