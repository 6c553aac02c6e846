"""Filtered strings against the span call's size query and the split call (include/trre_mi355x.h: trre_filter_device_strings,
trre_span_device_strings, trre_split_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process under the same spans program: the span call's size query (what Program.count_strings runs: the list
offsets alone), the filling split_strings, and the filling filter_strings plain and inverted — each with exactly the room its own
size query asked for.  ms per call (median of --steps after --warmup, host clock around the synchronous call), GB/s of input, and
what the filter and the split add over the size query of the same process.  The filter call is the size query's passes, a count
pass that reads the offsets and the list offsets only (k_filter_part, k_filter_count) and a compaction that reads the input once
and writes the kept strings as whole 16-byte vectors (k_filter_emit); DESIGN.md 4.9g has what was expected and what was
measured.  n_kept and out_len are checked against the counts.  The time of each pass: run this under `rocprofv3 --kernel-trace
--stats -- python tools/filter_strings_bench.py` (a run of its own, no counters in it) and read the k_filter_* rows.

    python tools/filter_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns '[0-9]+' ',']
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
                rc = lib.trre_span_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            found = k.value
            hit = (lo[1:] - lo[:-1]) > 0
            lengths = offs[1:] - offs[:-1]
            sizes = {}
            for invert in (0, 1):
                sel = ~hit if invert else hit
                rc = lib.trre_filter_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, invert, None, 0, None, None, 0, ctypes.byref(k),
                                                    ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
                # n_kept and out_len against the counts
                assert (k.value, m.value) == (int(sel.sum().item()), int(lengths[sel].sum().item())), (invert, k.value, m.value)
                sizes[invert] = (k.value, m.value)
            rc = lib.trre_split_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k),
                                               ctypes.byref(m), stream)
            assert rc in (0, api.E_CAPACITY), rc
            pieces, need = k.value, m.value
            out = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
            po = torch.empty(pieces + 1, dtype=torch.int64, device=dev)
            oo = torch.empty(nrec + 1, dtype=torch.int64, device=dev)
            rw = torch.empty(nrec + 1, dtype=torch.int64, device=dev)

            def split():
                rc = lib.trre_split_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), need, po.data_ptr(), pieces,
                                                   lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (pieces, need), (rc, k.value, m.value)

            def filt(invert):
                kept, length = sizes[invert]

                def call():
                    rc = lib.trre_filter_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, invert, out.data_ptr() if length else None,
                                                        length, oo.data_ptr() if kept else None, rw.data_ptr() if kept else None, kept,
                                                        ctypes.byref(k), ctypes.byref(m), stream)
                    assert rc == 0 and (k.value, m.value) == (kept, length), (rc, k.value, m.value)
                return call
            t_query = timed(query, args.steps, args.warmup)
            t_split = timed(split, args.steps, args.warmup)
            t_filter = timed(filt(0), args.steps, args.warmup)
            t_invert = timed(filt(1), args.steps, args.warmup)
            print(json.dumps({"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found,
                              "n_kept": sizes[0][0], "out_bytes": sizes[0][1], "n_kept_inverted": sizes[1][0], "out_bytes_inverted": sizes[1][1],
                              "size_query_ms": round(t_query, 3), "split_strings_ms": round(t_split, 3), "filter_strings_ms": round(t_filter, 3),
                              "filter_inverted_ms": round(t_invert, 3), "split_adds_ms": round(t_split - t_query, 3),
                              "filter_adds_ms": round(t_filter - t_query, 3), "filter_inverted_adds_ms": round(t_invert - t_query, 3),
                              "size_query_GBps": round(nb / t_query / 1e6, 1), "filter_strings_GBps": round(nb / t_filter / 1e6, 1)}), flush=True)
            del out, lo, po, oo, rw
        p.close()


if __name__ == "__main__":
    main()
