"""Field k of every string against the span call's size query, the split call and the filter call (include/trre_mi355x.h:
trre_field_device_strings, trre_span_device_strings, trre_split_device_strings, trre_filter_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process under the same spans program: the span call's size query (what Program.count_strings runs: the list
offsets alone), the filling split_strings, the filling filter_strings, and the filling field_strings for k = 0, 1 and -1 — each
with exactly the room its own size query asked for.  ms per call (median of --steps after --warmup, host clock around the
synchronous call), GB/s of input, and what each adds over the size query of the same process.  The field call is the size
query's passes, a pass over the strings (k_field_init), one more read of the framed text (k_field_pick), a count pass that reads
offsets and bounds only (k_filter_part, k_field_count) and a compaction that reads the input once and writes the fields alone as
whole 16-byte vectors (k_field_emit); DESIGN.md 4.9h has what was expected and what was measured.  n_valid is checked against the
counts.  The time of each pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/field_strings_bench.py` (a run
of its own, no counters in it) and read the k_field_* rows.

    python tools/field_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns ',' '[0-9]+']
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

KS = (0, 1, -1)


def main():
    ap = column_bench.parser()
    ap.add_argument("--patterns", nargs="+", default=[",", "[0-9]+"])
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
            bits = torch.zeros((nrec + 63) // 64, dtype=torch.int64, device=dev)

            def query():
                rc = lib.trre_span_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            found = k.value
            counts = lo[1:] - lo[:-1]
            sizes = {}
            for f in KS:
                rc = lib.trre_field_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, f, None, 0, None, bits.data_ptr(), ctypes.byref(k),
                                                   ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
                # n_valid against the counts: field f >= 0 needs f matches, field f < 0 needs -f - 1
                assert k.value == int((counts >= (f if f >= 0 else -f - 1)).sum().item()), (f, k.value)
                sizes[f] = (k.value, m.value)
            rc = lib.trre_filter_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, 0, None, 0, None, None, 0, ctypes.byref(k),
                                                ctypes.byref(m), stream)
            assert rc in (0, api.E_CAPACITY), rc
            kept, kept_bytes = k.value, m.value
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

            def filt():
                rc = lib.trre_filter_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, 0, out.data_ptr() if kept_bytes else None,
                                                    kept_bytes, oo.data_ptr() if kept else None, rw.data_ptr() if kept else None, kept,
                                                    ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (kept, kept_bytes), (rc, k.value, m.value)

            def field(f):
                valid, length = sizes[f]

                def call():
                    rc = lib.trre_field_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, f, out.data_ptr(), length, oo.data_ptr(),
                                                       bits.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                    assert rc == 0 and (k.value, m.value) == (valid, length), (rc, k.value, m.value)
                return call
            t_query = timed(query, args.steps, args.warmup)
            t_split = timed(split, args.steps, args.warmup)
            t_filter = timed(filt, args.steps, args.warmup)
            t_field = {f: timed(field(f), args.steps, args.warmup) for f in KS}
            row = {"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "split_out_bytes": need,
                   "filter_out_bytes": kept_bytes, "size_query_ms": round(t_query, 3), "split_strings_ms": round(t_split, 3),
                   "filter_strings_ms": round(t_filter, 3), "split_adds_ms": round(t_split - t_query, 3),
                   "filter_adds_ms": round(t_filter - t_query, 3)}
            for f in KS:
                name = "field_%s" % str(f).replace("-", "m")
                row.update({name + "_n_valid": sizes[f][0], name + "_out_bytes": sizes[f][1], name + "_ms": round(t_field[f], 3),
                            name + "_adds_ms": round(t_field[f] - t_query, 3), name + "_GBps": round(nb / t_field[f] / 1e6, 1)})
            print(json.dumps(row), flush=True)
            del out, lo, po, oo, rw, bits
        p.close()


if __name__ == "__main__":
    main()
