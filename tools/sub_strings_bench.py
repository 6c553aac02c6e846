"""Replaced strings against the calls they are made of and against the replace-all that exists (include/trre_mi355x.h:
trre_sub_device_strings, trre_span_device_strings, trre_find_device_strings, trre_scan_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process: the span call's size query under a spans program of the same pattern; the filling find call under a
find program; the filling scan_strings of the scan-mode program (the replace-all that exists, on whatever family it picks); and
under the sub program the size query and the filling call for (first, count) = (0, -1), (0, 1) and (1, 1) — each filling call
with exactly the room its own size query asked for.  ms per call (median of --steps after --warmup, host clock around the
synchronous call) and GB/s of input.  The sub call is the span call's scan and emit pass, the find call's texts scan and
unframing, two passes over the matches, one over the strings and the splice (k_sub_plan, k_sub_place, k_sub_offsets,
k_sub_emit); DESIGN.md 4.9i has what is expected of it.  (0, -1) is checked against scan_strings byte for
byte.  The time of each pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/sub_strings_bench.py` (a run of
its own, no counters in it) and read the k_sub_* rows.

    python tools/sub_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns ',:;' '[0-9]+:N' 'a:xyz']
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

SELECTIONS = ((0, -1), (0, 1), (1, 1))


def acceptor(pattern):
    """the input side of a pattern of the form P:text"""
    return pattern.rsplit(":", 1)[0]


def main():
    ap = column_bench.parser()
    ap.add_argument("--patterns", nargs="+", default=[",:;", "[0-9]+:N", "a:xyz"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    stripped, s_off = column_bench.line_column(n, dev)[1:]
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for pattern in args.patterns:
        sub, find, scan = (trre_amd.Program(pattern, "nft", mode) for mode in ("sub", "find", "scan"))
        spans = trre_amd.Program(acceptor(pattern), "nft", "spans")
        for label in args.forms.split(","):
            values, offs = column_bench.form(label, stripped, s_off)
            nrec, nb = offs.numel() - 1, values.numel()
            lo = torch.empty_like(offs)
            oo = torch.empty_like(offs)

            def query():
                rc = lib.trre_span_device_strings(spans._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            found = k.value
            rc = lib.trre_find_device_strings(find._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k),
                                              ctypes.byref(m), stream)
            assert rc in (0, api.E_CAPACITY) and k.value == found, (rc, k.value, found)
            texts = m.value
            sizes = {}
            for first, count in SELECTIONS:
                rc = lib.trre_sub_device_strings(sub._h, values.data_ptr(), nb, offs.data_ptr(), nrec, first, count, None, 0, None, ctypes.byref(k),
                                                 ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
                sizes[(first, count)] = (k.value, m.value)
            assert sizes[(0, -1)][0] == found
            room = max(max(s[1] for s in sizes.values()), texts, nb)
            out = torch.empty(room + 64, dtype=torch.uint8, device=dev)
            ref = torch.empty(room + 64, dtype=torch.uint8, device=dev)
            mo = torch.empty(found + 1, dtype=torch.int64, device=dev)

            def found_strings():
                rc = lib.trre_find_device_strings(find._h, values.data_ptr(), nb, offs.data_ptr(), nrec, out.data_ptr(), texts, mo.data_ptr(), found,
                                                  lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (found, texts), (rc, k.value, m.value)

            def scan_strings():
                rc = lib.trre_scan_device_strings(scan._h, values.data_ptr(), nb, offs.data_ptr(), nrec, ref.data_ptr(), room, oo.data_ptr(),
                                                  ctypes.byref(m), stream)
                assert rc == 0 and m.value == sizes[(0, -1)][1], (rc, m.value)

            def sub_query():
                rc = lib.trre_sub_device_strings(sub._h, values.data_ptr(), nb, offs.data_ptr(), nrec, 0, 1, None, 0, None, ctypes.byref(k),
                                                 ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc

            def replaced(sel):
                replaced_n, length = sizes[sel]

                def call():
                    rc = lib.trre_sub_device_strings(sub._h, values.data_ptr(), nb, offs.data_ptr(), nrec, sel[0], sel[1], out.data_ptr(), length,
                                                     lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                    assert rc == 0 and (k.value, m.value) == (replaced_n, length), (rc, k.value, m.value)
                return call
            t_query = timed(query, args.steps, args.warmup)
            t_find = timed(found_strings, args.steps, args.warmup)
            t_scan = timed(scan_strings, args.steps, args.warmup)
            t_sub_query = timed(sub_query, args.steps, args.warmup)
            t_sub = {}
            for sel in SELECTIONS:
                t_sub[sel] = timed(replaced(sel), args.steps, args.warmup)
                if sel == (0, -1):                   # the identity: every match replaced is the plain scan
                    length = sizes[sel][1]
                    assert torch.equal(out[:length], ref[:length]) and torch.equal(lo, oo), pattern
            row = {"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "texts_bytes": texts,
                   "span_size_query_ms": round(t_query, 3), "find_strings_ms": round(t_find, 3), "scan_strings_ms": round(t_scan, 3),
                   "scan_kernel": trre_amd.KERNEL_NAMES.get(scan.info.kernel, scan.info.kernel), "sub_size_query_ms": round(t_sub_query, 3)}
            for sel in SELECTIONS:
                name = "sub_%d_%s" % (sel[0], "all" if sel[1] < 0 else sel[1])
                row.update({name + "_replaced": sizes[sel][0], name + "_out_bytes": sizes[sel][1], name + "_ms": round(t_sub[sel], 3),
                            name + "_GBps": round(nb / t_sub[sel] / 1e6, 1)})
            print(json.dumps(row), flush=True)
            del out, ref, mo, lo, oo
        for p in (sub, find, scan, spans):
            p.close()


if __name__ == "__main__":
    main()
