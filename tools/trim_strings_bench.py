"""Trimmed strings against the span call's size query, the field call with k = 0 and what a user writes without the call
(include/trre_mi355x.h: trre_trim_device_strings, trre_span_device_strings, trre_field_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process under the same spans program: the span call's size query; the filling field_strings with k = 0 (the
same count and emit passes, another way to the bounds); the filling trim_strings for each side, with exactly the room its own size
query asked for; trim_ranges (one call, no output); and the form without the call: span_strings (its size query and its filling
call), the comparison of every string's first and last two matches with its offsets, and a ragged gather, in torch.  Before
anything is timed the torch form and the call are held against each other byte for byte, for every side.  ms per call (median of
--steps after --warmup, host clock around the synchronous call) and what each adds over the size query of the same process.
DESIGN.md 4.9l has what was expected and what was measured.  The time of each pass: run this under `rocprofv3 --kernel-trace
--stats -- python tools/trim_strings_bench.py` (a run of its own, no counters in it) and read the k_trim_* and k_field_* rows.

    python tools/trim_strings_bench.py [--gib 1] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns ' +' '[0-9]+']
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

SIDES = (("left", api.TRIM_LEFT), ("right", api.TRIM_RIGHT), ("both", api.TRIM_LEFT | api.TRIM_RIGHT))


def torch_form(p, values, offs, flags):
    """the trim without the call: (out, out_offsets, begin, end) from span_strings, comparisons and a ragged gather"""
    st, en, lo = p.span_strings(values, offs)
    s, e = offs[:-1], offs[1:]
    c = lo[1:] - lo[:-1]
    begin, end = s, e
    if st.numel():
        if flags & api.TRIM_LEFT:
            j = lo[:-1].clamp(max=st.numel() - 1)
            begin = torch.where((c > 0) & (st[j] == s), en[j], s)
        if flags & api.TRIM_RIGHT:
            j1 = (lo[1:] - 1).clamp(min=0)
            hit1 = (c > 0) & (en[j1] == e)
            end = torch.where(hit1, st[j1], e)
            j2 = (lo[1:] - 2).clamp(min=0)
            end = torch.where(hit1 & (c > 1) & (en[j2] == e), torch.minimum(end, st[j2]), end)
        end = torch.maximum(begin, end)
    length = end - begin
    oo = torch.zeros(offs.numel(), dtype=torch.int64, device=offs.device)
    torch.cumsum(length, 0, out=oo[1:])
    total = int(oo[-1].item())
    src = torch.arange(total, dtype=torch.int64, device=offs.device) + torch.repeat_interleave(begin - oo[:-1], length, output_size=total)
    return values[src], oo, begin, end


def main():
    ap = column_bench.parser(gib=1.0)
    ap.add_argument("--patterns", nargs="+", default=[" +", "[0-9]+"])
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
            out = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
            oo = torch.empty(nrec + 1, dtype=torch.int64, device=dev)

            def query():
                rc = lib.trre_span_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, None, 0, lo.data_ptr(), ctypes.byref(k), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            found = k.value
            # the call and the torch form, byte for byte, before anything is timed
            sizes, changed = {}, {}
            for side, flags in SIDES:
                got_out, got_oo = p.trim_strings(values, offs, side)
                got_begin, got_end = p.trim_ranges(values, offs, side)
                t_out, t_oo, t_begin, t_end = torch_form(p, values, offs, flags)
                assert torch.equal(got_oo, t_oo) and torch.equal(got_begin, t_begin) and torch.equal(got_end, t_end), (pattern, label, side)
                assert torch.equal(got_out, t_out), (pattern, label, side)
                sizes[side] = got_out.numel()
                changed[side] = int(((got_begin != offs[:-1]) | (got_end != offs[1:])).sum().item())
                del got_out, got_oo, got_begin, got_end, t_out, t_oo, t_begin, t_end
            rc = lib.trre_field_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, 0, None, 0, None, bits.data_ptr(), ctypes.byref(k),
                                               ctypes.byref(m), stream)
            assert rc in (0, api.E_CAPACITY), rc
            field_valid, field_bytes = k.value, m.value

            def field0():
                rc = lib.trre_field_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, 0, out.data_ptr(), field_bytes, oo.data_ptr(),
                                                   bits.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (field_valid, field_bytes), (rc, k.value, m.value)

            def trim(side, flags):
                def call():
                    rc = lib.trre_trim_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, flags, out.data_ptr(), sizes[side],
                                                      oo.data_ptr(), None, None, ctypes.byref(m), stream)
                    assert rc == 0 and m.value == sizes[side], (rc, m.value)
                return call

            t_query = timed(query, args.steps, args.warmup)
            t_field = timed(field0, args.steps, args.warmup)
            t_trim = {side: timed(trim(side, flags), args.steps, args.warmup) for side, flags in SIDES}
            t_ranges = timed(lambda: p.trim_ranges(values, offs, "both"), args.steps, args.warmup)
            t_torch = timed(lambda: torch_form(p, values, offs, api.TRIM_LEFT | api.TRIM_RIGHT), args.steps, args.warmup)
            row = {"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "size_query_ms": round(t_query, 3),
                   "field_0_out_bytes": field_bytes, "field_0_ms": round(t_field, 3), "field_0_adds_ms": round(t_field - t_query, 3)}
            for side, _ in SIDES:
                row.update({"trim_%s_changed" % side: changed[side], "trim_%s_out_bytes" % side: sizes[side],
                            "trim_%s_ms" % side: round(t_trim[side], 3), "trim_%s_adds_ms" % side: round(t_trim[side] - t_query, 3)})
            row.update({"trim_ranges_both_ms": round(t_ranges, 3), "trim_ranges_both_adds_ms": round(t_ranges - t_query, 3),
                        "span_strings_and_torch_both_ms": round(t_torch, 3)})
            print(json.dumps(row), flush=True)
            del out, lo, oo, bits
        p.close()


if __name__ == "__main__":
    main()
