"""Match k of every string against what a user does without it (include/trre_mi355x.h: trre_nth_device_strings,
trre_find_device_strings).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern and form, all
calls from the same process under the same find program: the find call's size query alone (both scans, the list offsets, no
text stored), and for k = 0, 1 and -1 the filling nth_strings — with exactly the room its own size query asked for — next to the
filling find_strings followed by the ragged gather in torch by list_off + k that picks the same entries out of all the texts.
ms per call (median of --steps after --warmup, host clock around the synchronous call) and GB/s of input.  No speed-up is
promised: the two scans dominate and are the find call's; what the nth call saves is the match-offset array, the memory of every
unselected text and a round trip.  The two results are compared once, before the timing.  DESIGN.md 4.9j has what was measured.
The time of each pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/nth_strings_bench.py` (a run of its own,
no counters in it) and read the k_nth_* rows.

    python tools/nth_strings_bench.py [--gib 2] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns '[0-9]+' '(cat:dog|dog:cat)']
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


def gather(texts, mo, lo, f):
    """entry f of every list out of all the texts, as a user writes it today: (out, out_offsets, valid)"""
    c = lo[1:] - lo[:-1]
    kk = c + f if f < 0 else torch.full_like(c, f)
    valid = (kk >= 0) & (kk < c)
    j = (lo[:-1] + kk)[valid]
    lens = torch.zeros_like(c)
    lens[valid] = mo[j + 1] - mo[j]
    oo = torch.zeros(c.numel() + 1, dtype=torch.int64, device=c.device)
    torch.cumsum(lens, 0, out=oo[1:])
    picked = lens[valid]
    shift = torch.repeat_interleave(mo[j] - oo[:-1][valid], picked)
    out = texts[shift + torch.arange(shift.numel(), dtype=torch.int64, device=c.device)]
    return out, oo, valid


def main():
    ap = column_bench.parser()
    ap.add_argument("--patterns", nargs="+", default=["[0-9]+", "(cat:dog|dog:cat)"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    lib = api.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    stripped, s_off = column_bench.line_column(n, dev)[1:]
    m, k = ctypes.c_size_t(), ctypes.c_size_t()
    for pattern in args.patterns:
        p = trre_amd.Program(pattern, "nft", "find")
        for label in args.forms.split(","):
            values, offs = column_bench.form(label, stripped, s_off)
            nrec, nb = offs.numel() - 1, values.numel()
            lo = torch.empty_like(offs)
            bits = torch.zeros((nrec + 63) // 64, dtype=torch.int64, device=dev)

            def query():
                rc = lib.trre_find_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, None, 0, None, 0, lo.data_ptr(), ctypes.byref(k),
                                                  ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
            query()
            found, need = k.value, m.value
            texts = torch.empty(need + 64, dtype=torch.uint8, device=dev)
            mo = torch.empty(found + 1, dtype=torch.int64, device=dev)
            oo = torch.empty(nrec + 1, dtype=torch.int64, device=dev)
            sizes = {}
            for f in KS:
                rc = lib.trre_nth_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, f, None, 0, None, bits.data_ptr(), ctypes.byref(k),
                                                 ctypes.byref(m), stream)
                assert rc in (0, api.E_CAPACITY), rc
                sizes[f] = (k.value, m.value)
            out = torch.empty(max(s[1] for s in sizes.values()) + 64, dtype=torch.uint8, device=dev)

            def find():
                rc = lib.trre_find_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, texts.data_ptr(), need, mo.data_ptr(), found,
                                                  lo.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                assert rc == 0 and (k.value, m.value) == (found, need), (rc, k.value, m.value)

            def nth(f):
                valid, length = sizes[f]

                def call():
                    rc = lib.trre_nth_device_strings(p._h, values.data_ptr(), nb, offs.data_ptr(), nrec, f, out.data_ptr(), length, oo.data_ptr(),
                                                     bits.data_ptr(), ctypes.byref(k), ctypes.byref(m), stream)
                    assert rc == 0 and (k.value, m.value) == (valid, length), (rc, k.value, m.value)
                return call

            def today(f):
                def call():
                    find()
                    return gather(texts, mo, lo, f)
                return call
            for f in KS:                                     # the same entries either way, once
                nth(f)()
                g_out, g_oo, g_valid = today(f)()
                assert torch.equal(g_oo, oo) and torch.equal(g_out, out[:sizes[f][1]]) and int(g_valid.sum().item()) == sizes[f][0], f
                del g_out, g_oo, g_valid
            t_query = timed(query, args.steps, args.warmup)
            t_find = timed(find, args.steps, args.warmup)
            row = {"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb, "n_matches": found, "find_out_bytes": need,
                   "find_size_query_ms": round(t_query, 3), "find_size_query_GBps": round(nb / t_query / 1e6, 1),
                   "find_strings_ms": round(t_find, 3)}
            for f in KS:
                name = "k_%s" % str(f).replace("-", "m")
                t_nth, t_today = timed(nth(f), args.steps, args.warmup), timed(today(f), args.steps, args.warmup)
                row.update({name + "_n_valid": sizes[f][0], name + "_out_bytes": sizes[f][1], name + "_nth_ms": round(t_nth, 3),
                            name + "_nth_GBps": round(nb / t_nth / 1e6, 1), name + "_find_gather_ms": round(t_today, 3),
                            name + "_find_gather_GBps": round(nb / t_today / 1e6, 1)})
            print(json.dumps(row), flush=True)
            del texts, mo, oo, out, lo, bits
        p.close()


if __name__ == "__main__":
    main()
