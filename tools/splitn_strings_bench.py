"""Splitting at the first or last matches only, and field k of that split, against what a caller has to do without them
(include/trre_mi355x.h: trre_splitn_device_strings, trre_fieldn_device_strings against trre_span_device_strings and
trre_split_device_strings plus torch).

On printable lines, with one string per line (~90 bytes) and with 4 KiB strings, prints one JSON line per pattern, form and
case — limit 1 from the front, limit 1 from the end, limit 3 from the front — all calls from the same process under the same
spans program:
  split   the filling split_strings(limit=, from_end=) with exactly the room its size query asked for, against the filling
          span_strings and the slicing in torch: the rule per match from the list offsets, a difference array and its running sum
          for the bytes inside the cutting matches, a boolean index for the output, the kept-byte ranks at the cutting matches'
          ends and the strings' ends for the piece offsets
  field   the filling field_strings(k, limit=, from_end=): k = 0 from the front (the key) and k = -1 from the end (the extension)
          against the filling split_strings and the ragged gather of one piece per string; k = 1 from the front (the value) and
          k = 0 from the end (the stem), which no piece of the unlimited split is, against span_strings and a ragged gather of
          the ranges
Every baseline's result is compared with the call's before anything is timed.  ms per call (median of --steps after --warmup,
host clock around the synchronous call) and GB/s of input.  No threshold is asserted anywhere; DESIGN.md 4.9k has one measured
run.  The time of each pass: run this under `rocprofv3 --kernel-trace --stats -- python tools/splitn_strings_bench.py` (a run of
its own, no counters in it) and read the k_splitn_* and k_fieldn_* rows.

    python tools/splitn_strings_bench.py [--gib 0.5] [--steps 5] [--warmup 1] [--forms line,4KiB] [--patterns ',' ' +']
"""
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

CASES = (("first", 1, False), ("last", 1, True), ("first3", 3, False))


def cutting_matches(lo, limit, from_end):
    """per match of the column: its string, and whether it cuts"""
    counts = lo[1:] - lo[:-1]
    string = torch.repeat_interleave(torch.arange(counts.numel(), device=lo.device), counts)
    r = torch.arange(string.numel(), device=lo.device) - lo[string]
    return string, ((counts[string] - r <= limit) if from_end else (r < limit))


def gather(values, start, length):
    """the ranges values[start[i] : start[i] + length[i]] concatenated, and their offsets"""
    oo = torch.zeros(length.numel() + 1, dtype=torch.int64, device=values.device)
    torch.cumsum(length, 0, out=oo[1:])
    src = torch.repeat_interleave(start - oo[:-1], length) + torch.arange(int(oo[-1].item()), device=values.device)
    return values[src], oo


def split_by_spans(p, values, offs, limit, from_end):
    """what split_strings(limit=, from_end=) returns, from span_strings and torch"""
    st, en, lo = p.span_strings(values, offs)
    string, cuts = cutting_matches(lo, limit, from_end)
    st, en, string = st[cuts], en[cuts], string[cuts]
    n, nrec = values.numel(), offs.numel() - 1
    delta = torch.zeros(n + 1, dtype=torch.int32, device=values.device)
    one = torch.ones(1, dtype=torch.int32, device=values.device)
    delta.index_add_(0, st, one.expand(st.numel()))
    delta.index_add_(0, en, -one.expand(en.numel()))
    keep = torch.cumsum(delta[:n], 0, dtype=torch.int32) == 0
    rank = torch.zeros(n + 1, dtype=torch.int64, device=values.device)
    torch.cumsum(keep, 0, out=rank[1:])
    cut_lo = torch.zeros(nrec + 1, dtype=torch.int64, device=values.device)
    torch.cumsum(torch.bincount(string, minlength=nrec), 0, out=cut_lo[1:])
    list_off = cut_lo + torch.arange(nrec + 1, device=values.device)
    piece_off = torch.zeros(int(list_off[-1].item()) + 1, dtype=torch.int64, device=values.device)
    piece_off[torch.arange(st.numel(), device=values.device) + 1 + string] = rank[en]
    piece_off[list_off[1:]] = rank[offs[1:]]
    return values[keep], piece_off, list_off


def field_by_pieces(p, values, offs, last):
    """piece 0 (the last piece) of every string of the unlimited split: split_strings and a ragged gather"""
    out, po, lo = p.split_strings(values, offs)
    piece = lo[1:] - 1 if last else lo[:-1]
    return gather(out, po[piece], po[piece + 1] - po[piece])


def field_by_spans(p, values, offs, from_end):
    """k = 1 behind the first match (k = 0 in front of the last one): span_strings and a ragged gather; a string without a match
    has no field 1, and is its own field 0"""
    st, en, lo = p.span_strings(values, offs)
    has = lo[1:] > lo[:-1]
    if from_end:
        end = torch.where(has, st[(lo[1:] - 1).clamp(min=0)], offs[1:]) if st.numel() else offs[1:]
        return gather(values, offs[:-1], end - offs[:-1])
    start = torch.where(has, en[lo[:-1].clamp(max=max(en.numel() - 1, 0))], offs[1:]) if en.numel() else offs[1:]
    return gather(values, start, offs[1:] - start)


def same(a, b):
    return all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a, b))


def main():
    ap = column_bench.parser(gib=0.5)
    ap.add_argument("--patterns", nargs="+", default=[",", " +"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(args.gib * (1 << 30))
    stripped, s_off = column_bench.line_column(n, dev)[1:]
    for pattern in args.patterns:
        p = trre_amd.Program(pattern, "nft", "spans")
        for label in args.forms.split(","):
            values, offs = column_bench.form(label, stripped, s_off)
            nrec, nb = offs.numel() - 1, values.numel()
            row = {"pattern": pattern, "strings": label, "nrec": nrec, "string_bytes": nb}
            t_all = timed(lambda: p.split_strings(values, offs), args.steps, args.warmup)
            row["split_strings_ms"] = round(t_all, 3)
            for name, limit, from_end in CASES:
                got = p.split_strings(values, offs, limit=limit, from_end=from_end)
                assert same(got, split_by_spans(p, values, offs, limit, from_end)), (pattern, label, name)
                t_new = timed(lambda: p.split_strings(values, offs, limit=limit, from_end=from_end), args.steps, args.warmup)
                t_old = timed(lambda: split_by_spans(p, values, offs, limit, from_end), args.steps, args.warmup)
                row.update({name + "_pieces": got[1].numel() - 1, name + "_out_bytes": got[0].numel(), name + "_splitn_ms": round(t_new, 3),
                            name + "_spans_torch_ms": round(t_old, 3), name + "_splitn_GBps": round(nb / t_new / 1e6, 1)})
                del got
            fields = (("key", 0, False, lambda: field_by_pieces(p, values, offs, False)),
                      ("ext", -1, True, lambda: field_by_pieces(p, values, offs, True)),
                      ("value", 1, False, lambda: field_by_spans(p, values, offs, False)),
                      ("stem", 0, True, lambda: field_by_spans(p, values, offs, True)))
            for name, k, from_end, old in fields:
                out, oo, valid = p.field_strings(values, offs, k, limit=1, from_end=from_end)
                assert same((out, oo), old()), (pattern, label, name)
                t_new = timed(lambda: p.field_strings(values, offs, k, limit=1, from_end=from_end), args.steps, args.warmup)
                t_old = timed(old, args.steps, args.warmup)
                row.update({name + "_n_valid": int(valid.sum().item()), name + "_out_bytes": out.numel(), name + "_fieldn_ms": round(t_new, 3),
                            name + ("_split_gather_ms" if name in ("key", "ext") else "_spans_torch_ms"): round(t_old, 3),
                            name + "_fieldn_GBps": round(nb / t_new / 1e6, 1)})
                del out, oo, valid
            print(json.dumps(row), flush=True)
        p.close()


if __name__ == "__main__":
    main()
