"""What the benches of the column calls share (tools/{match,find,span,split,filter,field}_strings_bench.py; `timed` also serves
records_bench.py and strings_bench.py): the common flags, the timing loop, and printable lines as a column of strings in the two
forms the benches measure — one string per line (~90 bytes) and 4 KiB strings."""
import argparse
import statistics
import time

import torch

import corpora


def parser(gib=2.0):
    """--gib, --steps, --warmup and --forms; a bench adds its own pattern flag"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=gib)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", default="line,4KiB")
    return ap


def timed(fn, steps, warmup):
    """ms per call of fn: the median of `steps` calls after `warmup`, host clock around the synchronous call"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def line_column(n, dev):
    """n bytes of printable lines, one string per line: (the text, the strings without their newlines, their offsets)"""
    x = corpora.printable_lines(n, corpora.SEED0 + 7, dev)
    step = 1 << 30                                   # (nonzero over the whole buffer at once is beyond torch's index range)
    ends = torch.cat([(x[lo:lo + step] == 10).nonzero().flatten() + (lo + 1) for lo in range(0, n, step)])
    stripped = torch.cat([x[lo:lo + step][x[lo:lo + step] != 10] for lo in range(0, n, step)])
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    s_off = torch.cat([zero, ends - torch.arange(1, ends.numel() + 1, dtype=torch.int64, device=dev)])
    return x, stripped, s_off


def form(label, stripped, s_off):
    """the column in the form `label`: "line", the strings as they are; else whole 4 KiB strings: (values, offsets)"""
    if label == "line":
        return stripped, s_off
    rows = stripped.numel() // 4096
    return stripped[:rows * 4096], torch.arange(0, rows * 4096 + 1, 4096, dtype=torch.int64, device=stripped.device)
