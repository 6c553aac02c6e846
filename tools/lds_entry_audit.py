#!/usr/bin/env python3
"""Audit of a gfx950 assembly listing (hipcc -S --cuda-device-only): LDS that is read before the kernel's first barrier after somebody
was asked to fill it.  tools/barrier_audit.py looks at the barriers that exist; this one looks for the barrier that is missing at a kernel's
entry: tables staged into LDS by all threads and read by the first phase with no s_barrier in between (k_mapgen, DESIGN.md 4.5c: a workgroup
whose other waves were late counted its first tile from what the workgroup before it on that CU had left in LDS).

For every kernel: the control-flow graph is walked FORWARD from the entry with one bit, "an LDS write has been seen" (ds_write*, a DS atomic,
a global / buffer load with the `lds` modifier).  A path ends at its first s_barrier.  A ds_read* reached with the bit set is a finding.
A thread that reads LDS before any write (its own scratch, a value from the launch before: none here) is not.  No allow-list.

    python tools/lds_entry_audit.py listing.s      prints the findings by kernel, then `early LDS reads: N`; exit status 0 either way
"""
import re
import sys

LDS_WRITE = re.compile(r"ds_(write|add|sub|rsub|or|and|xor|max|min|inc|dec|mskor|wrxchg|wrap|cmpst|cmpswap|pk_add|append|consume)"
                       r"|(buffer|global)_load\w*\s.*\blds\b")
BRANCH = re.compile(r"s_c?branch\w*\s+(\.LBB\d+_\d+)")


def functions(text):
    """{name: lines} of the listing's functions: from `_Z..:` to its .Lfunc_end (one kernel's blocks never run into the next's)"""
    funcs, cur, name = {}, [], None
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            if name:
                funcs[name] = cur
            name, cur = m.group(1), []
        elif name is not None:
            if ln.strip().startswith(".Lfunc_end"):
                funcs[name] = cur
                name = None
                continue
            cur.append(ln)
    if name:
        funcs[name] = cur
    return funcs


def blocks_of(lines):
    """basic blocks by label (the block splitting of barrier_audit.py) and the block each falls through to (None: it does not)"""
    blocks, order = {}, []
    lbl, cur = "<entry>", []
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks[lbl] = cur
            order.append(lbl)
            lbl, cur = m.group(1), []
            continue
        t = ln.strip()
        if not t or t.startswith(";") or t.startswith("."):
            continue
        cur.append(t.split(";")[0].strip())
    blocks[lbl] = cur
    order.append(lbl)
    falls = {}
    for i, b in enumerate(order):
        ins = blocks[b]
        ends = bool(ins) and (ins[-1].startswith("s_branch") or ins[-1].startswith("s_endpgm") or ins[-1].startswith("s_setpc"))
        falls[b] = order[i + 1] if not ends and i + 1 < len(order) else None
    return blocks, falls


def early_reads(lines):
    """[(block, instruction)]: every ds_read a path from the entry reaches after an LDS write and before a barrier (one per block)"""
    blocks, falls = blocks_of(lines)
    seen, stack, hits = set(), [("<entry>", False)], []
    while stack:
        b, wrote = stack.pop()
        if (b, wrote) in seen:
            continue
        seen.add((b, wrote))
        out = []                            # (a branch leaves its block with the bit as it is at the branch)
        stop = False
        for t in blocks[b]:
            if t.startswith("s_barrier"):
                stop = True
                break
            if LDS_WRITE.match(t):
                wrote = True
            elif t.startswith("ds_read") and wrote:
                hits.append((b, t))
                stop = True
                break
            m = BRANCH.match(t)
            if m and m.group(1) in blocks:
                out.append((m.group(1), wrote))
        stack.extend(out)
        if not stop and falls[b]:
            stack.append((falls[b], wrote))
    return sorted(set(hits))


def audit(path):
    """{kernel: [(block, instruction)]} for every kernel of the listing, clean ones with an empty list"""
    with open(path) as f:
        return {name: early_reads(lines) for name, lines in functions(f.read()).items()}


def main(argv):
    n = 0
    for name, hits in audit(argv[1]).items():
        for b, t in hits:
            n += 1
            print(name[:90], b, t)
    print("early LDS reads:", n)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
