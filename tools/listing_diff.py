#!/usr/bin/env python3
"""Two gfx950 assembly listings (hipcc -S --cuda-device-only, as tests/test_lds_audit.py's listing() builds them) compared kernel by
kernel: for a refactor that must leave the device code as it is.

    python tools/listing_diff.py OLD.s NEW.s

For every kernel in both listings: `identical` when the instruction text is the same — comments and assembler directives dropped, the
function's number taken out of its block labels (.LBB12_3 -> .LBB_3: a template more or less renumbers them) —, else `differs` with
each side's next_free_vgpr, next_free_sgpr, group_segment_fixed_size (LDS), private_segment_fixed_size (scratch) and instruction
count.  Then the kernels in one listing only.  The text and these numbers are all it looks at.  Exit status 0 either way."""
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{name: (instruction lines, {field: value})} of the listing's kernels: the functions that have an .amdhsa_kernel block"""
    with open(path) as f:
        text = f.read()
    out, name, body, meta, in_meta = {}, None, [], {}, False
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body, meta, in_meta = m.group(1), [], {}, False
            continue
        if name is None:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            if meta:
                out[name] = (body, meta)
            name = None
        elif s.startswith(".amdhsa_kernel"):
            in_meta = True
        elif s.startswith(".end_amdhsa_kernel"):
            in_meta = False
        elif in_meta:
            key, _, value = s.partition(" ")
            if key[len(".amdhsa_"):] in FIELDS:
                meta[key[len(".amdhsa_"):]] = int(value)
        elif s and (not s.startswith(".") or s.endswith(":")):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def n_instructions(body):
    return sum(1 for s in body if not s.endswith(":"))


def compare(old_path, new_path):
    """(lines to print, number of kernels that differ, names in one listing only)"""
    old, new = kernels(old_path), kernels(new_path)
    lines, differing = [], 0
    for name in sorted(set(old) & set(new)):
        if old[name][0] == new[name][0]:
            lines.append("identical  %s" % name)
            continue
        differing += 1
        lines.append("differs    %s" % name)
        for side, (body, meta) in (("old", old[name]), ("new", new[name])):
            lines.append("    %s: %s instructions=%d" % (side, " ".join("%s=%d" % (k, meta.get(k, -1)) for k in FIELDS), n_instructions(body)))
    only = [("only in old", sorted(set(old) - set(new))), ("only in new", sorted(set(new) - set(old)))]
    for label, names in only:
        lines += ["%s: %s" % (label, n) for n in names]
    both = len(set(old) & set(new))
    lines.append("kernels: %d in both, %d identical, %d differ, %d only in old, %d only in new" % (both, both - differing, differing, len(only[0][1]), len(only[1][1])))
    return lines, differing, only


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    print("\n".join(compare(argv[1], argv[2])[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
