"""What the nth tests share (tests/test_nth_strings.py, tests/test_nth_shim.py, tests/test_gpu_nth_strings.py): the yardstick.

The yardstick is the reference through the oracle, never the engine: tests/find_lib.py's Finder gives find(s), the list of the
outputs of the scan loop's successful attempts on a string, and entry k is Python's own indexing of that list: l[k] where
-len(l) <= k < len(l), else nothing — the definition of include/trre_mi355x.h, with k = -1 the last match and any k legal."""
from field_lib import bitmap  # noqa: F401  (the Arrow validity bitmap as the library writes it)


def pick(l, k):
    """match k of one string's list: bytes, or None when the string has no such match"""
    return l[k] if -len(l) <= k < len(l) else None


def expect(lists, k):
    """the call's three arrays from the strings' lists: (out bytes, out offsets, valid)"""
    out, oo, valid = [], [0], []
    for l in lists:
        e = pick(l, k)
        out.append(e or b"")
        oo.append(oo[-1] + len(out[-1]))
        valid.append(e is not None)
    return b"".join(out), oo, valid


def per_string(out, oo, valid):
    """the inverse: per string its entry or None, from the call's arrays"""
    return [out[oo[i]:oo[i + 1]] if valid[i] else None for i in range(len(oo) - 1)]
