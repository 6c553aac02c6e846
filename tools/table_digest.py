#!/usr/bin/env python3
"""What the pattern compiler makes of every golden pattern, one line per program: for a refactor that must leave the tables as they are.

    python tools/table_digest.py [path/to/libtrre_mi355x.so] > digest.txt

Every distinct pattern of tests/golden/golden.json (cases, all_cases, match_cases, lazy_cases; in order of first appearance) is compiled
on both engines in all seven modes.  A line holds the pattern's index, the engine, the mode, the return code, trre_last_error() where
the code is not zero, else every field of trre_info and the length and SHA-256 of each table export: trre_export_tables (t),
trre_export_stream_tables (s), trre_export_guided_tables 0-7 (g0-g7) and, for a DFT scan program, trre_debug_lazy_tables 0-2 (z0-z2).
Host only: no device is touched.  It compares nothing itself: run it on two builds and diff the outputs (the switches that change a
compile, TRRE_NFT_FOLD among them, are read from the environment as always)."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 1, 2, 3, 4, 8, 16)
INFO = ("engine", "kernel", "nft_states", "nft_cons_states", "dft_states", "table_rows", "table_classes", "table_bytes", "flags",
        "chunk_bytes", "stream_states", "stream_classes", "nft_nodes", "guided_rev_states", "guided_fwd_states")


class Info(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32 if name in ("engine", "kernel") else ctypes.c_uint32) for name in INFO]


def patterns():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        golden = json.load(f)
    seen = []
    for group in ("cases", "all_cases", "match_cases", "lazy_cases"):
        for case in golden[group]:
            if case["pattern"] not in seen:
                seen.append(case["pattern"])
    return [p.encode("latin-1") for p in seen]


def load(path):
    lib = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.trre_compile_mode.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.trre_last_error.restype = ctypes.c_char_p
    lib.trre_free.argtypes = [vp]
    lib.trre_free.restype = None
    lib.trre_get_info.argtypes = [vp, ctypes.POINTER(Info)]
    for fn in (lib.trre_export_tables, lib.trre_export_stream_tables):
        fn.argtypes, fn.restype = [vp, vp, sz], sz
    for fn in (lib.trre_export_guided_tables, lib.trre_debug_lazy_tables):
        fn.argtypes, fn.restype = [vp, ctypes.c_int, vp, sz], sz
    return lib


def digest(export):
    """`length:sha256` of what export(buf, cap) hands out"""
    n = export(None, 0)
    buf = ctypes.create_string_buffer(max(n, 1))
    export(buf, n)
    return "%d:%s" % (n, hashlib.sha256(buf.raw[:n]).hexdigest())


def main(argv):
    if len(argv) > 2:
        print(__doc__)
        return 2
    lib = load(argv[1] if len(argv) == 2 else os.path.join(ROOT, "trre_amd", "lib", "libtrre_mi355x.so"))
    for idx, pattern in enumerate(patterns()):
        for engine in (0, 1):
            for mode in MODES:
                prog = ctypes.c_void_p()
                rc = lib.trre_compile_mode(pattern, len(pattern), engine, mode, ctypes.byref(prog))
                fields = ["%d" % idx, "engine=%d" % engine, "mode=%d" % mode, "rc=%d" % rc]
                if rc != 0:
                    fields.append("error=%r" % lib.trre_last_error().decode("latin-1"))
                if prog:
                    info = Info()
                    fields.append("info_rc=%d" % lib.trre_get_info(prog, ctypes.byref(info)))
                    fields += ["%s=%d" % (name, getattr(info, name)) for name in INFO]
                    fields.append("t=" + digest(lambda b, n: lib.trre_export_tables(prog, b, n)))
                    fields.append("s=" + digest(lambda b, n: lib.trre_export_stream_tables(prog, b, n)))
                    fields += ["g%d=%s" % (w, digest(lambda b, n, w=w: lib.trre_export_guided_tables(prog, w, b, n))) for w in range(8)]
                    if engine == 1 and mode == 0:
                        fields += ["z%d=%s" % (w, digest(lambda b, n, w=w: lib.trre_debug_lazy_tables(prog, w, b, n))) for w in range(3)]
                    lib.trre_free(prog)
                print(" ".join(fields))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
