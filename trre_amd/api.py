"""ctypes binding of libtrre_mi355x.so (include/trre_mi355x.h).

Host-side mirror of the reference's command-line interface for the scan path:
``Program(pattern, engine)`` plays ``./trre PATTERN`` (engine="nft",
trre_nft.c:713-790) or ``./trre_dft PATTERN`` (engine="dft",
trre_dft.c:1199-1286); ``Program.scan(data)`` is the scan branch of main() over
a whole buffer.  The scan always runs on the GPU through the C ABI — there is no
Python or CPU implementation of it here, and a missing library or device raises.

PyTorch is used only as plumbing (device buffers, streams); it is imported
lazily so that pattern compilation and table inspection work without it.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRRE_LIB_PATH") or os.path.join(_HERE, "lib", "libtrre_mi355x.so")   # override: A/B builds only

ENGINE_NFT, ENGINE_DFT = 0, 1
MODE_SCAN, MODE_MATCH, MODE_SCAN_ALL, MODE_MATCH_ALL, MODE_FIND, MODE_SPANS = 0, 1, 2, 3, 4, 8
MODE_SUB = 16
_ENGINES = {"nft": ENGINE_NFT, "dft": ENGINE_DFT, ENGINE_NFT: ENGINE_NFT, ENGINE_DFT: ENGINE_DFT}

KERNEL_AUTO, KERNEL_BYTEMAP, KERNEL_TILE_LP, KERNEL_TILE_GEN, KERNEL_STREAM_LP, KERNEL_STREAM_GEN = 0, 1, 2, 3, 4, 5
KERNEL_GUIDED_LP, KERNEL_GUIDED_GEN = 6, 7
KERNEL_GENERATE = 8
KERNEL_BACKTRACK = 9
KERNEL_DFT_LAZY = 10
KERNEL_NAMES = {0: "auto", 1: "bytemap", 2: "tile_lp", 3: "tile_gen", 4: "stream_lp", 5: "stream_gen", 6: "guided_lp",
                7: "guided_gen", 8: "generate", 9: "backtrack", 10: "dft_lazy"}

FLAG_LENGTH_PRESERVING, FLAG_MEMORYLESS, FLAG_NO_OVERRUN = 1, 2, 4

E_SYNTAX, E_UNDEFINED, E_EPS_CYCLE, E_TOO_BIG, E_UNSUPPORTED = -1, -2, -3, -4, -5
E_DEVICE, E_ARG, E_DIVERGES, E_CAPACITY = -6, -7, -8, -9

FILTER_INVERT = 1
SPLIT_FROM_END = 1
TRIM_LEFT, TRIM_RIGHT = 1, 2
_TRIM_SIDES = {"left": TRIM_LEFT, "right": TRIM_RIGHT, "both": TRIM_LEFT | TRIM_RIGHT}


class TrreError(RuntimeError):
    """A failed library call; .code is the TRRE_E_* value, .message the
    reference-style 'error: ...' text."""

    def __init__(self, code, message, partial=None):
        super().__init__("%s (code %d)" % (message, code))
        self.code = code
        self.message = message
        self.partial = partial      # E_DIVERGES: what the reference had printed before it failed (bytes / tensor), or None


class Info(ctypes.Structure):
    _fields_ = [("engine", ctypes.c_int32), ("kernel", ctypes.c_int32), ("nft_states", ctypes.c_uint32),
                ("nft_cons_states", ctypes.c_uint32), ("dft_states", ctypes.c_uint32),
                ("table_rows", ctypes.c_uint32), ("table_classes", ctypes.c_uint32),
                ("table_bytes", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("chunk_bytes", ctypes.c_uint32),
                ("stream_states", ctypes.c_uint32), ("stream_classes", ctypes.c_uint32),
                ("nft_nodes", ctypes.c_uint32), ("guided_rev_states", ctypes.c_uint32),
                ("guided_fwd_states", ctypes.c_uint32)]


def build_library(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "all"], check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TrreError(E_DEVICE, "error: %s is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                                      "(the scan has no CPU fallback)" % LIB_PATH)
        try:
            import torch  # noqa: F401  (load torch's HIP runtime first so both share one libamdhip64)
        except Exception:  # pragma: no cover - torch is optional for host-only use
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.trre_compile_bytes.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(vp)]
        L.trre_compile_mode.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.trre_free.argtypes = [vp]
        L.trre_free.restype = None
        L.trre_last_error.restype = ctypes.c_char_p
        L.trre_get_info.argtypes = [vp, ctypes.POINTER(Info)]
        L.trre_set_kernel.argtypes = [vp, ctypes.c_int]
        L.trre_export_tables.argtypes = [vp, vp, sz]
        L.trre_export_tables.restype = sz
        L.trre_export_stream_tables.argtypes = [vp, vp, sz]
        L.trre_export_stream_tables.restype = sz
        L.trre_export_guided_tables.argtypes = [vp, ctypes.c_int, vp, sz]
        L.trre_export_guided_tables.restype = sz
        L.trre_scan_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
        L.trre_scan_device_records.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, ctypes.POINTER(sz), vp]
        L.trre_scan_device_strings.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, ctypes.POINTER(sz), vp]
        L.trre_match_device_strings.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_find_device_strings.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_span_device_strings.argtypes = [vp, vp, sz, vp, sz, vp, vp, sz, vp, ctypes.POINTER(sz), vp]
        L.trre_split_device_strings.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_filter_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_field_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int64, vp, sz, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_splitn_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int64, ctypes.c_uint32, vp, sz, vp, sz, vp, ctypes.POINTER(sz),
                                                 ctypes.POINTER(sz), vp]
        L.trre_fieldn_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32, vp, sz, vp, vp,
                                                 ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_trim_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp, vp, vp, ctypes.POINTER(sz), vp]
        L.trre_sub_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int64, ctypes.c_int64, vp, sz, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_nth_device_strings.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int64, vp, sz, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
        L.trre_scan_enqueue.argtypes = [vp, vp, sz, vp, sz, vp]
        L.trre_scan_finish.argtypes = [vp, ctypes.POINTER(sz)]
        L.trre_scan_host.argtypes = [vp, ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz), ctypes.c_int]
        L.trre_scan_host_multi.argtypes = [vp, ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz), ctypes.c_uint32]
        L.trre_set_profiling.argtypes = [vp, ctypes.c_int]
        L.trre_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.trre_debug_generate.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, vp, sz, ctypes.POINTER(sz)]
        L.trre_debug_lazy_tables.argtypes = [vp, ctypes.c_int, vp, sz]
        L.trre_debug_lazy_tables.restype = sz
        L.trre_debug_lazy_explore.argtypes = [vp, vp, sz, sz]
        L.trre_shard_bounds.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(sz)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise TrreError(rc, lib().trre_last_error().decode("latin-1"))


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def _column(values, offsets, stream):
    """a column of strings as the device calls take it, checked: (n, nrec, the stream's handle)"""
    import torch
    assert values.is_cuda and values.dtype == torch.uint8 and values.dim() == 1 and values.is_contiguous()
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.numel() >= 1
    s = stream if stream is not None else torch.cuda.current_stream(values.device).cuda_stream
    return values.numel(), offsets.numel() - 1, s


def _retry_capacity(call, out, m, device):
    """call(out) and, on E_CAPACITY, once more with a buffer of the size the call reported in m: (rc, out)"""
    import torch
    with torch.cuda.device(device):
        rc = call(out)
        if rc == E_CAPACITY:                       # variable-length output: retry with the size asked for
            out = torch.empty(m.value + 16, dtype=torch.uint8, device=device)
            rc = call(out)
    return rc, out


def _fetch(export, *args):
    """the two-call blob fetch: export(*args, None, 0) says the size, export(*args, buf, size) fills it; the bytes, b"" for none"""
    n = export(*args, None, 0)
    buf = ctypes.create_string_buffer(max(n, 1))
    export(*args, buf, n)
    return buf.raw[:n]


def _query_then_fill(call, query, alloc, sizes, device):
    """the size query call(*query), null pointers and no room, leaves what to allocate in sizes (c_size_t's); alloc(*their values)
    makes arrays of exactly that size and returns (result, the filling call's arguments); the filling call is made only when the
    query said E_CAPACITY, and reports the same sizes: the result"""
    import torch
    with torch.cuda.device(device):
        rc = call(*query)
        if rc not in (0, E_CAPACITY):
            _check(rc)
        asked = [x.value for x in sizes]
        result, fill = alloc(*asked)
        if rc == E_CAPACITY:
            _check(call(*fill))
            assert [x.value for x in sizes] == asked
    return result


def _validity(words, nrec, packed):
    """the validity bitmap the library wrote into words (int64): packed, its 8 * ceil(nrec / 64) bytes; else one torch.bool a string"""
    import torch
    bitmap = words.view(torch.uint8)[:8 * ((nrec + 63) // 64)]
    if packed:
        return bitmap
    shifts = torch.arange(8, dtype=torch.uint8, device=words.device)
    return ((bitmap.unsqueeze(1) >> shifts) & 1).to(torch.bool).flatten()[:nrec]


def _default_outputs(out, out_offsets, n, nrec, device):
    """out and out_offsets of the scan-like calls, made where the caller gave none"""
    import torch
    if out is None:
        out = torch.empty(max(n, 1) + 16, dtype=torch.uint8, device=device)
    if out_offsets is None:
        out_offsets = torch.empty(nrec + 1, dtype=torch.int64, device=device)
    return out, out_offsets


def _read_back(out, off, list_off=None):
    """the host read-back of the *_list methods: item j is out[off[j]:off[j + 1]], a list of bytes; with list_off a list of such
    lists, items list_off[i] .. list_off[i + 1] - 1 in list i"""
    blob = out.cpu().numpy().tobytes()
    o = off.cpu().numpy().tolist()
    items = [blob[o[j]:o[j + 1]] for j in range(len(o) - 1)]
    if list_off is None:
        return items
    lo = list_off.cpu().numpy().tolist()
    return [items[lo[i]:lo[i + 1]] for i in range(len(lo) - 1)]


def _pack(records, device):
    """a list of bytes as a column on the device: (recs, host offsets, values, offsets)"""
    import numpy as np
    import torch
    recs = [_bytes(r) for r in records]
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    dev = torch.device("cuda", device)
    packed = b"".join(recs)
    values = torch.frombuffer(bytearray(packed or b"\0"), dtype=torch.uint8)[:len(packed)].to(dev)
    return recs, off, values, torch.from_numpy(off).to(dev)


class Program:
    """A compiled pattern bound to one engine."""

    def __init__(self, pattern, engine="nft", mode="scan"):
        """mode "scan" (default), "match" (`trre -m`: whole-line matches only, NFT engine), "scan_all" (`trre -a`) or
        "match_all" (`trre -ma`): generator modes, every accepting path prints (NFT engine), or "find": every match of every
        string as a list per string (find_strings / find_list, NFT engine) and one match of every string (nth_strings /
        nth_list), or "spans": where every match of every string starts and ends (span_strings / span_list / count_strings,
        NFT engine) and the pieces between the matches (split_strings / split_list), the strings with a match or without one
        (filter_strings / filter_list) and one piece of every string (field_strings / field_list), or "sub": the first n
        matches of every string replaced by what they print (sub_strings / sub_list, NFT engine)"""
        self.pattern = _bytes(pattern)
        self.engine = _ENGINES[engine]
        self.mode = {"scan": MODE_SCAN, "match": MODE_MATCH, "scan_all": MODE_SCAN_ALL, "match_all": MODE_MATCH_ALL,
                     "find": MODE_FIND, "spans": MODE_SPANS, "sub": MODE_SUB}.get(mode, mode)
        self._h = ctypes.c_void_p()
        _check(lib().trre_compile_mode(self.pattern, len(self.pattern), self.engine, self.mode, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().trre_free(self._h)
            self._h = None

    __del__ = close

    @property
    def info(self):
        i = Info()
        _check(lib().trre_get_info(self._h, ctypes.byref(i)))
        return i

    def set_kernel(self, family):
        _check(lib().trre_set_kernel(self._h, family))

    def export_tables(self):
        return _fetch(lib().trre_export_tables, self._h)

    def export_stream_tables(self):
        return _fetch(lib().trre_export_stream_tables, self._h)

    def _guided(self, *which):
        """the blobs `which` of trre_export_guided_tables, each b"" where the program has none"""
        return tuple(_fetch(lib().trre_export_guided_tables, self._h, w) for w in which)

    def export_guided_tables(self):
        """(backward DFA blob, forward tables blob) of the guided families, or (b"", b"")"""
        return self._guided(0, 1)

    def export_accept_table(self):
        """match mode, guided tables: one byte per backward state, 1 where a line whose first byte carries that symbol is
        accepted (the verdict table of match_strings), or b"" """
        return self._guided(4)[0]

    def export_find_tables(self):
        """find mode: (backward DFA blob, texts forward tables blob, marks forward tables blob), or (b"", b"", b"")"""
        blobs = self._guided(0, 5, 6)
        return blobs if blobs[1] else (b"", b"", b"")

    def export_span_tables(self):
        """spans mode: (backward DFA blob, the markers' forward tables blob), or (b"", b"")"""
        blobs = self._guided(0, 7)
        return blobs if blobs[1] else (b"", b"")

    def export_gen_tables(self):
        """generator modes: the tables of the device enumeration (gen_block.hpp), or b"" """
        return self._guided(2)[0]

    def export_guard_tables(self):
        """the stack guard's tables (guard_block.hpp), or b"" when the pattern cannot exhaust the reference's stack"""
        return self._guided(3)[0]

    def lazy_tables(self):
        """DFT engine (CPU test tier): the lazily determinised tables as they stand: (header, entries, pool)"""
        return tuple(_fetch(lib().trre_debug_lazy_tables, self._h, which) for which in (0, 1, 2))

    def lazy_explore(self, misses, spec_states=0):
        """... and the exploration of a list of misses (numpy uint32, 16 words per record)"""
        import numpy as np
        m = np.ascontiguousarray(misses, dtype=np.uint32)
        _check(lib().trre_debug_lazy_explore(self._h, m.ctypes.data, len(m) // 16, spec_states))

    def allowed_kernels(self):
        ok = []
        for fam in (KERNEL_BYTEMAP, KERNEL_TILE_LP, KERNEL_TILE_GEN, KERNEL_STREAM_LP, KERNEL_STREAM_GEN, KERNEL_GUIDED_LP,
                    KERNEL_GUIDED_GEN, KERNEL_BACKTRACK, KERNEL_DFT_LAZY):
            if lib().trre_set_kernel(self._h, fam) == 0:
                ok.append(fam)
        lib().trre_set_kernel(self._h, KERNEL_AUTO)
        return ok

    # ---- device path ---------------------------------------------------------------
    def scan_tensor(self, inp, out=None, stream=None):
        """inp: 1-D uint8 CUDA tensor.  Returns a uint8 CUDA tensor view of the output."""
        import torch
        assert inp.is_cuda and inp.dtype == torch.uint8 and inp.dim() == 1 and inp.is_contiguous()
        n = inp.numel()
        if out is None:
            out = torch.empty(max(n, 1) + 16, dtype=torch.uint8, device=inp.device)
        s = stream if stream is not None else torch.cuda.current_stream(inp.device).cuda_stream
        m = ctypes.c_size_t()

        def call(o):
            return lib().trre_scan_device(self._h, inp.data_ptr(), n, o.data_ptr(), o.numel(), ctypes.byref(m), s)
        rc, out = _retry_capacity(call, out, m, inp.device)
        if rc == E_DIVERGES:
            raise TrreError(rc, lib().trre_last_error().decode("latin-1"), out[:m.value])
        _check(rc)
        return out[:m.value]

    def scan_records(self, values, offsets, out=None, out_offsets=None, stream=None):
        """Ragged records (trre_scan_device_records): values, a 1-D uint8 CUDA tensor, holds record i at
        values[offsets[i]:offsets[i+1]] (offsets: 1-D int64 CUDA tensor, nrec + 1 entries, from 0 to values.numel()).  Each
        record is scanned as if it were a file of its own.  Returns (out_values, out_offsets): record i's output is
        out_values[out_offsets[i]:out_offsets[i+1]].  out may be values itself (in place); a too small out is replaced."""
        n, nrec, s = _column(values, offsets, stream)
        out, out_offsets = _default_outputs(out, out_offsets, n, nrec, values.device)
        m = ctypes.c_size_t()

        def call(o):
            return lib().trre_scan_device_records(self._h, values.data_ptr(), n, offsets.data_ptr(), nrec, o.data_ptr(), o.numel(),
                                                  out_offsets.data_ptr(), ctypes.byref(m), s)
        rc, out = _retry_capacity(call, out, m, values.device)
        if rc == E_DIVERGES:
            raise TrreError(rc, lib().trre_last_error().decode("latin-1"), out[:m.value])
        _check(rc)
        return out[:m.value], out_offsets

    def scan_strings(self, values, offsets, out=None, out_offsets=None, stream=None):
        """Packed strings (trre_scan_device_strings): values, a 1-D uint8 CUDA tensor, holds string i at
        values[offsets[i]:offsets[i+1]] (offsets: 1-D int64 CUDA tensor, nrec + 1 entries, from 0 to values.numel()).  Each
        string is the content of one line, without a line end: its output is what the program prints for that line, without
        the framing newline (b"cat" under [a:A-z:Z] gives b"CAT"; an empty string gives what an empty line prints).  Returns
        (out_values, out_offsets): string i's output is out_values[out_offsets[i]:out_offsets[i+1]].  out may be values itself
        (in place); a too small out is replaced.  A string the reference does not survive raises TrreError with partial=None."""
        n, nrec, s = _column(values, offsets, stream)
        out, out_offsets = _default_outputs(out, out_offsets, n, nrec, values.device)
        m = ctypes.c_size_t()

        def call(o):
            return lib().trre_scan_device_strings(self._h, values.data_ptr(), n, offsets.data_ptr(), nrec, o.data_ptr(), o.numel(),
                                                  out_offsets.data_ptr(), ctypes.byref(m), s)
        rc, out = _retry_capacity(call, out, m, values.device)
        _check(rc)
        return out[:m.value], out_offsets

    def map_strings(self, records, device=0):
        """list of bytes in -> list of bytes out, the program applied to each string as one line (through scan_strings)"""
        return self._map_list(records, device, self.scan_strings)

    def scan_list(self, records, device=0):
        """list of bytes in -> list of bytes out, each record scanned as a file of its own (through scan_records)"""
        return self._map_list(records, device, self.scan_records)

    def match_strings(self, values, offsets, out=None, out_offsets=None, stream=None, packed=False):
        """Matched strings (trre_match_device_strings; a program compiled with mode="match"): values and offsets as for
        scan_strings, no string holding a b"\\n".  Returns (out_values, out_offsets, valid): valid[i] says whether the pattern
        accepts string i as a whole line, out_values[out_offsets[i]:out_offsets[i+1]] is what it becomes (empty when rejected).
        valid is a torch.bool tensor of nrec entries; with packed=True it is the Arrow validity bitmap as the library wrote it
        (uint8, 8 * ceil(nrec / 64) bytes, bit i & 7 of byte i >> 3).  out may be values itself; a too small out is replaced."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        out, out_offsets = _default_outputs(out, out_offsets, n, nrec, values.device)
        words = torch.zeros(max((nrec + 63) // 64, 1), dtype=torch.int64, device=values.device)     # (8-byte aligned)
        m, k = ctypes.c_size_t(), ctypes.c_size_t()

        def call(o):
            return lib().trre_match_device_strings(self._h, values.data_ptr(), n, offsets.data_ptr(), nrec, o.data_ptr(), o.numel(),
                                                   out_offsets.data_ptr(), words.data_ptr(), ctypes.byref(k), ctypes.byref(m), s)
        rc, out = _retry_capacity(call, out, m, values.device)
        _check(rc)
        return out[:m.value], out_offsets, _validity(words, nrec, packed)

    def match_list(self, records, device=0):
        """list of bytes in -> list out: what an accepted string becomes (bytes), None for a rejected one (through match_strings)"""
        recs, off, values, offsets = _pack(records, device)
        out, out_off, valid = self.match_strings(values, offsets)
        return [b if ok else None for b, ok in zip(_read_back(out, out_off), valid.cpu().numpy().tolist())]

    def find_strings(self, values, offsets, stream=None):
        """Found strings (trre_find_device_strings; a program compiled with mode="find"): values and offsets as for
        scan_strings, no string holding a b"\\n".  Returns (out, match_offsets, list_offsets): string i's matches are numbers
        list_offsets[i] .. list_offsets[i + 1] - 1, and match j's output is out[match_offsets[j]:match_offsets[j + 1]].  Two
        calls: the size query, then the one that fills buffers of exactly that size."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        list_off = torch.empty(nrec + 1, dtype=torch.int64, device=values.device)
        m, k = ctypes.c_size_t(), ctypes.c_size_t()

        def call(o, cap, mo, mcap):
            return lib().trre_find_device_strings(self._h, values.data_ptr(), n, offsets.data_ptr(), nrec, o, cap, mo, mcap,
                                                  list_off.data_ptr(), ctypes.byref(k), ctypes.byref(m), s)

        def alloc(k, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            match_off = torch.zeros(k + 1, dtype=torch.int64, device=values.device)
            return (out[:m], match_off, list_off), (out.data_ptr(), m, match_off.data_ptr(), k)
        return _query_then_fill(call, (None, 0, None, 0), alloc, (k, m), values.device)

    def find_list(self, records, device=0):
        """list of bytes in -> list of lists of bytes out: every match's output, string by string (through find_strings)"""
        recs, off, values, offsets = _pack(records, device)
        return _read_back(*self.find_strings(values, offsets))

    def nth_strings(self, values, offsets, k=0, stream=None, packed=False):
        """Match k of every string (trre_nth_device_strings; a program compiled with mode="find"): values and offsets as for
        scan_strings, no string holding a b"\\n".  ONE entry of every string's list of find_strings: match k, or, for k < 0,
        match k counted from the end (-1: the last), as re.search(p, s).group() (k = 0), s.str.findall(p).str.get(k) and SQL's
        regexp_substr(s, p, 1, k + 1).  Returns (out, out_offsets, valid): string i's entry is
        out[out_offsets[i]:out_offsets[i + 1]], empty when the string has no such match, and valid[i] says whether it has (an
        empty output of a match that exists is valid).  valid is a torch.bool tensor of nrec entries; with packed=True it is the
        Arrow validity bitmap as the library wrote it (uint8, 8 * ceil(nrec / 64) bytes, bit i & 7 of byte i >> 3).  Two calls:
        the size query, then the one that fills a buffer of exactly that size."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        words = torch.zeros(max((nrec + 63) // 64, 1), dtype=torch.int64, device=values.device)     # (8-byte aligned)
        m, v = ctypes.c_size_t(), ctypes.c_size_t()

        def call(o, cap, oo):
            return lib().trre_nth_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, o, cap, oo,
                                                 words.data_ptr(), ctypes.byref(v), ctypes.byref(m), s)

        def alloc(v, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            out_off = torch.zeros(nrec + 1, dtype=torch.int64, device=values.device)     # (no entry has bytes: all zero, as they are)
            return (out[:m], out_off), (out.data_ptr(), m, out_off.data_ptr())
        return _query_then_fill(call, (None, 0, None), alloc, (v, m), values.device) + (_validity(words, nrec, packed),)

    def nth_list(self, records, k=0, device=0):
        """list of bytes in -> list out: the output of match k of every string (bytes), None where the string has no such match
        (through nth_strings)"""
        recs, off, values, offsets = _pack(records, device)
        out, out_off, valid = self.nth_strings(values, offsets, k)
        return [b if ok else None for b, ok in zip(_read_back(out, out_off), valid.cpu().numpy().tolist())]

    def _span_call(self, values, offsets, stream):
        """trre_span_device_strings on a column: (call(d_start, d_end, span_cap) -> rc, *n_matches, list_offsets)"""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        list_off = torch.empty(nrec + 1, dtype=torch.int64, device=values.device)
        k = ctypes.c_size_t()

        def call(st, en, cap):
            return lib().trre_span_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, st, en, cap,
                                                  list_off.data_ptr(), ctypes.byref(k), s)
        return call, k, list_off

    def span_strings(self, values, offsets, stream=None):
        """Match spans (trre_span_device_strings; a program compiled with mode="spans"): values and offsets as for scan_strings,
        no string holding a b"\\n".  Returns (starts, ends, list_offsets), int64: string i's matches are numbers list_offsets[i]
        .. list_offsets[i + 1] - 1, and match j is values[starts[j]:ends[j]] — positions in values, absolute.  Two calls: the
        size query, then the one that fills arrays of exactly that size."""
        import torch
        call, k, list_off = self._span_call(values, offsets, stream)

        def alloc(k):
            starts = torch.empty(k, dtype=torch.int64, device=values.device)
            ends = torch.empty(k, dtype=torch.int64, device=values.device)
            return (starts, ends, list_off), (starts.data_ptr(), ends.data_ptr(), k)
        return _query_then_fill(call, (None, None, 0), alloc, (k,), values.device)

    def count_strings(self, values, offsets, stream=None):
        """matches per string (str.count; > 0: str.contains), int64 — the size query alone: no span is stored"""
        import torch
        call, _, list_off = self._span_call(values, offsets, stream)
        with torch.cuda.device(values.device):
            rc = call(None, None, 0)
        if rc not in (0, E_CAPACITY):
            _check(rc)
        return list_off[1:] - list_off[:-1]

    def span_list(self, records, device=0):
        """list of bytes in -> per string a list of (start, end) relative to that string, as m.span() of re.finditer (through
        span_strings)"""
        recs, off, values, offsets = _pack(records, device)
        starts, ends, list_off = self.span_strings(values, offsets)
        st, en, lo = starts.cpu().numpy().tolist(), ends.cpu().numpy().tolist(), list_off.cpu().numpy().tolist()
        return [[(st[j] - int(off[i]), en[j] - int(off[i])) for j in range(lo[i], lo[i + 1])] for i in range(len(recs))]

    def split_strings(self, values, offsets, stream=None, *, limit=-1, from_end=False):
        """Split strings (trre_split_device_strings; a program compiled with mode="spans"): values and offsets as for
        scan_strings, no string holding a b"\\n".  Every string is cut at every match, as re.split cuts it.  Returns (out,
        piece_offsets, list_offsets): string i's pieces are numbers list_offsets[i] .. list_offsets[i + 1] - 1 (one more than
        its matches), and piece k is out[piece_offsets[k]:piece_offsets[k + 1]].  Two calls: the size query, then the one that
        fills buffers of exactly that size.
        limit >= 0 (trre_splitn_device_strings) cuts at the first `limit` matches of every string only, with from_end=True at
        the last `limit`; a match that does not cut stays in its piece: limit=1 is line.split(sep, 1) and str.partition,
        limit=1 with from_end=True s.rsplit(sep, 1) and str.rpartition, limit=n re.split(p, s, maxsplit=n) for n >= 1; limit=0
        cuts nothing, and a negative limit cuts at every match.  With the defaults the call is trre_split_device_strings."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        list_off = torch.empty(nrec + 1, dtype=torch.int64, device=values.device)
        m, k = ctypes.c_size_t(), ctypes.c_size_t()
        limited = limit != -1 or from_end

        def call(o, cap, po, pcap):
            if limited:
                return lib().trre_splitn_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, limit,
                                                        SPLIT_FROM_END if from_end else 0, o, cap, po, pcap, list_off.data_ptr(),
                                                        ctypes.byref(k), ctypes.byref(m), s)
            return lib().trre_split_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, o, cap, po, pcap,
                                                   list_off.data_ptr(), ctypes.byref(k), ctypes.byref(m), s)

        def alloc(k, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            piece_off = torch.zeros(k + 1, dtype=torch.int64, device=values.device)
            return (out[:m], piece_off, list_off), (out.data_ptr(), m, piece_off.data_ptr(), k)
        return _query_then_fill(call, (None, 0, None, 0), alloc, (k, m), values.device)

    def split_list(self, records, device=0, *, limit=-1, from_end=False):
        """list of bytes in -> per string the list of its pieces (bytes), as re.split gives them (through split_strings; limit and
        from_end as there)"""
        recs, off, values, offsets = _pack(records, device)
        return _read_back(*self.split_strings(values, offsets, limit=limit, from_end=from_end))

    def filter_strings(self, values, offsets, invert=False, stream=None):
        """Filtered strings (trre_filter_device_strings; a program compiled with mode="spans"): values and offsets as for
        scan_strings, no string holding a b"\\n".  The strings with at least one match are kept whole and the rest dropped, as
        s[s.str.contains(p)]; with invert=True the strings without a match are kept (grep -v).  Returns (out, out_offsets,
        rows): kept string r is out[out_offsets[r]:out_offsets[r + 1]] and was string rows[r] of the column (int64, strictly
        increasing: the index that filters the sibling columns).  Two calls: the size query, then the one that fills buffers of
        exactly that size."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        flags = FILTER_INVERT if invert else 0
        m, k = ctypes.c_size_t(), ctypes.c_size_t()

        def call(o, cap, oo, rows, rcap):
            return lib().trre_filter_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, flags, o, cap, oo, rows,
                                                    rcap, ctypes.byref(k), ctypes.byref(m), s)

        def alloc(k, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            out_off = torch.zeros(k + 1, dtype=torch.int64, device=values.device)
            rows = torch.empty(k, dtype=torch.int64, device=values.device)
            return (out[:m], out_off, rows), (out.data_ptr(), m, out_off.data_ptr(), rows.data_ptr(), k)
        return _query_then_fill(call, (None, 0, None, None, 0), alloc, (k, m), values.device)

    def filter_list(self, records, invert=False, device=0):
        """list of bytes in -> (the kept strings, their indices in the list) (through filter_strings)"""
        recs, off, values, offsets = _pack(records, device)
        out, out_off, rows = self.filter_strings(values, offsets, invert=invert)
        return _read_back(out, out_off), rows.cpu().numpy().tolist()

    def field_strings(self, values, offsets, k, stream=None, packed=False, *, limit=-1, from_end=False):
        """Field k of every string (trre_field_device_strings; a program compiled with mode="spans"): values and offsets as for
        scan_strings, no string holding a b"\\n".  Every string is split at every match, as split_strings does, and ONE piece of
        it taken: piece k, or, for k < 0, piece k counted from the end (-1: the last), as s.str.split(p).str.get(k) and SQL's
        split_part.  Returns (out, out_offsets, valid): string i's field is out[out_offsets[i]:out_offsets[i + 1]], empty when the
        string has no such piece, and valid[i] says whether it has.  valid is a torch.bool tensor of nrec entries; with
        packed=True it is the Arrow validity bitmap as the library wrote it (uint8, 8 * ceil(nrec / 64) bytes, bit i & 7 of byte
        i >> 3).  Two calls: the size query, then the one that fills a buffer of exactly that size.
        limit and from_end (trre_fieldn_device_strings) are split_strings': the field is piece k of that limited split — limit=1
        with k=1 the value of b"key=v=w", limit=1, from_end=True with k=0 the stem of b"x.tar.gz".  With the defaults the call is
        trre_field_device_strings."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        words = torch.zeros(max((nrec + 63) // 64, 1), dtype=torch.int64, device=values.device)     # (8-byte aligned)
        m, v = ctypes.c_size_t(), ctypes.c_size_t()
        limited = limit != -1 or from_end

        def call(o, cap, oo):
            if limited:
                return lib().trre_fieldn_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, limit,
                                                        SPLIT_FROM_END if from_end else 0, o, cap, oo, words.data_ptr(), ctypes.byref(v),
                                                        ctypes.byref(m), s)
            return lib().trre_field_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, k, o, cap, oo,
                                                   words.data_ptr(), ctypes.byref(v), ctypes.byref(m), s)

        def alloc(v, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            out_off = torch.zeros(nrec + 1, dtype=torch.int64, device=values.device)     # (no field has bytes: all zero, as they are)
            return (out[:m], out_off), (out.data_ptr(), m, out_off.data_ptr())
        return _query_then_fill(call, (None, 0, None), alloc, (v, m), values.device) + (_validity(words, nrec, packed),)

    def field_list(self, records, k, device=0, *, limit=-1, from_end=False):
        """list of bytes in -> list out: field k of every string (bytes), None where the string has no such piece (through
        field_strings; limit and from_end as there)"""
        recs, off, values, offsets = _pack(records, device)
        out, out_off, valid = self.field_strings(values, offsets, k, limit=limit, from_end=from_end)
        return [b if ok else None for b, ok in zip(_read_back(out, out_off), valid.cpu().numpy().tolist())]

    def _trim_call(self, values, offsets, side, stream):
        """trre_trim_device_strings on a column: (call(d_out, cap, d_out_off, d_begin, d_end) -> rc, *out_len, nrec)"""
        if side not in _TRIM_SIDES:
            raise ValueError("side must be 'left', 'right' or 'both', not %r" % (side,))
        flags = _TRIM_SIDES[side]
        n, nrec, s = _column(values, offsets, stream)
        m = ctypes.c_size_t()

        def call(o, cap, oo, begin, end):
            return lib().trre_trim_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, flags, o, cap, oo,
                                                  begin, end, ctypes.byref(m), s)
        return call, m, nrec

    def trim_strings(self, values, offsets, side="both", stream=None):
        """Trimmed strings (trre_trim_device_strings; a program compiled with mode="spans"): values and offsets as for
        scan_strings, no string holding a b"\\n".  Every string loses the match that starts at its start (side="left":
        s.str.lstrip, removeprefix), the match that ends at its end (side="right": rstrip, removesuffix) or both (side="both":
        strip, SQL's TRIM, re.sub('^P|P$', '', s)); one match a side, so strip() of a class is the pattern [class]+.  Returns
        (out, out_offsets): string i's entry is out[out_offsets[i]:out_offsets[i + 1]].  Two calls: the size query, then the one
        that fills a buffer of exactly that size."""
        import torch
        call, m, nrec = self._trim_call(values, offsets, side, stream)

        def alloc(m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            out_off = torch.zeros(nrec + 1, dtype=torch.int64, device=values.device)     # (no entry has bytes: all zero, as they are)
            return (out[:m], out_off), (out.data_ptr(), m, out_off.data_ptr(), None, None)
        return _query_then_fill(call, (None, 0, None, None, None), alloc, (m,), values.device)

    def trim_ranges(self, values, offsets, side="both", stream=None):
        """The view form of trim_strings: (begin, end), int64, nrec entries each — string i's entry is values[begin[i]:end[i]],
        positions in values, absolute.  One call without output: nothing is copied."""
        import torch
        call, _, nrec = self._trim_call(values, offsets, side, stream)
        begin = torch.empty(nrec, dtype=torch.int64, device=values.device)
        end = torch.empty(nrec, dtype=torch.int64, device=values.device)
        with torch.cuda.device(values.device):
            rc = call(None, 0, None, begin.data_ptr(), end.data_ptr())
        if rc not in (0, E_CAPACITY):
            _check(rc)
        return begin, end

    def trim_list(self, records, side="both", device=0):
        """list of bytes in -> list of bytes out: every string trimmed (through trim_strings)"""
        if side not in _TRIM_SIDES:
            raise ValueError("side must be 'left', 'right' or 'both', not %r" % (side,))
        recs, off, values, offsets = _pack(records, device)
        return _read_back(*self.trim_strings(values, offsets, side))

    def sub_strings(self, values, offsets, count=-1, first=0, stream=None):
        """Some of every string's matches replaced by what they print (trre_sub_device_strings; a program compiled with
        mode="sub"): values and offsets as for scan_strings, no string holding a b"\\n".  Match r of its string (r = 0, 1, ..) is
        replaced when first <= r and (count < 0 or r - first < count): count=1 is sed's s/x/y/ and re.sub(.., count=1), first=k
        with count=1 the k-th occurrence only, first=k with count=-1 every one from the k-th on; the defaults replace all.
        Everything else of the string stays, a NUL and what is behind it included.  Returns (out, out_offsets): string i's
        output is out[out_offsets[i]:out_offsets[i + 1]].  Two calls: the size query, then the one that fills a buffer of
        exactly that size."""
        import torch
        n, nrec, s = _column(values, offsets, stream)
        m, r = ctypes.c_size_t(), ctypes.c_size_t()

        def call(o, cap, oo):
            return lib().trre_sub_device_strings(self._h, values.data_ptr() if n else None, n, offsets.data_ptr(), nrec, first, count, o, cap, oo,
                                                 ctypes.byref(r), ctypes.byref(m), s)

        def alloc(r, m):
            out = torch.empty(m + 16, dtype=torch.uint8, device=values.device)
            out_off = torch.zeros(nrec + 1, dtype=torch.int64, device=values.device)     # (every output empty: all zero, as they are)
            return (out[:m], out_off), (out.data_ptr(), m, out_off.data_ptr())
        return _query_then_fill(call, (None, 0, None), alloc, (r, m), values.device)

    def sub_list(self, records, count=-1, first=0, device=0):
        """list of bytes in -> list of bytes out: every string with the selected matches replaced (through sub_strings)"""
        recs, off, values, offsets = _pack(records, device)
        return _read_back(*self.sub_strings(values, offsets, count=count, first=first))

    @staticmethod
    def _map_list(records, device, scan):
        recs, off, values, offsets = _pack(records, device)
        return _read_back(*scan(values, offsets))

    def enqueue(self, inp, out, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(inp.device).cuda_stream
        _check(lib().trre_scan_enqueue(self._h, inp.data_ptr(), inp.numel(), out.data_ptr(), out.numel(), s))

    def finish(self):
        m = ctypes.c_size_t()
        _check(lib().trre_scan_finish(self._h, ctypes.byref(m)))
        return m.value

    def scan(self, data, device=0, device_mask=None):
        """bytes in -> bytes out through trre_scan_host (H2D, GPU scan, D2H); with device_mask (0 = every
        visible GPU) through trre_scan_host_multi, line-sharded over the selected GPUs."""
        import numpy as np
        data = _bytes(data)
        cap = len(data) + 64
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)              # (not zero-filled: the library writes what it reports)
            m = ctypes.c_size_t()
            if device_mask is None:
                rc = lib().trre_scan_host(self._h, data, len(data), out.ctypes.data_as(ctypes.c_char_p), cap, ctypes.byref(m), device)
            else:
                rc = lib().trre_scan_host_multi(self._h, data, len(data), out.ctypes.data_as(ctypes.c_char_p), cap, ctypes.byref(m),
                                                device_mask)
            if rc == E_CAPACITY:
                cap = m.value + 64
                continue
            if rc == E_DIVERGES:
                raise TrreError(rc, lib().trre_last_error().decode("latin-1"), out[:m.value].tobytes())
            _check(rc)
            return out[:m.value].tobytes()
        _check(rc)

    def generate_with_symbols(self, data, sym):
        """generator modes, host only (CPU test tier): the enumeration with viability symbols computed elsewhere"""
        import numpy as np
        data, sym = _bytes(data), _bytes(sym)
        cap = 1 << 16
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)
            m = ctypes.c_size_t()
            rc = lib().trre_debug_generate(self._h, data, len(data), sym, out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(m))
            if rc == E_CAPACITY:
                cap = m.value + 64
                continue
            if rc == E_DIVERGES:
                raise TrreError(rc, lib().trre_last_error().decode("latin-1"), out[:m.value].tobytes())
            _check(rc)
            return out[:m.value].tobytes()
        _check(rc)

    def set_profiling(self, on=True):
        _check(lib().trre_set_profiling(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _check(lib().trre_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value


def shard_bounds(data, nshards):
    """Byte offsets that cut `data` into nshards pieces at '\\n' boundaries."""
    data = _bytes(data)
    b = (ctypes.c_size_t * (nshards + 1))()
    _check(lib().trre_shard_bounds(data, len(data), nshards, b))
    return list(b)
