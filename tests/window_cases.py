"""Inputs for the positional-window kernel (k_stream_lpw; scan_block.hpp: WtLane, WtMover) whose edges are PLACED, not hoped for, written once for
the CPU tier (tests/test_window_cases.py: the host shim) and the GPU tier (tests/gpu_window_check.py, tests/test_gpu_window.py).  Pure Python:
nothing here touches a GPU, the library or the oracle.

Geometry.  The runtime aligns the input pointer down to 16 bytes: with the input `a` bytes off alignment (0..15) the data starts at VIRTUAL offset
a and ends at vend = a + n, and lane k walks the virtual offsets [k B, (k + 1) B) — B the lane size, a multiple of 128.  Every offset in this file
is virtual; data[i] is virtual offset a + i.  A piece is 64 bytes, an output row 128, a wave 64 lanes, a workgroup 256.

What a lane does (WtLane::init / check / back), which is what the cases are about and what expected_redo() restates by hand:
    init    lo = k B, hi = min(lo + B, vend).  A lane with lo < a + 64 or hi + 192 > vend is REDONE (the redo zones: the first 64 bytes and the
            last 3 * 64 + B).  Else fs = the first offset in [lo, hi) with a '\\n' right before it; none: the lane never walks.  It starts walking
            at rv = (fs - lo) & ~127 and writes the block that holds fs bytewise.
    walk    piece by piece until the first '\\n' at or behind hi - 1 — its last line's end, at e — has gone by; if e lies in the last 16 bytes of
            its piece ((e - lo) % 64 >= 48) one piece more, for the output block that needs the next block's first bytes.
    check   at the top of every piece: rv > vend - lo - 192 hands the lane over mid-walk (a very long last line; no line end before the input's).

A Case:
    name        what it is about; the same names for every lane size and every program
    data        the bytes (n = vend - a of them)
    a, B        the misalignment and the lane size it was built for
    edges       [Edge(name, virtual offset)]: what the case claims to contain; tests/test_window_cases.py checks every claim in the bytes.
                head:*    the offset is the first line start of its lane (a key ends right before the '\\n' in front of it, one starts at it)
                tail:hi+d the offset holds the '\\n' that ends the last line of the lane whose end `hi` is d below it (a key before, one behind)
                inline:*  a lane edge inside ONE line that covers whole lanes: a key ends at it, a key starts at it
                split:kind:i   a key has its first i bytes below the offset, an edge of that kind (i = len(key): it ends there, the next one starts)
                run:*, end:*, final:*, first:*, nul:*   see ends() and main()
    no_start    the lanes the case claims to have NO line start in (they go inactive at init)
    redo        the lanes expected to be redone: expected_redo(), from the bytes and the three rules above
    nul         the input holds a NUL: the window launch is void, the general family answers (the bytes are the oracle's all the same)

Every placed edge sits outside the redo zones unless the case is about them (the end:*, final:* and nul:last_piece cases are).  Between the placed
stretches lies seeded word soup: short lines of words, the program's key and pieces of it among them.  Placed stretches never overlap (_Canvas.claim).
Every line stays under LONG bytes: runtime.cpp's long_line_switch hands inputs with a line of 32 KiB to the general family.

Lanes of 16 384 bytes: one line cannot cover two whole lanes under that limit, so `one line covering 2 / 3 / 65 lanes` exist at the smaller sizes
only, and the long final line is 3 B / 2 there; everything else is the same layout, scaled."""
import collections
import functools
import random

PIECE, ROW, WAVE, GROUP = 64, 128, 64, 256
LONG = 32768 - 1024
NL = 0x0A
Prog = collections.namedtuple("Prog", "tag pat eng key delay form")
Edge = collections.namedtuple("Edge", "name off")
Case = collections.namedtuple("Case", "name data a B edges no_start redo nul")

# form: what the launcher chooses for the tables (asserted from export_stream_tables() in tests/test_window_cases.py, not assumed): "pair" (narrow
# entries that also have the pair form), "narrow" (delay <= 3, the pair form would not fit the LDS), "wide" (delay 4..7)
_ZOO = "(cat:dog|dog:cat|pig:cow|cow:pig|hen:fox|fox:hen|owl:bat|bat:owl)"
PROGRAMS = [Prog(tag + "_" + eng, pat, eng, key, delay, form) for tag, pat, key, delay, form in [
    ("swap2", "(ab:ba|ba:ab)", b"ab", 1, "pair"),
    ("catdog", "(cat:dog|dog:cat)", b"cat", 2, "pair"),
    ("zoo", _ZOO, b"cat", 2, "narrow"),
    ("ther", "ther:THER", b"ther", 3, "pair"),
    ("there", "there:THERE", b"there", 4, "wide"),
    ("abcdef", "abcdef:ABCDEF", b"abcdef", 5, "wide"),
    ("abcdefg", "abcdefg:GFEDCBA|hell:HELL", b"abcdefg", 6, "wide"),
    ("abcdefgh", "abcdefgh:ABCDEFGH", b"abcdefgh", 7, "wide"),
] for eng in ("nft", "dft")]
# (program, engine) pairs without a window form: the only cases a tier may leave out.  None today.
NO_WINDOW_FORM = []
# the 16 KiB job runs one narrow and one wide program
BIG_PROGRAMS = ["catdog_nft", "abcdefg_nft"]

HEAD_RESIDUES = (0, 1, 15, 16, 17, 63, 64, 65, 112, 127)


def tails(B):
    """the placements of the '\\n' that ends a lane's last line, relative to the lane's end hi"""
    out = collections.OrderedDict()
    for d in (-1, 0, 1, 15, 16, 47, 48, 49, 63, 64):
        out["hi%+d" % d if d else "hi"] = d
    out["hi+B-1"] = B - 1
    out["hi+B"] = B
    return out


SPLIT_KINDS = {"dword": lambda e, B: e % 4 == 0 and e % 16 != 0, "block": lambda e, B: e % 16 == 0 and e % 64 != 0,
               "piece": lambda e, B: e % 64 == 0 and e % 128 != 0, "row": lambda e, B: e % 128 == 0, "lane": lambda e, B: e % B == 0,
               "wave": lambda e, B: e % (WAVE * B) == 0 and e % (GROUP * B) != 0, "workgroup": lambda e, B: e % (GROUP * B) == 0}


@functools.lru_cache(maxsize=None)
def _soup_block(key, seed):
    rng = random.Random(seed * 1000 + len(key))
    vocab = [key, key, key[:-1], key[1:], key[:1], key + key[:1], key + key, b"the", b"quick", b"fox,", b"a", b"lazy", b"hello", b"dog", b"cat",
             b"world;", b"0", b"hell", b"abc", b"there", b""]
    out = bytearray()
    while len(out) < 99000:
        out += b" ".join(rng.choice(vocab) for _ in range(rng.randint(0, 14))) + b"\n"
    return bytes(out)


def soup(n, key, seed):
    """n bytes of seeded short lines (at most ~130 bytes each) of words, `key` and pieces of it among them"""
    blk = _soup_block(key, seed)
    return (blk * (n // len(blk) + 1))[:n]


_FLAT = b"0.1 2,3;4 5-6:7 8_9 " * 8


def flat(s, n):
    """n bytes without a '\\n', a NUL or a letter (no program's key), varying with the offset s"""
    return (_FLAT[s % 20:] + _FLAT * (n // len(_FLAT) + 1))[:n]


class _Canvas:
    def __init__(self, B, a, key, vend, seed):
        assert B % ROW == 0 and 0 <= a < 16 and len(key) <= 8
        self.B, self.a, self.key, self.K, self.vend = B, a, key, len(key), vend
        self.v = bytearray(soup(vend, key, seed))          # indexed by VIRTUAL offset; [0, a) is not part of the input
        self.v[vend - 1] = NL
        self.edges, self.no_start, self.claims, self.nul = [], set(), [], False
        self.claim(a, a + self.K + 1)
        self.v[a:a + self.K + 1] = key + b" "              # the first line starts a key at byte 0
        self.edges.append(Edge("first:key_at_byte_0", a))

    def claim(self, s, e):
        assert self.a <= s < e <= self.vend, (s, e, self.vend)
        assert all(e <= s0 or e0 <= s for s0, e0 in self.claims), ("placed stretches overlap", s, e)
        self.claims.append((s, e))

    def put(self, off, b):
        self.v[off:off + len(b)] = b

    def keys_around(self, off):
        self.put(off - self.K, self.key + self.key)

    def edge(self, name, off):
        self.edges.append(Edge(name, off))

    def head(self, L, r, name):
        """the first line start of lane L at its offset r: a stretch without '\\n' from in front of the lane to the '\\n' at r - 1"""
        lo = L * self.B
        X, K = lo + r, self.K
        self.claim(lo - 24, X + K + 2)
        self.put(lo - 24, flat(lo, X + K + 2 - (lo - 24)))
        self.v[X - 1] = NL
        self.put(X - 1 - K, self.key)
        self.put(X, self.key)
        self.edge("head:" + name, X)

    def head_none(self, L):
        """a '\\n' at B - 1, the only one of lane L: the line starts at the next lane's offset 0 and lane L has no start"""
        lo, hi, K = L * self.B, (L + 1) * self.B, self.K
        self.claim(lo - 24, hi + K + 2)
        self.put(lo - 24, flat(lo, hi + K + 2 - (lo - 24)))
        self.v[hi - 1] = NL
        self.put(hi - 1 - K, self.key)
        self.put(hi, self.key)
        self.no_start.add(L)
        self.edge("head:nl_at_B-1_next_lane_starts_at_0", hi)

    def head_two_nl(self, L):
        """'\\n' at both -1 and 0 of lane L: an empty line at its offset 0"""
        lo, K = L * self.B, self.K
        self.claim(lo - 24, lo + K + 3)
        self.put(lo - 24, flat(lo, K + 27))
        self.v[lo - 1] = self.v[lo] = NL
        self.put(lo - 1 - K, self.key)
        self.put(lo + 1, self.key)
        self.edge("head:nl_at_-1_and_0", lo)

    def empty_lines(self, L, count=300):
        """`count` empty lines across the start of lane L"""
        lo, K = L * self.B, self.K
        s = lo - count // 2
        self.claim(s - K - 1, s + count + K + 1)
        self.put(s - K - 1, b" " + self.key + bytes([NL]) * count + self.key + b" ")
        self.edge("run:%d_empty_lines" % count, s)

    def tail(self, L, name, d):
        """the last line of lane L starts 30 bytes in front of the lane's end hi and ends with the '\\n' at hi + d"""
        hi, K = (L + 1) * self.B, self.K
        X, s = hi + d, hi - 30
        self.claim(s - 1, X + K + 3)
        self.v[s - 1] = NL
        self.put(s, flat(s, X + K + 3 - s))
        self.v[X] = NL
        self.put(X - K, self.key)
        self.put(X + 1, self.key)
        if d >= self.B - 1:
            self.no_start.add(L + 1)
        self.edge("tail:" + name, X)

    def one_line(self, L, m, name):
        """ONE line from 10 bytes in front of lane L to 10 bytes behind lane L + m - 1: m lanes without a line start; keys on both sides of
        every lane edge in it and every 97 bytes"""
        s, e, K = L * self.B - 10, (L + m) * self.B + 10, self.K
        assert e - s < LONG
        self.claim(s - 1, e + 1)
        self.v[s - 1] = self.v[e] = NL
        self.put(s, flat(s, e - s))
        for off in range(s + 40, e - 40, 97):
            self.put(off, self.key)
        for j in range(L, L + m + 1):
            self.put(j * self.B - K - 1, b" " + self.key + self.key + b" ")
            self.edge("inline:%s:lane_%d" % (name, j), j * self.B)
        self.no_start.update(range(L, L + m))

    def split(self, E, i, kind):
        """the key with its first i bytes below E (i = K: it ends at E and the next one starts there)"""
        K = self.K
        assert 1 <= i <= K and SPLIT_KINDS[kind](E, self.B), (E, i, kind)
        text = b" " + self.key + (self.key if i == K else b"") + b" "
        self.claim(E - i - 1, E - i - 1 + len(text))
        self.put(E - i - 1, text)
        self.edge("split:%s:%d" % (kind, i), E)

    def case(self, name):
        assert len(self.v) == self.vend
        data = bytes(self.v[self.a:])
        return Case(name, data, self.a, self.B, tuple(self.edges), tuple(sorted(self.no_start)), tuple(expected_redo(data, self.a, self.B)), self.nul)


def expected_redo(data, a, B):
    """the lanes the window kernel hands to the redo pass, from WtLane::init and WtLane::check restated by hand (see the module's docstring)"""
    v = b"\xaa" * a + data
    vend, out = len(v), []
    for k in range((vend + B - 1) // B):
        lo, hi = k * B, min(k * B + B, vend)
        if lo < a + PIECE or hi + 3 * PIECE > vend:
            out.append(k)
            continue
        if v[lo - 1] != NL and not 0 <= v.find(b"\n", lo, hi - 1):
            continue                                        # no line start in [lo, hi): a '\n' at hi - 1 starts the NEXT lane's line
        room = vend - lo - 3 * PIECE
        e = v.find(b"\n", hi - 1)
        if e < 0:
            out.append(k)                                   # no line end before the input's: walks on until `check` stops it
            continue
        last_rv = (e - lo) // PIECE * PIECE + (PIECE if (e - lo) % PIECE >= PIECE - 16 else 0)
        if last_rv > room:
            out.append(k)
    return out


MAIN_LANES = 600


def main(B, a, key):
    """the edges of the issue's groups 1 - 4 in ONE buffer of 600 lanes (two workgroup edges, nine wave edges), soup between them"""
    c = _Canvas(B, a, key, MAIN_LANES * B + 100, 1)
    K = c.K
    deep = 3 * ROW if B >= 1024 else 0                      # (larger lanes: the residues in the lane's fourth output row)
    # Lane 1 starts behind the redone lane 0.  Everywhere else the bytes at a lane's first line start are ALSO written by the lane that owns the
    # line in front of it (it walks on to the end of the piece its '\n' lies in, and stores whole blocks); the redo pass writes its own lines
    # and no more: only here the bytewise head of WtLane::emit is the one writer of those bytes.
    c.head(1, 35, "lane_1_behind_the_redone_lane")
    L = 2
    for r in HEAD_RESIDUES:                                 # 1. the head
        c.head(L, (deep + r) % B, "residue_%d" % r)
        L += 2
    c.head(L, B - 40, "last_piece")
    c.head(L + 2, B - 1, "at_B-1")
    c.head_none(L + 4)
    c.head_two_nl(L + 7)
    c.empty_lines(L + 11)
    L += 15
    for name, d in tails(B).items():                        # 3. the tail
        c.tail(L, name, d)
        L += 4
    pos = {"dword": 36, "block": 48, "piece": 64, "row": ROW if B > ROW else 0, "lane": 0}
    for kind in ("dword", "block", "piece", "row", "lane"):  # 4. a key across five kinds of edge, at every inner position, and ending there
        for i in range(1, K + 1):
            c.split(L * B + pos[kind], i, kind)
            L += 1
    for m in (1, 2, 3):                                     # 2. no line start in a lane
        if m * B + 20 < LONG:
            c.one_line(L + 1, m, "%d_lane%s" % (m, "s" if m > 1 else ""))
        L += m + 3
    assert L < 250, L
    if 2 * B + 20 < LONG:
        c.one_line(255, 2, "across_workgroup_edge")
    else:
        c.one_line(256, 1, "across_workgroup_edge")
    if 65 * B + 20 < LONG:
        c.one_line(320, 65, "whole_wave")
    c.split(192 * B, K, "wave")
    c.split(448 * B, 1, "wave")
    c.split(576 * B, max(K - 1, 1), "wave")
    c.split(512 * B, max(K // 2, 1), "workgroup")
    return c.case("main")


END_LANES = 8
VEND_RESIDUES = (0, 1, 16, 63, 64, 65, 191, 192, 193)


def ends(B, a, key):
    """5. the ends of the input and 6. a NUL: one small buffer (eight lanes and a bit) per case"""
    out = []
    for r in VEND_RESIDUES:
        c = _Canvas(B, a, key, END_LANES * B + r, 10 + r)
        c.edge("end:vend_%d" % r, c.vend)
        out.append(c.case("vend_%d" % r))
    long_final = 3 * B if 3 * B < LONG else 3 * B // 2
    for name, n in (("1", 1), ("64", 64), ("193", 193), ("long", long_final)):
        c = _Canvas(B, a, key, END_LANES * B + 77, 30 + len(name))
        s = c.vend - n
        c.claim(s - 1, c.vend)
        c.v[s - 1] = NL
        c.put(s, flat(s, n))
        if n >= 64:                                          # (the final line starts and ends with the key; its last byte is no '\n')
            c.put(s, key)
            c.put(c.vend - c.K, key)
        c.edge("final:%s" % name, s)
        out.append(c.case("final_" + name))
    for name, L, r in (("lane_end", 3, B - 1), ("lane_start", 4, 0), ("skipped_head", 3, 3), ("last_piece", None, None)):
        c = _Canvas(B, a, key, END_LANES * B + 77, 40 + len(name))
        if name == "skipped_head":
            c.head(3, 40, "behind_a_nul")
        off = L * B + r if L is not None else c.vend - 30
        if name != "skipped_head":
            c.claim(off - c.K - 1, off + c.K + 2)
            c.put(off - c.K - 1, b" " + key + b"\0" + key + b" ")
        else:
            c.v[off] = 0
        c.nul = True
        c.edge("nul:" + name, off)
        out.append(c.case("nul_" + name))
    return out


@functools.lru_cache(maxsize=None)
def cases(B, a, key):
    """the cases for lanes of B bytes, an input a bytes off 16-byte alignment and a program whose key is `key` (built once: a tuple)"""
    out = [main(B, a, key)] + ends(B, a, key)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


NAMES = ["main"] + ["vend_%d" % r for r in VEND_RESIDUES] + ["final_1", "final_64", "final_193", "final_long"] + \
        ["nul_lane_end", "nul_lane_start", "nul_skipped_head", "nul_last_piece"]


def program(tag):
    return next(p for p in PROGRAMS if p.tag == tag)
