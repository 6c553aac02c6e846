"""Inputs that make the state guesses of the exact sub-ranges WRONG with ordinary patterns and ordinary bytes, written once for
the CPU tier (tests/test_exact_repair_cases.py: the host shim) and the GPU tier (tests/gpu_repair_check.py, tests/test_gpu_exact_repair.py).
Pure Python: nothing here touches a GPU, the library or the oracle.

A lane guesses the state at the start `lo` of its sub-range from the 256 bytes before it (LOOK), the backward lanes of the guided families the
state at their end `hi` from the 256 bytes behind it.  A transducer whose state does not forget defeats that:
    forward    `aa:x` inside a run of `a`: the state is the parity of the distance to the run's start, the guess takes it from lo - 256.  Lanes and
               the look-back are even, so a run that starts at an ODD offset is guessed wrong in every lane it covers beyond the look-back, one
               that starts at an even offset in none.  Only the first such lane is flagged (the ones behind it agree with each other); the repair
               walks on through them to the end of its workgroup (G = 256 lanes), the next round starts at the next workgroup.
    backward   `(a|b)*c:x` inside a run of [ab]: the state at hi is "a `c` ends this run".  A run that goes on for more than 256 bytes behind hi
               and ends in `c` is guessed wrong in every lane it crosses; the rightmost is flagged and sweeps on to the left through the others.
`(ab:x|ba:yy)` synchronises itself and never misses: it is no provoking case.

Every builder takes the lane size L (the GPU tier runs 2048 and 128); a workgroup is G = 256 * L bytes.  A Case:
    name, pat, eng        the pattern and its engine ("nft" | "dft")
    family                "guided_gen" forced, or None: the family the library chooses
    data                  the input
    expect                ("forward", k): at least k forward repair rounds; ("backward", 1): at least one backward repair round — and no more:
                          of the lanes a run is guessed wrong in only the rightmost is flagged (the others agree with each other), its sweep goes
                          left through all of them whatever the workgroup, runs do not share a lane's guess, so ONE round settles every run;
                          ("none",): no repair round at all; None: nothing said about rounds, the bytes alone
    single                the forward rounds are decided by the input alone: ONE lane is flagged per round, the order in which lanes run cannot
                          change their number — 1 + the workgroup edges the wrongly guessed part of the run crosses (forward_rounds())

The oracle's time for every case of cases(2048) plus cases(128), measured where this file was written (one core, the C restatement under
oracle/): 3.1 s in all, the largest single case 0.4 s.  The NFT engine's cost grows with the square of the length of a run of [ab], so the
backward cases keep most runs at 300 - 1 500 bytes and have a handful of up to 4 700 (all far under 30 000: the reference's search stack holds
65 536 items)."""
import collections
import functools
import random

LOOK = 256                         # scan_block.hpp: kSpecLook, and the look-ahead of the backward lanes' guess
Case = collections.namedtuple("Case", "name pat eng family data expect single")

PARITY = [("aa:x", "nft"), ("aa:x", "dft"), ("(aa:x|a:y)", "nft")]          # two states inside a run of `a`: one flagged lane per round
THIRDS = ("aaa:xy", "dft")                                                   # three: lanes of 2 048 bytes are guessed wrong two times in three
BACKWARD = [("(a|b)*c:x", "nft"), ("(a|b)*c:x", "dft"), ("[ab]+c:X", "nft")]    # backward DFAs of 5 - 6 states: 4-bit symbols, two to a byte (sym_mode 2)
BYTE_SYMBOLS = ("((a|b)*c:x|d[e-h][e-h][e-h][e-h]g:y)", "nft")                   # 38 backward states: a symbol per byte (sym_mode 1)
# the forward programs that admit guided_gen run once more with that family forced: all of them do (test_exact_repair_cases.py checks that this
# is every program of PARITY and THIRDS whose allowed_kernels() has the family, so the list cannot lag behind the front end)
GUIDED = PARITY + [THIRDS]
SHORT = b"a short line with aa and aaa in it, abc abbc\n"


def filler(n, seed=3):
    """exactly n bytes of short lines (words over `a b c d` and blanks), the last byte a '\\n'"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choices(b"aabbcd  e", k=rng.randint(1, 70))) + b"\n"
    del out[n:]
    if n:
        out[-1] = 0x0A
    return bytes(out)


def flat(n):
    """n bytes without a '\\n' and without an `a` (a stretch longer than the look-back in front of a run: the guess has no line start to hold on to)"""
    return (b"the dog, the fox; " * (n // 18 + 1))[:n]


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------

def long_run(L, lead=1, edges=3):
    """a lead-in of `lead` bytes `b`, a run of `a` over `edges` workgroup edges (edges * G + 1001 bytes), `c\\n` and a short line"""
    return b"b" * lead + b"a" * (edges * 256 * L + 1001) + b"c\n" + SHORT


def forward_rounds(data, L):
    """repair rounds of a parity pattern on an input with ONE run of `a` longer than L + LOOK, from the geometry alone: 0 when the run starts
    at an even offset; else 1 for the first lane whose look-back begins inside the run, + 1 for every workgroup edge behind that lane's start
    and inside the run (the lane that starts there is the next one whose predecessor knows better)"""
    s = data.index(b"a" * (L + LOOK + 1))
    e = s
    while e < len(data) and data[e] == 0x61:
        e += 1
    if s % 2 == 0:
        return 0
    first = (s + LOOK) // L * L + L                   # the first lane start with lo - LOOK > s
    if first >= e:
        return 0
    G = 256 * L
    return 1 + len([k for k in range(G, e, G) if k > first])


def max_flagged_lanes(data, L):
    """an upper bound on the forward repair rounds of ANY order of execution, from the input alone: the most lanes of one run of `a` whose
    look-back begins inside the run (only they can guess wrong).  Every round settles at least the leftmost flagged lane of every run for good:
    the lane before it is not flagged and nothing upstream walks into it — a walk from an earlier run ends at the latest where that run ends,
    the state forgets there —, so its exit is final and the flagged lane starts from the truth."""
    worst, i, n = 0, 0, len(data)
    while i < n:
        s = data.find(b"a" * (LOOK + 1), i)
        if s < 0:
            break
        e = s
        while e < n and data[e] == 0x61:
            e += 1
        worst = max(worst, len(range((s + LOOK) // L * L + L, e + 1, L)))
        i = e
    return worst


def window_forward(L):
    """ten runs of 3 L + 1 bytes `a`, each in front of a lane start lo: the run's first byte at lo - d for d in (0, 1, 255, 256, 257), first with
    no line start within 600 bytes in front of it (a guess), then with a '\\n' right in front of it (a line start inside the window: the exact bit)"""
    out = bytearray(filler(4 * L, 5))
    k = 0
    for nl in (False, True):
        for d in (0, 1, 255, 256, 257):
            lo = (len(out) + 700 + 257) // L * L + L
            pre = lo - d - len(out)
            assert pre >= 700
            out += filler(pre - 600, 7 + k) + flat(600)
            if nl:
                out[-1] = 0x0A
            assert len(out) == lo - d
            out += b"a" * (3 * L + 1) + b"b c\n"
            k += 1
    return bytes(out + filler(L + 33, 6))


def many_runs(L):
    """forty seeded runs of 300 - 9 000 `a` separated by `b`, '\\n', ` c `, `bb` (the same bytes for every L): several flagged lanes to a workgroup"""
    rng = random.Random(40)
    out = bytearray(b"x")
    for k in range(40):
        out += b"a" * rng.randint(300, 9000) + (b"b", b"\n", b" c ", b"bb")[rng.randrange(4)]
    return bytes(out + b"\n" + SHORT)


def tail(L, more=0):
    """the long run up to the LAST byte of the buffer: no final newline, the length no multiple of L; `more`: that many bytes longer"""
    data = b"b" + b"a" * (256 * L + L // 2 + 76 + more)
    assert len(data) % L and data[-1:] == b"a"
    return data


# ---- backward --------------------------------------------------------------------------------------------------------------------------------

def _ab(rng, n):
    return bytes(rng.choices(b"ab", k=n))


def backward_runs(L):
    """thirty seeded runs of [ab], each ending in one of `c`, `d`, `c\\n`, '\\n', blank, between short lines: 28 of 300 - 1 500 bytes (300 is the
    shortest that misses a 256-byte guess), two of 2 500 and 4 000, one of more than 2 L + 600 that ends in `c` (it crosses a lane
    edge with more than the look-ahead behind it) — and one of 3 000 ending in `c` that lies across a multiple of G = 256 L (L = 2048: G itself): the repair
    walks left over a grid-block edge"""
    rng = random.Random(30)
    G = 256 * L
    ends = (b"c", b"d", b"c\n", b"\n", b" ")
    lengths = [rng.randint(300, 1500) for _ in range(28)] + [2500, 4000]
    rng.shuffle(lengths)
    out = bytearray(filler(333, 9))
    for k, n in enumerate(lengths):
        out += _ab(rng, n) + ends[k % 5] + b" " + filler(rng.randint(40, 400), 50 + k)
    out += b"d " + _ab(rng, 2 * L + 601) + b"c\n"
    edge = (len(out) + 3000 + G - 1) // G * G         # (L = 2048: G itself)
    out += filler(edge - 1500 - len(out), 10)
    out += _ab(rng, 3000) + b"c z\n" + filler(2 * L + 77, 12)
    assert b"\n" not in out[edge - 1400:edge + 1400]
    return bytes(out)


def window_backward(L):
    """six runs of [ab] from L + 10 bytes in front of a lane end hi to hi + d, where a `c` sits, d in (255, 256, 257) — and then a '\\n' in its place"""
    rng = random.Random(31)
    out = bytearray(filler(3 * L + 50, 13))
    for k, end in enumerate((b"c", b"c", b"c", b"\n", b"\n", b"\n")):
        d = (255, 256, 257)[k % 3]
        hi = (len(out) + 100) // L * L + 4 * L
        start = hi - L - 10
        out += filler(start - len(out), 14 + k)
        out += _ab(rng, hi + d - start) + end
        assert out[hi + d] == end[0]
        out += b" z\n" if end == b"c" else b""
    return bytes(out + filler(L + 21, 15))


# ---- the table -------------------------------------------------------------------------------------------------------------------------------

def _tag(pat, eng, family=None):
    names = {"aa:x": "aa", "(aa:x|a:y)": "aa_a", "aaa:xy": "aaa", "(a|b)*c:x": "star", "[ab]+c:X": "plus", BYTE_SYMBOLS[0]: "star_bytesym"}
    return "%s_%s%s" % (names[pat], eng, "_guided" if family else "")


@functools.lru_cache(maxsize=None)
def cases(L):
    """the cases for lanes of L bytes, in the order the jobs run them (built once: a tuple)"""
    out = []
    run, control = long_run(L), long_run(L, lead=2)
    wf, mr = window_forward(L), many_runs(L)

    def both(kind, progs, data, expect, single):
        """the family the library chooses, then guided_gen forced (the programs of GUIDED: the same scan behind a backward pass)"""
        for family in (None, "guided_gen"):
            for pat, eng in progs:
                if family is None or (pat, eng) in GUIDED:
                    out.append(Case(kind + "_" + _tag(pat, eng, family), pat, eng, family, data, expect, single and (pat, eng) != THIRDS))
    both("long_run", PARITY + [THIRDS], run, ("forward", 4), True)
    both("control", PARITY, control, ("none",), True)
    both("window_forward", [("aa:x", "nft"), ("aa:x", "dft"), THIRDS], wf, None, False)
    both("many_runs", [("aa:x", "nft"), THIRDS], mr, ("forward", 1), False)
    for more in (0, 5):
        out.append(Case("tail_%d_aa_nft" % more, "aa:x", "nft", None, tail(L, more), ("forward", 2), True))
        out.append(Case("tail_%d_aa_dft" % more, "aa:x", "dft", None, tail(L, more), ("forward", 2), True))
    br, wb = backward_runs(L), window_backward(L)
    for pat, eng in BACKWARD + [BYTE_SYMBOLS]:
        out.append(Case("backward_runs_" + _tag(pat, eng), pat, eng, None, br, ("backward", 1), False))
    for pat, eng in BACKWARD + [BYTE_SYMBOLS]:
        out.append(Case("window_backward_" + _tag(pat, eng), pat, eng, None, wb, None, False))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(L):
    return {c.name: c for c in cases(L)}


# ---- references written here: a left-to-right greedy replace per line, no regex engine ---------------------------------------------------------

GREEDY = {"aa:x": [(b"aa", b"x")], "(aa:x|a:y)": [(b"aa", b"x"), (b"a", b"y")], "aaa:xy": [(b"aaa", b"xy")]}


def greedy(pat, data):
    """what a scan under `pat` prints: at every position the first alternative that matches is replaced, else the byte is copied.  A run of `a`
    is the only place these patterns match, so a run of n is rewritten in closed form (the long runs have 1.5 million bytes)"""
    rules = GREEDY[pat]
    if data[-1:] != b"\n":                  # (the reference reads lines: the last byte of a last line without a '\n' goes where the '\n' would)
        data = data[:-1] + b"\n"
    out, i, n = [], 0, len(data)
    while i < n:
        j = data.find(b"a", i)
        if j < 0:
            out.append(data[i:])
            break
        out.append(data[i:j])
        i = j
        while i < n and data[i] == 0x61:
            i += 1
        run = i - j
        k, text = len(rules[0][0]), rules[0][1]
        out.append(text * (run // k))
        rest = run % k
        out.append(rules[1][1] * rest if len(rules) > 1 else b"a" * rest)
    return b"".join(out)
