"""What the GPU tests of the column calls share (test_gpu_{records,strings,match_strings,find_strings,span_strings,split_strings,
filter_strings,field_strings}.py and test_gpu_column_calls_interleaved.py): a column on the device at a chosen misalignment,
sentinel-filled output arrays with a pad behind the room, the two checks of what a call left of them, the read-back, and the
sequence of input sizes that makes the buffers the calls share grow and shrink.  The two checks take any tensor: they are tested
on CPU tensors in test_gpu_column_lib.py."""
import random

from span_lib import pack  # noqa: F401  (the column of a list of strings: (bytes, offsets))

FILL = -7                   # the sentinel of the int64 arrays
BFILL = 0xA5                # ... of the byte arrays
PAD = 8                     # sentinel elements behind the room a call is given
STR_TILE = 16384            # a tile of the staged text of the string calls
REC_TILE = 65536            # ... of the records call
LARGE = 330 * 1024


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(data, mis=0):
    """the bytes on the device, at an address that is `mis` past a 16-byte boundary"""
    import torch
    t = torch.zeros(len(data) + 32, dtype=torch.uint8, device=dev())
    at = (-t.data_ptr()) % 16 + mis
    v = t[at:at + len(data)]
    if data:
        v.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    assert len(data) == 0 or v.data_ptr() % 16 == mis % 16
    return v


def off_dev(off):
    import torch
    return torch.tensor(list(off), dtype=torch.int64, device=dev())


def words(n):
    import torch
    return torch.full((n,), FILL, dtype=torch.int64, device=dev())


def carve(cap, mis=0):
    """a sentinel-filled byte array of cap + PAD bytes on the device, `mis` past a 16-byte boundary"""
    import torch
    t = torch.full((cap + PAD + 32,), BFILL, dtype=torch.uint8, device=dev())
    at = (-t.data_ptr()) % 16 + mis
    return t[at:at + cap + PAD]


def blob(t):
    return t.cpu().numpy().tobytes()


def lst(t):
    return t.cpu().numpy().tolist()


def sentinel(t):
    return BFILL if t.element_size() == 1 else FILL


def assert_prefix(t, want, label=None):
    """the used prefix of a sentinel-filled array is `want` (bytes for a byte array, a list for a word array) and everything
    behind it is still the sentinel"""
    used = len(want)
    assert (blob(t[:used]) if isinstance(want, bytes) else lst(t[:used])) == want, label
    assert bool((t[used:] == sentinel(t)).all()), label


def assert_untouched(t, label=None):
    """a sentinel-filled array is all sentinel still"""
    assert bool((t == sentinel(t)).all()), label


def bitmap_of(valid, nrec):
    """the bitmap's bytes and what lies behind them, from the sentinel-filled words"""
    nw = (nrec + 63) // 64
    return blob(valid[:nw]), lst(valid[nw:])


def soup(rng, alphabet, n, longest=30):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, longest))) for _ in range(n)]


def sequence(seed, tiny, word, framed=True):
    """the inputs of an interleaved test by label, each a list of strings; word(rng, k): a string of k bytes.  A tile is STR_TILE
    bytes of the staged text, which frames every string with one byte more; with framed=False it is STR_TILE bytes of the strings"""
    rng = random.Random(seed)
    large, total = [], 0
    while total < LARGE:
        large.append(word(rng, rng.choice((0, 0, 1, 2, 5, 17, 40, 100, 300, 2000))))
        total += len(large[-1])
    assert b"" in large and total + len(large) > 20 * STR_TILE and total > 5 * REC_TILE
    each, frames = STR_TILE // 16 - framed, 16 * framed
    tile = [word(rng, each) for _ in range(16)]
    more = tile[:15] + [word(rng, each + 1)]
    assert len(tiny) == 3 and sum(map(len, tile)) + frames == STR_TILE and sum(map(len, more)) + frames == STR_TILE + 1
    return {"tiny": [tiny], "large": large, "tiny again": [tiny], "none": [], "large again": large, "one tile": tile,
            "one tile and a byte": more}
