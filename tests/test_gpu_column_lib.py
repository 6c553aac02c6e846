"""The two checks that the GPU tests of the column calls share (tests/gpu_column_lib.py: assert_prefix, assert_untouched), on CPU
tensors: they pass on an untouched tail and fail on one changed element — the first behind the prefix, the last of the pad, one in
between, and one inside the prefix.  The guard that the shared check is no weaker than the copies it replaced."""
import pytest

from gpu_column_lib import BFILL, FILL, PAD, assert_prefix, assert_untouched

WANT = {"bytes": bytes(range(1, 18)), "words": list(range(100, 117))}


def array(kind, used):
    """a sentinel-filled array with `used` elements written and the pad behind them: (tensor, the expectation)"""
    import torch
    dtype, fill = (torch.uint8, BFILL) if kind == "bytes" else (torch.int64, FILL)
    t = torch.full((used + PAD,), fill, dtype=dtype)
    want = WANT[kind][:used]
    t[:used] = torch.tensor(list(want), dtype=dtype)
    return t, want


@pytest.mark.parametrize("used", (0, 1, 17))
@pytest.mark.parametrize("kind", ("bytes", "words"))
def test_prefix_and_tail(kind, used):
    t, want = array(kind, used)
    assert_prefix(t, want)
    assert_untouched(t[used:])
    for at in (used, used + PAD - 1, used + PAD // 2):
        t, want = array(kind, used)
        t[at] += 1
        with pytest.raises(AssertionError):
            assert_prefix(t, want, ("tail", at))
        with pytest.raises(AssertionError):
            assert_untouched(t[used:], ("tail", at))
    for at in range(used):
        t, want = array(kind, used)
        t[at] += 1
        with pytest.raises(AssertionError):
            assert_prefix(t, want, ("prefix", at))
    if used:
        with pytest.raises(AssertionError):
            assert_prefix(array(kind, used)[0], want[:-1])             # a shorter expectation: the tail starts inside the data


def test_the_sentinel_goes_by_the_element_size():
    import torch
    assert_untouched(torch.full((PAD,), BFILL, dtype=torch.uint8))
    assert_untouched(torch.full((PAD,), FILL, dtype=torch.int64))
    with pytest.raises(AssertionError):
        assert_untouched(torch.full((PAD,), FILL & 0xFF, dtype=torch.uint8))
