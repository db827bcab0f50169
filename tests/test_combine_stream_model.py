"""CPU: the closing schedule of multi-capture decoding across calls (tests/combine_stream_model.py) against the one-call grouping rule
(tests/combine_model.group_captures) on random inputs cut into calls at random points.

- the stream model's concatenated closed groups are group_captures' groups of the concatenation, for max_group 2, 4 and 8
- a call closes at most n + 1 groups (n without a flush), and reports each group in the call that holds its closing event
- an open group never has more than max_group - 1 members
- groups_out: call-local ids in closing order, GROUP_OPEN for the members left open, -1 for unusable captures
"""
import numpy as np
import pytest

from tests import combine_model as CM
from tests import combine_stream_model as SM

NCELLS = 300


def _captures(seed, n_frames=14):
    """runs of 1-7 copies of random "frames", some cells flipped in every copy, some captures unusable"""
    g = np.random.default_rng(seed)
    sym, col = [], []
    for _ in range(n_frames):
        fs, fc = g.integers(0, 16, NCELLS), g.integers(0, 4, NCELLS)
        for _ in range(int(g.integers(1, 8))):
            s, c = fs.copy(), fc.copy()
            flip = g.random(NCELLS) < g.choice([0.0, 0.05, 0.2])       # (0.2 twice over is below 750 per mille now and then: a break inside a run)
            s[flip] = g.integers(0, 16, int(flip.sum()))
            sym.append(s)
            col.append(c)
    sym, col = np.asarray(sym, np.uint8), np.asarray(col, np.uint8)
    usable = g.random(len(sym)) >= 0.1
    return sym, col, usable


def _cuts(g, n):
    """call sizes that sum to n: many calls of one capture among larger ones"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(n - sum(sizes), int(g.choice([1, 1, 1, 2, 3, 5, 9]))))
    return sizes


@pytest.mark.parametrize("max_group", [2, 4, 8])
@pytest.mark.parametrize("seed", range(6))
def test_stream_groups_equal_the_one_call_groups(seed, max_group):
    sym, col, usable = _captures(seed)
    n = len(sym)
    want = CM.group_captures(sym, col, usable, 0, max_group)
    want_groups = [CM.members(want, g) for g in range(CM.n_groups(want))]
    g = np.random.default_rng(1000 + seed)
    sizes = _cuts(g, n)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    model = SM.StreamModel(0, max_group)
    got, seen_open = [], 0
    for c, size in enumerate(sizes):
        lo = int(starts[c])
        last = c == len(sizes) - 1
        out, closed, gsizes = model.call(sym[lo:lo + size], col[lo:lo + size], usable[lo:lo + size], flush=last)
        assert len(closed) <= size + (1 if last else 0)                # n + 1 with the flush, n without
        assert gsizes == [len(m) for m in closed]
        assert len(model.open) <= max_group - 1
        seen_open = max(seen_open, len(model.open))
        # groups_out: ids in closing order for the call's own members, OPEN for what stays, -1 for the unusable
        for k in range(size):
            if not usable[lo + k]:
                assert out[k] == -1
            elif out[k] == SM.GROUP_OPEN:
                assert (c, k) in [src for _, _, src in model.open]
            else:
                assert (c, k) in closed[out[k]]
        ids = [int(v) for v in out if v >= 0]
        assert ids == sorted(ids)
        got += [[int(starts[cc]) + kk for cc, kk in members] for members in closed]
    assert not model.open
    assert got == want_groups
    if max_group > 2:
        assert seen_open >= 2                                          # the inputs do carry groups of several members across calls


def test_one_capture_per_call_and_the_cap():
    sym = np.zeros((6, NCELLS), np.uint8)
    col = np.zeros((6, NCELLS), np.uint8)
    res = SM.run([(sym[k:k + 1], col[k:k + 1], None) for k in range(6)], [False] * 5 + [True], 0, 4)
    assert [r[0].tolist() for r in res] == [[SM.GROUP_OPEN]] * 3 + [[0], [SM.GROUP_OPEN], [0]]
    assert [r[2] for r in res] == [[], [], [], [4], [], [2]]            # the full group closes with its fourth member, no flush needed
    assert res[3][1] == [[(0, 0), (1, 0), (2, 0), (3, 0)]]


def test_flush_with_nothing_open_and_n_zero():
    model = SM.StreamModel()
    out, closed, gsizes = model.call(np.zeros((0, NCELLS), np.uint8), np.zeros((0, NCELLS), np.uint8), flush=True)
    assert len(out) == 0 and closed == [] and gsizes == []
    with pytest.raises(ValueError):
        model.call(np.zeros((0, NCELLS), np.uint8), np.zeros((0, NCELLS), np.uint8), flush=False)
    with pytest.raises(ValueError):
        SM.StreamModel(0, 9)


def test_unusable_capture_closes_the_carried_group():
    sym = np.zeros((3, NCELLS), np.uint8)
    col = np.zeros((3, NCELLS), np.uint8)
    model = SM.StreamModel()
    out, closed, _ = model.call(sym[:2], col[:2])
    assert out.tolist() == [SM.GROUP_OPEN] * 2 and closed == []
    out, closed, gsizes = model.call(sym[2:], col[2:], usable=[False])
    assert out.tolist() == [-1] and closed == [[(0, 0), (0, 1)]] and gsizes == [2]
    assert model.call(sym[:0], col[:0], flush=True)[1] == []
