"""CPU: tests/stitch_stream_model.py (torn-capture stitching across calls) held to tests/stitch_model.stitch_batch.

Random symbol and colour arrays with planted bands on both axes (consecutive captures agree on a run of lines, like torn captures do), some
captures unusable, cut into calls at random places, single captures included. Rows 1... of every call, and row 0 of every call behind the
first, are the one-shot pairs -- records, counts and cells -- in order; the first row of a stream is a non-candidate without counts, and so is
a row 0 whose carried capture was unusable (the one-shot pair is then a non-candidate as well).
"""
import numpy as np
import pytest

from libcimbar_amd import geometry
from tests import stitch_model as SM
from tests import stitch_stream_model as SSM

MODES = [68, 67, 66, 4, 8]


def _sequence(mode, axis, n, g):
    """n captures: capture k + 1 repeats capture k on a random run of lines (sometimes none, sometimes all), fresh noise elsewhere"""
    geo = geometry.for_mode(mode)
    line, L, _ = SM.lines_of(mode, axis)
    ncol = 1 << geo.COLOR_BITS
    sym = np.zeros((n, geo.NCELLS), np.uint8)
    col = np.zeros((n, geo.NCELLS), np.uint8)
    sym[0], col[0] = g.integers(0, 16, geo.NCELLS), g.integers(0, ncol, geo.NCELLS)
    for k in range(1, n):
        sym[k], col[k] = g.integers(0, 16, geo.NCELLS), g.integers(0, ncol, geo.NCELLS)
        kind = g.integers(0, 6)
        if kind == 0:
            continue                                   # nothing shared
        a, b = (0, L) if kind == 1 else sorted(g.choice(L + 1, 2, replace=False))   # kind 1: the whole frame (the group decode's case)
        keep = (line >= a) & (line < b)
        if kind == 2 and b - a > 4:                    # a band with damaged lines inside
            for l in g.choice(np.arange(a + 1, b - 1), int(g.integers(1, max(2, (b - a) // 3))), replace=False):
                keep &= line != l
        sym[k][keep], col[k][keep] = sym[k - 1][keep], col[k - 1][keep]
    usable = g.random(n) > 0.15
    return sym, col, usable


def _cuts(n, g):
    """a random composition of n, single captures included"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(min(n - sum(sizes), g.choice([1, 1, 2, 3, 5]))))
    return sizes


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_any_cut_reports_the_one_shot_pairs(mode, axis):
    g = np.random.default_rng(900 + 2 * mode + axis)
    n = 14
    sym, col, usable = _sequence(mode, axis, n, g)
    for params in ((0, 0), (900, 5)):
        want_tears, want_cnt, want_cells = SM.stitch_batch(mode, sym, col, axis, *params, usable=usable)
        assert (want_tears[:, 0] >= 0).any() and (want_tears[:, 0] < 0).any()      # candidates and non-candidates both
        for sizes in ([1] * n, [n], _cuts(n, g), _cuts(n, g), _cuts(n, g)):
            model = SSM.StitchStreamModel(mode)
            at = 0
            for size in sizes:
                tears, cnt, cells = model.call(sym[at:at + size], col[at:at + size], axis, *params, usable=usable[at:at + size])
                assert tears.shape == (size, 4) and cnt.shape[0] == size and cells.shape[0] == 2 * size
                # rows 1...: the one-shot pairs at - 1 + r
                assert (tears[1:] == want_tears[at:at + size - 1]).all(), (sizes, at)
                assert (cnt[1:] == want_cnt[at:at + size - 1]).all(), (sizes, at)
                assert (cells[2:] == want_cells[2 * at:2 * (at + size - 1)]).all(), (sizes, at)
                if at == 0 or not usable[at - 1]:
                    # no usable carry: a non-candidate without counts (the one-shot pair of an unusable capture is no candidate either)
                    assert tears[0].tolist() == [-1, -1, -1, 0] and not cnt[0].any() and not cells[:2].any(), (sizes, at)
                    assert at == 0 or want_tears[at - 1, 0] == -1
                else:
                    assert (tears[0] == want_tears[at - 1]).all() and (cnt[0] == want_cnt[at - 1]).all(), (sizes, at)
                    assert (cells[:2] == want_cells[2 * (at - 1):2 * at]).all(), (sizes, at)
                at += size
                assert (model.carry[0] == sym[at - 1]).all() and (model.carry[1] == col[at - 1]).all() and model.carry[2] == bool(usable[at - 1])


def test_parameters_belong_to_the_reporting_call_and_a_refused_call_leaves_the_carry():
    mode = 66
    g = np.random.default_rng(77)
    sym, col, _ = _sequence(mode, 0, 2, g)
    line, L, _ = SM.lines_of(mode, 0)
    keep = (line >= 20) & (line < 28)
    sym[1], col[1] = g.integers(0, 16, sym.shape[1]), g.integers(0, 4, sym.shape[1])
    sym[1][keep], col[1][keep] = sym[0][keep], col[0][keep]
    model = SSM.StitchStreamModel(mode)
    first = model.call(sym[:1], col[:1], axis=1, min_band=1)
    assert first[0].tolist() == [[-1, -1, -1, 0]]
    for bad in (dict(axis=2), dict(axis=0, min_band=L + 1)):
        with pytest.raises(ValueError):
            model.call(sym[1:], col[1:], **bad)
    with pytest.raises(ValueError):
        model.call(sym[:0], col[:0])
    assert (model.carry[0] == sym[0]).all()
    # the same carried capture, judged by the second call's axis and band
    assert model.call(sym[1:], col[1:], axis=0, min_band=9)[0].tolist() == [[-1, -1, -1, 8]]
    model.carry = (sym[0], col[0], True)
    assert model.call(sym[1:], col[1:], axis=0)[0].tolist() == [[20, 28, 24, 8]]
    model.reset()
    assert model.call(sym[1:], col[1:], axis=0)[0].tolist() == [[-1, -1, -1, 0]]
