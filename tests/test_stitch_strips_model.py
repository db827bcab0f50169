"""CPU: the strip rule of torn-capture stitching (tests/stitch_strips_model.py; include/cimbar_hip.h, cimbar_hip_set_stitch_strips) on
hand-made arrays and on oracle-decoded frames, and the conditions tests/test_gpu_stitch_strips.py rests on.

- hand-made flags on both sides of each clause: half the strips located, an unlocated strip inheriting its split (with a tie), every located
  strip over the whole frame, min_band and the 3/4 rule per strip, an unusable capture; mode 66 cells through stitch_pair: counts, widths,
  the per-strip split in both directions
- width(l, j) is positive for S <= 8 in every mode on both axes, 2 at the least (mode 66, axis 1, S = 8)
- S = 1 is tests/stitch_model.py: on the hand-made pairs and on the oracle-decoded torn frames of tests/stitch_cases.py
- the slanted tears of tests/stitch_strips_cases.py, decoded by the oracle, five modes x two axes x two directions x three parameter sets:
  the whole-line rule reports {-1, -1, -1, 0} (no line is flagged), and the strip rule at S = 4 and S = 8 returns the shared frame's own
  cells in every cell, in the pair's direction
- capture path: the 1080p slanted pairs through the oracle's extractor and decoder: the whole-line rule finds no candidate and the
  strip-stitched cells differ from the shared frame's stream in at most half the correctable bytes of any Reed-Solomon block
"""
import ctypes
import os

import numpy as np
import pytest

from libcimbar_amd import decoder, geometry
from oracle import pyref
from oracle.pyref import P
from tests import stitch_cases as SC
from tests import stitch_model as SM
from tests import stitch_strips_cases as XC
from tests import stitch_strips_model as XM

MODE = 66                                   # the smallest grid
AXES = (0, 1)
L0 = 40                                     # the lines of the hand-made flag arrays


def _flags(S, bands, L=L0):
    """(S, L) flags: strip j's lines [a, b) set for bands[j] = (a, b), none for None; a third element lists lines cleared again"""
    f = np.zeros((S, L), bool)
    for j, band in enumerate(bands):
        if band is not None:
            f[j, band[0]:band[1]] = True
            for l in (band[2] if len(band) > 2 else ()):
                f[j, l] = False
    return f


def test_half_the_strips_located():
    # S = 4: two located strips are enough, one is not
    tear, rec = XM.decide(_flags(4, [(10, 20), None, (12, 22), None]), L0, 4, 2)
    assert tear.tolist() == [10, 22, 17, 20] and rec[:, 2].tolist() == [15, 15, 17, 17]
    tear, rec = XM.decide(_flags(4, [(10, 20), None, None, None]), L0, 4, 2)
    assert tear.tolist() == [-1, -1, -1, 10] and rec.tolist() == [[10, 20, -1, 10]] + [[-1, -1, -1, 0]] * 3
    # S = 5: 2 * 3 >= 5, 2 * 2 < 5
    assert XM.decide(_flags(5, [(10, 20), None, (10, 20), None, (10, 20)]), L0, 5, 2)[0].tolist() == [10, 20, 15, 30]
    assert XM.decide(_flags(5, [(10, 20), None, (10, 20), None, None]), L0, 5, 2)[0].tolist() == [-1, -1, -1, 20]
    # S = 1 with its strip located, S = 2 with one of two
    assert XM.decide(_flags(1, [(10, 20)]), L0, 1, 2)[0].tolist() == [10, 20, 15, 10]
    assert XM.decide(_flags(2, [None, (10, 20)]), L0, 2, 2)[0].tolist() == [10, 20, 15, 10]
    # an unusable capture: the strips are located all the same, nothing is resolved
    tear, rec = XM.decide(_flags(2, [(8, 18), (10, 20)]), L0, 2, 2, usable=False)
    assert tear.tolist() == [-1, -1, -1, 20] and rec.tolist() == [[8, 18, -1, 10], [10, 20, -1, 10]]


def test_an_unlocated_strip_takes_the_nearest_located_split():
    # strip 1 lies between 0 and 2: the tie goes to the lower index; strip 3 has 2 next to it
    tear, rec = XM.decide(_flags(4, [(4, 10), None, (20, 30), None]), L0, 4, 2)
    assert rec[:, 2].tolist() == [7, 7, 25, 25] and tear.tolist() == [4, 30, 25, 16]
    # no tie: strips 1 and 2 each take the neighbour they touch
    tear, rec = XM.decide(_flags(4, [(4, 10), None, None, (20, 30)]), L0, 4, 2)
    assert rec[:, 2].tolist() == [7, 7, 25, 25]
    # S = 8: strip 0 takes the first located strip above it, strip 4 is two away from both 2 and 6 (the lower), 3 and 5 take the one they touch
    tear, rec = XM.decide(_flags(8, [None, (4, 10), (6, 12), None, None, None, (20, 30), (22, 32)]), L0, 8, 2)
    assert rec[:, 2].tolist() == [7, 7, 9, 9, 9, 25, 25, 27] and tear.tolist() == [4, 32, 9, 32]
    # the record's split is strip S >> 1's, located or not
    assert XM.decide(_flags(2, [(4, 10), None]), L0, 2, 2)[0].tolist() == [4, 10, 7, 6]
    assert XM.decide(_flags(3, [None, (4, 10), (20, 30)]), L0, 3, 2)[0].tolist() == [4, 30, 7, 16]


def test_every_located_strip_over_the_whole_frame_is_no_candidate():
    whole = (0, L0)
    tear, rec = XM.decide(_flags(4, [whole] * 4), L0, 4, 2)
    assert tear.tolist() == [-1, -1, -1, 4 * L0] and rec[:, :3].tolist() == [[0, L0, -1]] * 4
    # an unlocated strip beside them changes nothing
    assert XM.decide(_flags(4, [whole, None, whole, whole]), L0, 4, 2)[0].tolist() == [-1, -1, -1, 3 * L0]
    # one located strip one line short at either end: a candidate, and the whole-frame strips split in their middle
    tear, rec = XM.decide(_flags(4, [whole, whole, (1, L0), whole]), L0, 4, 2)
    assert tear.tolist() == [0, L0, (1 + L0) >> 1, 4 * L0 - 1] and rec[:, 2].tolist() == [L0 >> 1, L0 >> 1, (1 + L0) >> 1, L0 >> 1]
    assert XM.decide(_flags(4, [whole, (0, L0 - 1), whole, whole]), L0, 4, 2)[0].tolist() == [0, L0, L0 >> 1, 4 * L0 - 1]
    # a short strip that is not located does not count
    assert XM.decide(_flags(4, [whole, (5, 6), whole, whole]), L0, 4, 2)[0].tolist() == [-1, -1, -1, 3 * L0 + 1]


def test_min_band_and_the_three_quarter_rule_hold_per_strip():
    # a one-line band is located with min_band 1 only
    bands = [(10, 20), (10, 11), (10, 20), (10, 11)]
    tear, rec = XM.decide(_flags(4, bands), L0, 4, 2)
    assert rec[:, :2].tolist() == [[10, 20], [-1, -1], [10, 20], [-1, -1]] and rec[:, 3].tolist() == [10, 1, 10, 1] and tear[0] == 10
    tear, rec = XM.decide(_flags(4, bands), L0, 4, 1)
    assert rec[:, :3].tolist() == [[10, 20, 15], [10, 11, 10], [10, 20, 15], [10, 11, 10]] and tear.tolist() == [10, 20, 15, 22]
    # min_band 10 keeps the ten-line strips, 11 leaves none
    assert XM.decide(_flags(4, bands), L0, 4, 10)[0].tolist() == [10, 20, 15, 22]
    assert XM.decide(_flags(4, bands), L0, 4, 11)[0].tolist() == [-1, -1, -1, 22]
    # eight lines with two cleared pass 4 f >= 3 (b - a), with three they do not: that strip alone drops out
    tear, rec = XM.decide(_flags(2, [(20, 28, (22, 25)), (20, 28, (22, 24, 25))]), L0, 2, 2)
    assert rec.tolist() == [[20, 28, 24, 6], [-1, -1, 24, 5]] and tear.tolist() == [20, 28, 24, 11]
    # a stray flagged line far off stretches b_j - a_j the same way
    f = _flags(2, [(20, 28), (20, 28)])
    f[1, 39] = True
    assert XM.decide(f, L0, 2, 2)[1][:, :2].tolist() == [[20, 28], [-1, -1]]


def test_width_is_positive_in_every_mode():
    least = {}
    for mode in SC.MODES:
        for axis in AXES:
            line, L, width = SM.lines_of(mode, axis)
            for S in range(1, 9):
                strip, w = XM.strips_of(mode, axis, S)
                assert w.shape == (S, L) and (w.sum(axis=0) == width).all() and 0 <= strip.min() and strip.max() == S - 1
                assert w.min() > 0, (mode, axis, S)
                least[(mode, axis, S)] = int(w.min())
    assert min(least.values()) == 2 == least[(66, 1, 8)]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            XM.strips_of(66, 0, bad)


def _pair_strips(axis, S, bands, seed=1, short=None):
    """two captures' cells of mode 66 that agree in strip j on the lines bands[j] = [a, b) and nowhere else; short = (j, l, c): only the
    first c cells of line l in strip j agree"""
    geo = geometry.for_mode(MODE)
    g = np.random.default_rng(seed)
    s0, c0 = g.integers(0, 16, geo.NCELLS).astype(np.uint8), g.integers(0, 4, geo.NCELLS).astype(np.uint8)
    line, L, _ = SM.lines_of(MODE, axis)
    strip, _ = XM.strips_of(MODE, axis, S)
    agree = np.zeros(geo.NCELLS, bool)
    for j, band in enumerate(bands):
        if band is not None:
            agree |= (strip == j) & (line >= band[0]) & (line < band[1])
    if short is not None:
        j, l, c = short
        agree[np.flatnonzero((strip == j) & (line == l))[c:]] = False
    idx = np.flatnonzero(~agree)
    s1, c1 = s0.copy(), c0.copy()
    s1[idx[0::2]] = (s0[idx[0::2]] + 3) % 16
    c1[idx[1::2]] = (c0[idx[1::2]] + 1) % 4
    return s0, c0, s1, c1


@pytest.mark.parametrize("axis", AXES)
def test_cells_counts_and_the_permille_threshold_per_strip(axis):
    line, L, _ = SM.lines_of(MODE, axis)
    S = 4
    strip, width = XM.strips_of(MODE, axis, S)
    bands = [(10, 16), (13, 19), None, (19, 25)]          # a tear that rises nine lines over the frame, six shared lines
    s0, c0, s1, c1 = _pair_strips(axis, S, bands)
    tear, rec, cnt, cells = XM.stitch_pair(MODE, s0, c0, s1, c1, axis, S)
    assert rec.tolist() == [[10, 16, 13, 6], [13, 19, 16, 6], [-1, -1, 16, 0], [19, 25, 22, 6]] and tear.tolist() == [10, 25, 16, 18]
    for j, band in enumerate(bands):
        want = np.zeros(L, np.int64)
        if band is not None:
            want[band[0]:band[1]] = width[j, band[0]:band[1]]
        assert (cnt[j] == want).all()
    k0, k1 = (c0 << 4) | s0, (c1 << 4) | s1
    low = line < np.array([13, 16, 16, 22])[strip]
    assert (cells[0] == np.where(low, k1, k0)).all() and (cells[1] == np.where(low, k0, k1)).all()
    # the whole-line rule sees no line at 750 per mille: at most two strips of four agree on any line
    assert SM.stitch_pair(MODE, s0, c0, s1, c1, axis)[0].tolist() == [-1, -1, -1, 0]
    # the threshold is the strip's own width on that line: the smallest passing count, and one below
    w = int(width[1, 13])
    need = -(-750 * w // 1000)
    assert need * 1000 >= 750 * w > (need - 1) * 1000
    assert XM.stitch_pair(MODE, *_pair_strips(axis, S, bands, short=(1, 13, need)), axis, S)[1][1].tolist() == [13, 19, 16, 6]
    assert XM.stitch_pair(MODE, *_pair_strips(axis, S, bands, short=(1, 13, need - 1)), axis, S)[1][1].tolist() == [14, 19, 16, 5]
    need9 = -(-900 * w // 1000)
    assert XM.stitch_pair(MODE, *_pair_strips(axis, S, bands, short=(1, 13, need9 - 1)), axis, S, 900)[1][1].tolist() == [14, 19, 16, 5]
    # a non-candidate has zero cells and keeps its counts
    tear, rec, cnt2, cells = XM.stitch_pair(MODE, s0, c0, s1, c1, axis, S, usable=False)
    assert tear.tolist() == [-1, -1, -1, 18] and not cells.any() and (cnt2 == cnt).all() and (rec[:, 2] == -1).all()


def test_batch_layout():
    geo = geometry.for_mode(MODE)
    a = _pair_strips(0, 4, [(10, 16), (13, 19), None, (19, 25)], seed=2)
    b = _pair_strips(0, 4, [(40, 50)] * 4, seed=3)
    S, C = np.stack([a[0], a[2], b[0], b[2]]), np.stack([a[1], a[3], b[1], b[3]])
    tears, recs, cnt, cells = XM.stitch_batch(MODE, S, C, 0, 4)
    assert tears.shape == (3, 4) and recs.shape == (3, 4, 4) and cnt.shape == (3, 4, geo.DIM_Y) and cells.shape == (6, geo.NCELLS)
    assert tears[0].tolist() == [10, 25, 16, 18] and tears[2].tolist() == [40, 50, 45, 40] and tears[1, 0] == -1
    assert not cells[2:4].any() and cells[0].any() and cells[5].any()
    assert XM.stitch_batch(MODE, S, C, 0, 4, usable=[1, 0, 1, 1])[0][:, 0].tolist() == [-1, -1, 40]
    t1, r1, n1, c1 = XM.stitch_batch(MODE, S[:1], C[:1], 1, 8)
    assert t1.shape == (0, 4) and r1.shape == (0, 8, 4) and n1.shape == (0, 8, geo.DIM_X) and c1.shape == (0, geo.NCELLS)


def _same_as_the_plain_model(mode, s0, c0, s1, c1, axis, **kw):
    tear, cnt, cells = SM.stitch_pair(mode, s0, c0, s1, c1, axis, **kw)
    xtear, rec, xcnt, xcells = XM.stitch_pair(mode, s0, c0, s1, c1, axis, 1, **kw)
    assert xtear.tolist() == tear.tolist() and (xcnt[0] == cnt).all() and (xcells == cells).all()
    assert rec[0, 3] == tear[3] and rec[0, 2] == tear[2]
    return tear


@pytest.mark.parametrize("axis", AXES)
def test_one_strip_is_the_plain_model_on_hand_made_pairs(axis):
    _, L, _ = SM.lines_of(MODE, axis)
    for bands in ([(10, 31)], [(0, L)], [(1, L)], [(30, 31)], [None]):
        pair = _pair_strips(axis, 1, bands)
        for kw in ({}, dict(min_band=1), dict(min_agree_permille=990), dict(usable=False)):
            _same_as_the_plain_model(MODE, *pair, axis, **kw)


def _oracle_cells(mode, frame, preprocess=0, ccm=None):
    _, _, mask, ccm = pyref.oracle_decode(frame, preprocess, 2, ccm, mode=mode)
    s, c, _ = pyref.oracle_stage(mode=mode)
    return s, c, mask, ccm


@pytest.mark.parametrize("mode", SC.MODES)
def test_one_strip_is_the_plain_model_on_the_torn_frames(mode):
    frames, _ = SC.rendered(mode)
    seen = 0
    for axis in AXES:
        for direction in (0, 1):
            for name in SC.TEARS:
                p1, p2 = SC.tear_pixels(mode, axis, name)
                T1, T2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction)
                s1, c1, _, _ = _oracle_cells(mode, T1)
                s2, c2, _, _ = _oracle_cells(mode, T2)
                seen += _same_as_the_plain_model(mode, s1, c1, s2, c2, axis)[0] >= 0
    assert seen == 2 * 2 * len(SC.TEARS)
    # ... and on a batch with noise-damaged band lines on both sides of the 3/4 rule
    for axis in AXES:
        batch = SC.damaged_band_batch(mode, axis)
        cells = [_oracle_cells(mode, f)[:2] for f in batch]
        got = [_same_as_the_plain_model(mode, *cells[k], *cells[k + 1], axis)[0] >= 0 for k in range(len(batch) - 1)]
        assert got[0] and not got[3]


@pytest.mark.parametrize("mode", SC.MODES)
def test_slanted_tears_defeat_whole_lines_and_strips_recover_the_frame(mode):
    geo = geometry.for_mode(mode)
    frames, _ = SC.rendered(mode)
    sB, cB, mB, _ = _oracle_cells(mode, frames[1])
    assert mB == geo.FULL_MASK
    want = (cB << 4) | (sB & 15)
    for axis in AXES:
        for direction in (0, 1):
            for slant in XC.SLANTS:
                batch = XC.slanted_batch(mode, axis, direction, slant)
                s1, c1, m1, _ = _oracle_cells(mode, batch[1])
                s2, c2, m2, _ = _oracle_cells(mode, batch[2])
                what = (mode, axis, direction, slant)
                assert m1 != geo.FULL_MASK and m2 != geo.FULL_MASK, what
                tear, cnt, cells = SM.stitch_pair(mode, s1, c1, s2, c2, axis)
                assert tear.tolist() == [-1, -1, -1, 0] and not cells.any(), (what, tear.tolist())
                for S in XC.STRIPS:
                    tear, rec, _, cells = XM.stitch_pair(mode, s1, c1, s2, c2, axis, S)
                    assert tear[0] >= 0, (what, S, rec.tolist())
                    assert (cells[direction] == want).all(), (what, S, int((cells[direction] != want).sum()), rec.tolist())
                    assert (cells[1 - direction] != want).sum() > geo.NCELLS // 2, (what, S)


def test_damaged_strips_batch_has_located_and_unlocated_strips():
    for axis in AXES:
        batch = XC.damaged_strips_batch(MODE, axis)
        cells = [_oracle_cells(MODE, f)[:2] for f in batch]
        tear, rec, _, _ = XM.stitch_pair(MODE, *cells[0], *cells[1], axis, 4)
        assert tear[0] >= 0 and (rec[:, 0] >= 0).tolist() == [True, False, True, True] and rec[1, 2] == rec[0, 2], rec.tolist()
        tear, rec, _, _ = XM.stitch_pair(MODE, *cells[3], *cells[4], axis, 4)
        assert tear[0] == -1 and (rec[:, 0] >= 0).tolist() == [False, False, True, False] and (rec[:, 2] == -1).all(), rec.tolist()


def _stream_block_errors(geo, cells, want):
    """the bytes per Reed-Solomon block in which two cell sets' streams differ (modes 68 / 67 / 66: symbol blocks, then colour blocks)"""
    order = geo.interleave_indices()
    out = []
    for shift, bits in ((0, 4), (4, 2)):
        per = 8 // bits
        a = ((cells[order] >> shift) & ((1 << bits) - 1)).reshape(-1, per)
        b = ((want[order] >> shift) & ((1 << bits) - 1)).reshape(-1, per)
        out.append((a != b).any(axis=1).reshape(-1, geo.RS_BLOCK).sum(axis=1))
    return np.concatenate(out)


@pytest.mark.parametrize("fmt", SC.CAPTURE_FORMATS)
@pytest.mark.parametrize("case", XC.CAPTURE_CASES, ids=lambda c: "axis%d-dir%d" % c)
def test_capture_path_inputs_leave_half_the_correction_margin(oracle, case, fmt):
    axis, direction = case
    geo = geometry.for_mode(68)
    frames, _ = SC.rendered(68)
    sB, cB, _, _ = _oracle_cells(68, frames[1])
    caps, (w, h) = XC.capture_pairs_slanted(axis, direction, fmt)
    ccm = pyref.CoCcm()
    got = []
    for k in range(4):                                   # in batch order, the colour-correction matrix carried as the capture path carries it
        frame = np.zeros(geo.FRAME_SHAPE, np.uint8)
        assert oracle.co_extract_fmt(P(caps[k]), w, h, fmt, P(frame), None) > 0
        s, c, mask, ccm = _oracle_cells(68, frame, preprocess=1, ccm=ccm)
        got.append((s, c, mask))
    assert got[0][2] == got[3][2] == geo.FULL_MASK and got[1][2] != geo.FULL_MASK and got[2][2] != geo.FULL_MASK
    tear, cnt, _ = SM.stitch_pair(68, got[1][0], got[1][1], got[2][0], got[2][1], axis)
    print("gap", XC.CAPTURE_GAP, "whole lines:", tear.tolist(), "best line per mille", int((cnt * 1000 // SM.lines_of(68, axis)[2]).max()))
    assert tear[0] == -1                                 # the whole-line rule finds no candidate at XC.CAPTURE_GAP
    for S in XC.STRIPS:
        tear, rec, _, cells = XM.stitch_pair(68, got[1][0], got[1][1], got[2][0], got[2][1], axis, S)
        assert tear[0] >= 0, (S, rec.tolist())
        errors = _stream_block_errors(geo, cells[direction], (cB << 4) | (sB & 15))
        print("strips", S, "bytes in error per block: max", errors.max(), "sum", errors.sum())
        assert errors.max() <= geo.RS_PARITY // 2 // 2   # half of what a block corrects (15 of 155 bytes): 7


def test_library_exports_the_strip_setting():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = ctypes.CDLL(decoder.LIB_PATH)
    for name in ("cimbar_hip_set_stitch_strips", "cimbar_hip_get_stitch_strips"):
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS
    assert (decoder.TAP_STITCH_STRIPS, decoder.TAP_STITCH_STRIP_LINES) == (22, 23)
