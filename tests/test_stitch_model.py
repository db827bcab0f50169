"""CPU: the rule of torn-capture stitching (tests/stitch_model.py) on hand-made arrays and on oracle-decoded torn frames, the capture-path
inputs the GPU test uses, and the library's new C symbols.

- hand-made arrays, mode 66, both axes: band, split and both directions; a band over the whole frame, no flagged line and a band shorter than
  min_band are no candidates; the 3/4 rule and the permille threshold on both sides of their edges; the narrow anchor lines use their own width
- rendered frames torn at the positions of tests/stitch_cases.py (the ones the GPU tests use), decoded by the oracle, all five modes, both
  axes, both directions: the stitched cells in the pair's direction equal the shared frame's own oracle cells
- capture path: the 1080p pairs of tests/stitch_cases.py through the oracle's extractor and decoder: the stitched cells differ from the shared
  frame's stream in at most half the correctable bytes of any Reed-Solomon block (a condition on the inputs of the GPU test)
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

MODE = 66                                   # the smallest grid
AXES = (0, 1)


def _pair(axis, counts, seed=1):
    """two captures' (symbols, colours) of mode 66 whose first counts[l] cells of line l (in cell order) agree and whose other cells differ
    (alternately in the symbol and in the colour)"""
    geo = geometry.for_mode(MODE)
    g = np.random.default_rng(seed)
    s0, c0 = g.integers(0, 16, geo.NCELLS).astype(np.uint8), g.integers(0, 4, geo.NCELLS).astype(np.uint8)
    s1, c1 = s0.copy(), c0.copy()
    line, L, width = SM.lines_of(MODE, axis)
    for l in range(L):
        idx = np.flatnonzero(line == l)[int(counts[l]):]
        s1[idx[0::2]] = (s0[idx[0::2]] + 3) % 16
        c1[idx[1::2]] = (c0[idx[1::2]] + 1) % 4
    return s0, c0, s1, c1


def _band(axis, a, b, inside=None):
    """per-line agreement counts: every cell of the lines [a, b) (or `inside` of them), none of the others"""
    _, L, width = SM.lines_of(MODE, axis)
    counts = np.zeros(L, np.int64)
    counts[a:b] = width[a:b] if inside is None else inside
    return counts


@pytest.mark.parametrize("axis", AXES)
def test_band_split_and_both_directions(axis):
    line, L, width = SM.lines_of(MODE, axis)
    assert L == (69 if axis == 0 else 80) and width.sum() == geometry.for_mode(MODE).NCELLS
    for a, b in ((10, 31), (0, 20), (40, L), (33, 35)):
        s0, c0, s1, c1 = _pair(axis, _band(axis, a, b))
        tear, cnt, cells = SM.stitch_pair(MODE, s0, c0, s1, c1, axis)
        s = (a + b) >> 1
        assert tear.tolist() == [a, b, s, b - a]
        assert (cnt[a:b] == width[a:b]).all() and not cnt[:a].any() and not cnt[b:].any()
        k0, k1 = (c0 << 4) | s0, (c1 << 4) | s1
        assert (cells[0] == np.where(line < s, k1, k0)).all()
        assert (cells[1] == np.where(line < s, k0, k1)).all()
        assert (cells[0][line >= s] == k0[line >= s]).all() and (cells[0][line < s] == k1[line < s]).all()


@pytest.mark.parametrize("axis", AXES)
def test_no_candidates(axis):
    _, L, width = SM.lines_of(MODE, axis)
    # the band over the whole frame: two captures of one frame
    tear, cnt, cells = SM.stitch_pair(MODE, *_pair(axis, width), axis)
    assert tear.tolist() == [-1, -1, -1, L] and not cells.any() and (cnt == width).all()
    # ... but one line short of it at either end is a candidate
    assert SM.stitch_pair(MODE, *_pair(axis, _band(axis, 1, L)), axis)[0].tolist() == [1, L, (1 + L) >> 1, L - 1]
    assert SM.stitch_pair(MODE, *_pair(axis, _band(axis, 0, L - 1)), axis)[0].tolist() == [0, L - 1, (L - 1) >> 1, L - 1]
    # no flagged line
    tear, cnt, cells = SM.stitch_pair(MODE, *_pair(axis, np.zeros(L, int)), axis)
    assert tear.tolist() == [-1, -1, -1, 0] and not cells.any() and not cnt.any()
    # a band shorter than min_band (default 2)
    one = _pair(axis, _band(axis, 30, 31))
    assert SM.stitch_pair(MODE, *one, axis)[0].tolist() == [-1, -1, -1, 1]
    assert SM.stitch_pair(MODE, *one, axis, min_band=2)[0].tolist() == [-1, -1, -1, 1]
    assert SM.stitch_pair(MODE, *one, axis, min_band=1)[0].tolist() == [30, 31, 30, 1]
    five = _pair(axis, _band(axis, 30, 35))
    assert SM.stitch_pair(MODE, *five, axis, min_band=5)[0].tolist() == [30, 35, 32, 5]
    assert SM.stitch_pair(MODE, *five, axis, min_band=6)[0].tolist() == [-1, -1, -1, 5]
    # an unusable capture
    assert SM.stitch_pair(MODE, *five, axis, usable=False)[0].tolist() == [-1, -1, -1, 5]
    # what the library refuses
    for bad in (dict(axis=2), dict(axis=-1), dict(axis=axis, min_band=L + 1)):
        with pytest.raises(ValueError):
            SM.stitch_pair(MODE, *five, **bad)
    assert SM.stitch_pair(MODE, *five, axis, min_band=L)[0].tolist() == [-1, -1, -1, 5]


@pytest.mark.parametrize("axis", AXES)
def test_three_quarter_rule_on_both_sides_of_its_edge(axis):
    # a band of 8 lines: with 2 of the inner lines damaged 4 * 6 >= 3 * 8 holds, with 3 it does not
    counts = _band(axis, 20, 28)
    counts[[22, 25]] = 0
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [20, 28, 24, 6]
    counts[23] = 0
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [-1, -1, -1, 5]
    # a stray flagged line far from the band stretches b - a and fails the rule the same way
    counts = _band(axis, 20, 28)
    counts[60] = SM.lines_of(MODE, axis)[2][60]
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [-1, -1, -1, 9]


@pytest.mark.parametrize("axis", AXES)
def test_permille_threshold_on_both_sides_of_its_edge(axis):
    _, L, width = SM.lines_of(MODE, axis)
    w = int(width[30])
    assert w == (80 if axis == 0 else 69)
    need = -(-750 * w // 1000)                      # the smallest count with count * 1000 >= 750 * width: 60 | 52
    assert need * 1000 >= 750 * w > (need - 1) * 1000
    counts = _band(axis, 30, 40)
    counts[30] = need
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [30, 40, 35, 10]
    counts[30] = need - 1
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [31, 40, 35, 9]
    # the caller's threshold: 900 per mille
    need9 = -(-900 * w // 1000)
    counts[30] = need9
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis, min_agree_permille=900)[0].tolist() == [30, 40, 35, 10]
    counts[30] = need9 - 1
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis, min_agree_permille=900)[0].tolist() == [31, 40, 35, 9]
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis, min_agree_permille=0)[0].tolist() == [30, 40, 35, 10]


@pytest.mark.parametrize("axis", AXES)
def test_anchor_lines_use_their_own_width(axis):
    _, L, width = SM.lines_of(MODE, axis)
    narrow, full = int(width[2]), int(width[30])
    assert (narrow, full) == ((68, 80) if axis == 0 else (57, 69)) and (width[:6] == narrow).all() and (width[-6:] == narrow).all()
    need = -(-750 * narrow // 1000)                 # 51 | 43: below what a full line needs (60 | 52)
    assert need < -(-750 * full // 1000)
    counts = _band(axis, 2, 12)
    counts[2:6] = need
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [2, 12, 7, 10]
    counts[2] = need - 1
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [3, 12, 7, 9]
    counts = _band(axis, L - 12, L - 1)
    counts[L - 6:L - 1] = need
    assert SM.stitch_pair(MODE, *_pair(axis, counts), axis)[0].tolist() == [L - 12, L - 1, (2 * L - 13) >> 1, 11]


def test_batch_layout():
    geo = geometry.for_mode(MODE)
    a = _pair(0, _band(0, 10, 30), seed=2)
    b = _pair(0, _band(0, 40, 60), seed=3)
    S, C = np.stack([a[0], a[2], b[0], b[2]]), np.stack([a[1], a[3], b[1], b[3]])
    tears, cnt, cells = SM.stitch_batch(MODE, S, C, 0)
    assert tears.shape == (3, 4) and cnt.shape == (3, geo.DIM_Y) and cells.shape == (6, geo.NCELLS)
    assert tears[0].tolist() == [10, 30, 20, 20] and tears[2].tolist() == [40, 60, 50, 20] and tears[1, 0] == -1
    assert not cells[2:4].any() and cells[0].any() and cells[5].any()
    assert SM.stitch_batch(MODE, S, C, 0, usable=[1, 0, 1, 1])[0][:, 0].tolist() == [-1, -1, 40]
    t1, n1, c1 = SM.stitch_batch(MODE, S[:1], C[:1], 1)
    assert t1.shape == (0, 4) and n1.shape == (0, geo.DIM_X) and c1.shape == (0, geo.NCELLS)


def _oracle_cells(mode, frame, preprocess=0, ccm=None):
    _, _, mask, ccm = pyref.oracle_decode(frame, preprocess, 2, ccm, mode=mode)
    s, c, _ = pyref.oracle_stage(mode=mode)
    return s, c, mask, ccm


@pytest.mark.parametrize("mode", SC.MODES)
def test_model_on_oracle_decoded_torn_frames(mode):
    geo = geometry.for_mode(mode)
    frames, _ = SC.rendered(mode)
    sB, cB, mB, _ = _oracle_cells(mode, frames[1])
    assert mB == geo.FULL_MASK
    want = (cB << 4) | (sB & 15)
    for axis in AXES:
        for direction in (0, 1):
            for name in SC.TEARS:
                p1, p2 = SC.tear_pixels(mode, axis, name)
                T1, T2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction)
                s1, c1, m1, _ = _oracle_cells(mode, T1)
                s2, c2, m2, _ = _oracle_cells(mode, T2)
                assert m1 != geo.FULL_MASK and m2 != geo.FULL_MASK
                tear, _, cells = SM.stitch_pair(mode, s1, c1, s2, c2, axis)
                a, b, s, f = tear.tolist()
                # the band is the lines both captures show of B, to within the line a tear cuts through
                l1, l2 = (p1 - geo.OFFSET) / geo.PITCH, (p2 - geo.OFFSET) / geo.PITCH
                assert l1 <= a <= l1 + 1 and l2 - 1 <= b <= l2 + 1 and f == b - a, (mode, axis, direction, name, tear)
                assert (cells[direction] == want).all(), (mode, axis, direction, name, int((cells[direction] != want).sum()))
                assert (cells[1 - direction] != want).sum() > geo.NCELLS // 2


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
@pytest.mark.parametrize("case", SC.CAPTURE_CASES, ids=lambda c: "axis%d-dir%d-%s" % c)
def test_capture_path_inputs_leave_half_the_correction_margin(oracle, case, fmt):
    axis, direction, name = case
    geo = geometry.for_mode(68)
    frames, _ = SC.rendered(68)
    sB, cB, _, _ = _oracle_cells(68, frames[1])
    caps, (w, h) = SC.capture_pairs(axis, direction, name, fmt)
    ccm = pyref.CoCcm()
    got = []
    for k in range(4):                                   # in batch order, the colour-correction matrix carried as the capture path carries it
        frame = np.zeros(geo.FRAME_SHAPE, np.uint8)
        assert oracle.co_extract_fmt(P(caps[k]), w, h, fmt, P(frame), None) > 0
        s, c, mask, ccm = _oracle_cells(68, frame, preprocess=1, ccm=ccm)
        got.append((s, c, mask))
    assert got[0][2] == got[3][2] == geo.FULL_MASK and got[1][2] != geo.FULL_MASK and got[2][2] != geo.FULL_MASK
    tear, _, cells = SM.stitch_pair(68, got[1][0], got[1][1], got[2][0], got[2][1], axis)
    assert tear[0] >= 0
    errors = _stream_block_errors(geo, cells[direction], (cB << 4) | (sB & 15))
    print("bytes in error per block: max", errors.max(), "sum", errors.sum())
    assert errors.max() <= geo.RS_PARITY // 2 // 2       # half of what a block corrects (15 of 155 bytes): 7


def test_library_exports_the_stitched_entry_points():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = ctypes.CDLL(decoder.LIB_PATH)
    for name in ("cimbar_hip_decode_batch_stitched", "cimbar_hip_scan_extract_decode_batch_stitched_fmt"):
        assert hasattr(lib, name), name
    assert (decoder.TAP_STITCH_CELLS, decoder.TAP_STITCH_LINES) == (18, 19)
