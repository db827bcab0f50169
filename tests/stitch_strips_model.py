"""A numpy restatement of torn-capture stitching strip by strip (include/cimbar_hip.h, cimbar_hip_set_stitch_strips; csrc/stitch.hip.inc
k_stitch_pairs_strips), written from the rule rather than from the kernel.

lines, L, eq, min_agree_permille and min_band are tests/stitch_model.py's. With S strips, for consecutive captures k and k+1 and an axis:
  strip      across(i) = the cell's index on the other axis (axis 0: its grid column, A = DIM_X; axis 1: its grid row, A = DIM_Y);
             strip(i) = across(i) * S // A. width(l, j) = the cells of line l in strip j.
  flag(l, j) cnt(l, j) * 1000 >= min_agree_permille * width(l, j), cnt(l, j) = the sum of eq over those cells
  per strip  a_j = the lowest flagged line, b_j = the highest flagged line + 1, f_j = the flagged lines; located iff f_j >= 1,
             b_j - a_j >= min_band and 4 f_j >= 3 (b_j - a_j); its own split (a_j + b_j) >> 1
  candidate  both captures usable, 2 * located >= S, and some located strip with a_j > 0 or b_j < L
  splits     a located strip keeps its own; any other takes the split of the nearest located strip by index, the lower index on a tie
  cells      direction 0: cell i from capture k+1 if line(i) < s_strip(i), else from capture k; direction 1 the reverse
  record     {min a_j, max b_j over the located strips, s_(S >> 1), sum f_j}; a non-candidate {-1, -1, -1, sum f_j}

decide(flags (S, L) bool, L, S, min_band, usable) -> (tear (4,), strips (S, 4) {a_j, b_j, s_j, f_j}: a_j = b_j = -1 for a strip that is not
                                                      located, s_j = the resolved split, -1 in a non-candidate)
stitch_pair(mode, sym0, col0, sym1, col1, axis, strips, ...) -> (tear, strips, cnt (S, L) uint16, cells (2, NCELLS) uint8, zero for a non-candidate)
stitch_batch(mode, symbols, colors, axis, strips, ...)       -> (tears (n-1, 4), strips (n-1, S, 4), cnt (n-1, S, L), cells (2 (n-1), NCELLS))
"""
import numpy as np

from libcimbar_amd import geometry
from tests import stitch_model as SM


def strips_of(mode, axis, S):
    """(strip (NCELLS,) int, width (S, L) int) of the mode's cells on `axis` with S strips"""
    if not 1 <= S <= 8:
        raise ValueError("strips must be 1 .. 8")
    geo = geometry.for_mode(mode)
    xy = geo.cell_positions()
    line, L, _ = SM.lines_of(mode, axis)
    across = (xy[:, axis] - geo.OFFSET) // geo.PITCH
    A = geo.DIM_X if axis == 0 else geo.DIM_Y
    strip = across * S // A
    width = np.zeros((S, L), np.int64)
    np.add.at(width, (strip, line), 1)
    return strip, width


def decide(flags, L, S, min_band, usable=True):
    flags = np.asarray(flags, bool).reshape(S, L)
    out = np.full((S, 4), -1, np.int32)
    own = {}
    for j in range(S):
        idx = np.flatnonzero(flags[j])
        f = len(idx)
        out[j, 3] = f
        if f >= 1:
            a, b = int(idx[0]), int(idx[-1]) + 1
            if b - a >= min_band and 4 * f >= 3 * (b - a):
                out[j, :2] = (a, b)
                own[j] = (a + b) >> 1
    fsum = int(out[:, 3].sum())
    partial = any(out[j, 0] > 0 or out[j, 1] < L for j in own)
    if not (usable and 2 * len(own) >= S and partial):
        return np.array([-1, -1, -1, fsum], np.int32), out
    for j in range(S):
        # the nearest located strip by index; sorted() is stable, so the lower index wins a tie
        out[j, 2] = own[sorted(own, key=lambda q: abs(q - j))[0]]
    loc = sorted(own)
    return np.array([out[loc, 0].min(), out[loc, 1].max(), out[S >> 1, 2], fsum], np.int32), out


def stitch_pair(mode, sym0, col0, sym1, col1, axis=0, strips=1, min_agree_permille=0, min_band=0, usable=True):
    geo = geometry.for_mode(mode)
    S = int(strips)
    min_agree, min_band = SM.resolve(mode, axis, min_agree_permille, min_band)
    line, L, _ = SM.lines_of(mode, axis)
    strip, width = strips_of(mode, axis, S)
    s0, s1 = np.asarray(sym0, np.uint8), np.asarray(sym1, np.uint8)
    c0, c1 = np.asarray(col0, np.uint8), np.asarray(col1, np.uint8)
    cmask = (1 << geo.COLOR_BITS) - 1
    eq = ((s0 & 15) == (s1 & 15)) & ((c0 & cmask) == (c1 & cmask))
    cnt = np.zeros((S, L), np.int64)
    np.add.at(cnt, (strip[eq], line[eq]), 1)
    tear, rec = decide(cnt * 1000 >= min_agree * width, L, S, min_band, usable)
    cells = np.zeros((2, geo.NCELLS), np.uint8)
    if tear[0] >= 0:
        low = line < rec[strip, 2]
        cells[0] = np.where(low, (c1 << 4) | (s1 & 15), (c0 << 4) | (s0 & 15))
        cells[1] = np.where(low, (c0 << 4) | (s0 & 15), (c1 << 4) | (s1 & 15))
    return tear, rec, cnt.astype(np.uint16), cells


def stitch_batch(mode, symbols, colors, axis=0, strips=1, min_agree_permille=0, min_band=0, usable=None):
    n = len(symbols)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    geo = geometry.for_mode(mode)
    S = int(strips)
    _, L, _ = SM.lines_of(mode, axis)
    p = max(n - 1, 0)
    tears, recs = np.zeros((p, 4), np.int32), np.zeros((p, S, 4), np.int32)
    cnt, cells = np.zeros((p, S, L), np.uint16), np.zeros((2 * p, geo.NCELLS), np.uint8)
    for k in range(p):
        tears[k], recs[k], cnt[k], cells[2 * k:2 * k + 2] = stitch_pair(mode, symbols[k], colors[k], symbols[k + 1], colors[k + 1], axis, S,
                                                                        min_agree_permille, min_band, bool(usable[k] and usable[k + 1]))
    return tears, recs, cnt, cells
