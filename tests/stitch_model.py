"""A numpy restatement of torn-capture stitching (include/cimbar_hip.h, cimbar_hip_decode_batch_stitched; csrc/stitch.hip.inc
k_stitch_pairs), written from the rule rather than from the kernel.

For consecutive captures k and k+1 of a batch and an axis:
  lines      axis 0: line(i) = the cell's grid row (y_i - OFFSET) / PITCH, L = DIM_Y; axis 1: its grid column (x_i - OFFSET) / PITCH,
             L = DIM_X. width(l) = the cells on line l (smaller on the lines that cross the anchors).
  eq(i)      symbol and colour both equal, under the masks of the group decode's agreement count: symbol & 15, colour & (colours - 1)
  flag(l)    cnt(l) * 1000 >= min_agree_permille * width(l), cnt(l) = the sum of eq over the line; min_agree_permille <= 0 means 750
  band       a = the lowest flagged line, b = the highest flagged line + 1, f = the number of flagged lines
  candidate  both captures usable, f >= 1, b - a >= min_band (min_band <= 0 means 2), 4 f >= 3 (b - a), and a > 0 or b < L
  split      s = (a + b) >> 1. Direction 0: cell i comes from capture k+1 if line(i) < s, else from capture k; direction 1 the reverse.
             Symbol and colour are the chosen capture's.

stitch_pair(mode, sym0, col0, sym1, col1, axis, ...) -> (tear (4,) int32 {a, b, s, f}, a = b = s = -1 for a non-candidate,
                                                         cnt (L,) uint16,
                                                         cells (2, NCELLS) uint8 colour << 4 | symbol per direction, zero for a non-candidate)
stitch_batch(mode, symbols, colors, axis, ...)       -> (tears (n-1, 4), cnt (n-1, L), cells (2 (n-1), NCELLS)): pair k, direction d at 2k + d
    raises ValueError where the library returns CIMBAR_HIP_EINVAL (axis outside {0, 1}, min_band above L)
"""
import numpy as np

from libcimbar_amd import geometry


def lines_of(mode, axis):
    """(line (NCELLS,) int, L, width (L,) int) of the mode's cells on `axis`"""
    if axis not in (0, 1):
        raise ValueError("axis must be 0 or 1")
    geo = geometry.for_mode(mode)
    xy = geo.cell_positions()
    line = (xy[:, 1 - axis] - geo.OFFSET) // geo.PITCH
    L = geo.DIM_Y if axis == 0 else geo.DIM_X
    return line, L, np.bincount(line, minlength=L)


def resolve(mode, axis, min_agree_permille, min_band):
    _, L, _ = lines_of(mode, axis)
    if min_band > L:
        raise ValueError("min_band above the lines of the axis")
    return (750 if min_agree_permille <= 0 else int(min_agree_permille)), (2 if min_band <= 0 else int(min_band))


def stitch_pair(mode, sym0, col0, sym1, col1, axis=0, min_agree_permille=0, min_band=0, usable=True):
    geo = geometry.for_mode(mode)
    min_agree, min_band = resolve(mode, axis, min_agree_permille, min_band)
    line, L, width = lines_of(mode, axis)
    s0, s1 = np.asarray(sym0, np.uint8), np.asarray(sym1, np.uint8)
    c0, c1 = np.asarray(col0, np.uint8), np.asarray(col1, np.uint8)
    cmask = (1 << geo.COLOR_BITS) - 1
    eq = ((s0 & 15) == (s1 & 15)) & ((c0 & cmask) == (c1 & cmask))
    cnt = np.bincount(line[eq], minlength=L)
    flag = cnt.astype(np.int64) * 1000 >= min_agree * width.astype(np.int64)
    f = int(flag.sum())
    tear = np.array([-1, -1, -1, f], np.int32)
    cells = np.zeros((2, geo.NCELLS), np.uint8)
    if f >= 1:
        idx = np.flatnonzero(flag)
        a, b = int(idx[0]), int(idx[-1]) + 1
        if usable and b - a >= min_band and 4 * f >= 3 * (b - a) and (a > 0 or b < L):
            s = (a + b) >> 1
            tear[:3] = (a, b, s)
            low = line < s
            cells[0] = np.where(low, (c1 << 4) | (s1 & 15), (c0 << 4) | (s0 & 15))
            cells[1] = np.where(low, (c0 << 4) | (s0 & 15), (c1 << 4) | (s1 & 15))
    return tear, cnt.astype(np.uint16), cells


def stitch_batch(mode, symbols, colors, axis=0, min_agree_permille=0, min_band=0, usable=None):
    n = len(symbols)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    geo = geometry.for_mode(mode)
    _, L, _ = lines_of(mode, axis)
    resolve(mode, axis, min_agree_permille, min_band)
    p = max(n - 1, 0)
    tears, cnt, cells = np.zeros((p, 4), np.int32), np.zeros((p, L), np.uint16), np.zeros((2 * p, geo.NCELLS), np.uint8)
    for k in range(p):
        tears[k], cnt[k], cells[2 * k:2 * k + 2] = stitch_pair(mode, symbols[k], colors[k], symbols[k + 1], colors[k + 1], axis, min_agree_permille,
                                                               min_band, bool(usable[k] and usable[k + 1]))
    return tears, cnt, cells
