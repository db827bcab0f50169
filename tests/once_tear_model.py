"""Tear skipping restated in numpy from the wording of include/cimbar_hip.h ("Tear skipping"): the per-line counts of a capture's signature
against its two neighbours', the flags, the search for an orientation and a split, which captures are eligible (from
tests/repeat_skip_model.walk's runs), and lists 1 and 2 with the guard, given pass 1's masks. Nothing here comes from the kernel side; the
GPU tests compare the device's records, roles and lists with these, value for value."""
import functools

import numpy as np

from libcimbar_amd import geometry
from tests import repeat_skip_model as RM

LINE_DEFAULT, SIDE_DEFAULT = 750, 2
TORN = 3                                   # CIMBAR_HIP_ONCE_TORN
NO_TEAR = (-1, -1, 0, 0)


def resolve(line_permille=0, min_side=0):
    return (LINE_DEFAULT if line_permille <= 0 else line_permille), (SIDE_DEFAULT if min_side <= 0 else min_side)


@functools.lru_cache(maxsize=None)
def lines(mode, axis):
    """(line(i) of every cell, L, width(l)): axis 0 the grid rows, axis 1 the grid columns, as the stitched calls define them"""
    geo = geometry.for_mode(mode)
    xy = geo.cell_positions()
    line = (xy[:, 1 if axis == 0 else 0] - geo.OFFSET) // geo.PITCH
    L = geo.DIM_Y if axis == 0 else geo.DIM_X
    return line, L, np.bincount(line, minlength=L)


def line_counts(mode, axis, sig, other):
    """cnt(l): the cells on line l whose signature equals the other capture's"""
    line, L, _ = lines(mode, axis)
    return np.bincount(line[np.asarray(sig) == np.asarray(other)], minlength=L)


def pq(cnt_p, cnt_n, width, line_permille):
    """p(l) = flagP & ~flagN, q(l) = flagN & ~flagP, flag(l) = cnt(l) * 1000 >= line_permille * width(l)"""
    fp = np.asarray(cnt_p, np.int64) * 1000 >= line_permille * np.asarray(width, np.int64)
    fn = np.asarray(cnt_n, np.int64) * 1000 >= line_permille * np.asarray(width, np.int64)
    return fp & ~fn, fn & ~fp


def search(p, q, min_side):
    """the tear of one axis: (o, s, first, last) of the admissible pair with the largest first + last, ties to the lower o, then the lower
    s; None where no pair is admissible"""
    L = len(p)
    best = None
    for o in (0, 1):
        a, b = (p, q) if o == 0 else (q, p)
        for s in range(min_side, L - min_side + 1):
            first, last = int(a[:s].sum()), int(b[s:].sum())
            if 8 * first >= 7 * s and 8 * last >= 7 * (L - s):
                if best is None or first + last > best[2] + best[3]:
                    best = (o, s, first, last)
    return best


def tear(mode, prev, sig, nxt, axis, line_permille=0, min_side=0):
    """the record {axis * 2 + o, s, first, last} of an ELIGIBLE capture, NO_TEAR where it is no candidate. axis 2: either axis, axis 0's
    tear where both have one"""
    line_permille, min_side = resolve(line_permille, min_side)
    for ax in ((0, 1) if axis == 2 else (axis,)):
        _, _, width = lines(mode, ax)
        p, q = pq(line_counts(mode, ax, sig, prev), line_counts(mode, ax, sig, nxt), width, line_permille)
        found = search(p, q, min_side)
        if found:
            return (ax * 2 + found[0],) + found[1:]
    return NO_TEAR


def eligible(k, n, runs, members):
    return 1 <= k <= n - 2 and runs[k - 1] >= 0 and runs[k] >= 0 and runs[k + 1] >= 0 and len(members[runs[k]]) == 1


def records(mode, sigs, runs, members, axis, line_permille=0, min_side=0):
    """(n, 4) int32: the record of every capture"""
    n = len(sigs)
    out = np.tile(np.array(NO_TEAR, np.int32), (n, 1))
    for k in range(n):
        if eligible(k, n, runs, members):
            out[k] = tear(mode, sigs[k - 1], sigs[k], sigs[k + 1], axis, line_permille, min_side)
    return out


def candidates(rec):
    return [k for k in range(len(rec)) if rec[k][0] >= 0]


def list1(members, rec):
    """the representatives without the candidates, in capture order"""
    cand = set(candidates(rec))
    return [k for k in (RM.representative(m) for m in members) if k not in cand]


def second(mode, runs, members, rec, masks1):
    """(list 2, the torn captures) given masks1 = {capture: mask} of list 1's decode. A candidate is torn when the representatives of both
    neighbours' runs came back with full masks (a representative that is itself a candidate did not come back); every other candidate and
    the other members of every run whose representative is incomplete make list 2, in capture order."""
    full = geometry.for_mode(mode).FULL_MASK
    cand = candidates(rec)
    complete = lambda k: int(masks1.get(RM.representative(members[runs[k]]), 0)) == full
    torn = [k for k in cand if complete(k - 1) and complete(k + 1)]
    two = [k for k in cand if k not in torn]
    for m in members:
        rep = RM.representative(m)
        if rep not in cand and int(masks1[rep]) != full:
            two += [k for k in m if k != rep]
    return sorted(two), torn


def roles(n, runs, l1, l2, torn):
    r = RM.roles(n, runs, l1, l2)
    r[list(torn)] = TORN
    return r


def line_permilles(mode, axis, sig, other):
    """per line, the agreement with the other capture in permille of the line's cells, rounded down (the margins the tests assert)"""
    _, _, width = lines(mode, axis)
    return line_counts(mode, axis, sig, other) * 1000 // width
