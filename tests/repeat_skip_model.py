"""Repeat-capture skipping restated in numpy (include/cimbar_hip.h "repeat-capture skipping", libcimbar_amd/csrc/repeat.hip.inc): the ink
signature of a deskewed frame, the agreement of neighbours, the run walk, representatives, the two decode lists, roles, and the per-run fill
given per-capture chunks and masks. The GPU tests compare the device's outputs with these, bit for bit."""
import numpy as np

from libcimbar_amd import geometry

AGREE_DEFAULT, RUN_DEFAULT = 900, 4
UNUSABLE, SKIPPED, REP, FALLBACK = -1, 0, 1, 2


def cell_sums(mode, frame):
    """(NCELLS, 3) uint64: R_c, S_c, B_c over pixel rows y + 2 .. y + 5 and columns x .. x + 7 of every cell's nominal position"""
    geo = geometry.for_mode(mode)
    assert frame.shape == geo.FRAME_SHAPE and frame.dtype == np.uint8
    xy = geo.cell_positions()
    rows = xy[:, 1, None] + np.arange(2, 6)[None, :]                       # (NCELLS, 4)
    cols = xy[:, 0, None] + np.arange(8)[None, :]                          # (NCELLS, 8)
    px = frame[rows[:, :, None], cols[:, None, :]].astype(np.uint64)       # (NCELLS, 4, 8, 3)
    rgb = px.sum(axis=(1, 2))
    return np.stack([rgb[:, 0], rgb.sum(axis=1), rgb[:, 2]], axis=1)


def signature(mode, frame):
    """(NCELLS,) uint8: [R_c S_A > S_c R_A] | [B_c S_A > S_c B_A] << 1, strict, in unsigned 64-bit integers"""
    s = cell_sums(mode, frame)
    RA, SA, BA = (np.uint64(s[:, k].sum()) for k in range(3))
    red = s[:, 0] * SA > s[:, 1] * RA
    blue = s[:, 2] * SA > s[:, 1] * BA
    return (red.astype(np.uint8) | (blue.astype(np.uint8) << 1)).astype(np.uint8)


def signatures(mode, frames):
    return np.stack([signature(mode, f) for f in frames])


def agreement(sigs):
    """(n - 1,) uint32: the cells of equal signature in captures k and k + 1"""
    sigs = np.asarray(sigs)
    return (sigs[:-1] == sigs[1:]).sum(axis=1).astype(np.uint32)


def permille(mode, a, b):
    """the agreement of two frames in permille of the cells, rounded down"""
    n = geometry.for_mode(mode).NCELLS
    return int((signature(mode, a) == signature(mode, b)).sum()) * 1000 // n


def walk(ncells, agree, usable=None, min_agree_permille=0, max_run=0):
    """runs[k] (-1: in no run) and the member lists of the runs, by the rule of the header"""
    n = len(agree) + 1
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    min_agree = AGREE_DEFAULT if min_agree_permille <= 0 else min_agree_permille
    max_run = RUN_DEFAULT if max_run <= 0 else max_run
    runs = np.full(n, -1, np.int32)
    members = []
    for k in range(n):
        if not usable[k]:
            continue
        new = (k == 0 or not usable[k - 1] or int(agree[k - 1]) * 1000 < min_agree * ncells or len(members[-1]) >= max_run)
        if new:
            members.append([])
        members[-1].append(k)
        runs[k] = len(members) - 1
    return runs, members


def representative(members):
    return members[(len(members) - 1) // 2]


def plan(mode, frames, usable=None, min_agree_permille=0, max_run=0, sigs=None):
    """what can be said in front of any decode: (sigs, agree, runs, members, list1)"""
    sigs = signatures(mode, frames) if sigs is None else sigs
    agree = agreement(sigs)
    runs, members = walk(geometry.for_mode(mode).NCELLS, agree, usable, min_agree_permille, max_run)
    return sigs, agree, runs, members, [representative(m) for m in members]


def fallback_list(mode, members, rep_masks):
    """list 2: the other members, in capture order, of every run whose representative's mask (rep_masks, by run) is not full"""
    full = geometry.for_mode(mode).FULL_MASK
    out = []
    for m, mask in zip(members, rep_masks):
        if int(mask) != full:
            out += [k for k in m if k != representative(m)]
    return sorted(out)


def roles(n, runs, list1, list2):
    r = np.where(np.asarray(runs) < 0, UNUSABLE, SKIPPED).astype(np.int32)
    r[list(list1)] = REP
    r[list(list2)] = FALLBACK
    return r


def run_fill(mode, n, members, chunks, masks):
    """(rchunks (n, CHUNKS, CHUNK), rmasks (n,)) from the per-capture chunks and masks: the OR of the members' masks; chunk j from the
    representative where it delivered it, else from the lowest-index member that did, else zeros; zero slots from the run count on"""
    geo = geometry.for_mode(mode)
    rchunks = np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    rmasks = np.zeros(n, np.uint32)
    for r, m in enumerate(members):
        rep = representative(m)
        for k in m:
            rmasks[r] |= np.uint32(masks[k])
        for j in range(geo.CHUNKS_PER_FRAME):
            order = [rep] + [k for k in m if k != rep]
            for k in order:
                if (int(masks[k]) >> j) & 1:
                    rchunks[r, j] = chunks[k, j]
                    break
    return rchunks, rmasks
