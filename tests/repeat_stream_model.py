"""Repeat-capture skipping across calls restated in numpy on top of tests/repeat_skip_model.py (include/cimbar_hip.h "repeat-capture skipping
across calls", libcimbar_amd/csrc/repeat.hip.inc "runs across calls"): the carry as a small object, a call's plan in front of any decode (the
walk seeded with the carried run, segments, their P, list 1), list 2, roles, the cumulative per-run fill and the new carry. The GPU tests
compare the device's outputs with these, bit for bit.

The walk is RM.walk over a VIRTUAL batch: min(len, max_run) stand-ins for the carried run's members (usable, agreeing in every cell) in front
of the call's captures. That is the rule's own wording -- capture 0 continues the carried run iff both are usable, they agree and the run has
fewer than max_run members -- and not the arithmetic the kernel uses."""
import dataclasses

import numpy as np

from libcimbar_amd import geometry
from tests import repeat_skip_model as RM


@dataclasses.dataclass
class Carry:
    """what a once-stream call leaves: the last capture's signature and usable word; len, P and the row of its run (0 / 0 / zeros when it is
    unusable). NOTHING (usable False, no signature) after create or reset."""
    sig: object = None
    usable: bool = False
    length: int = 0
    P: int = 0
    row: object = None


NOTHING = Carry()


@dataclasses.dataclass
class Plan:
    sigs: np.ndarray      # (n, NCELLS)
    agree: np.ndarray     # (n,) entry 0 against the carry, 0 when the carry is unusable
    runs: np.ndarray      # (n,) the run of every capture in this call's numbering, -1: in no run
    members: list         # the segments: every run's members in this call
    continued: int        # run 0 continues the carried run
    seg_p: list           # P of every segment
    list1: list


def agreement(carry, sigs):
    sigs = np.asarray(sigs)
    first = int((carry.sig == sigs[0]).sum()) if carry.usable else 0
    return np.concatenate([np.array([first], np.uint32), RM.agreement(sigs)]).astype(np.uint32)


def plan(mode, carry, frames, usable=None, min_agree_permille=0, max_run=0, sigs=None):
    geo = geometry.for_mode(mode)
    sigs = RM.signatures(mode, frames) if sigs is None else np.asarray(sigs)
    n = len(sigs)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    agree = agreement(carry, sigs)
    cap = RM.RUN_DEFAULT if max_run <= 0 else max_run
    v = min(carry.length, cap) if carry.usable else 0           # the stand-ins of the carried run's members
    v_agree = np.concatenate([np.full(max(v - 1, 0), geo.NCELLS, np.uint32), agree if v else agree[1:]])
    v_usable = np.concatenate([np.ones(v, bool), usable])
    v_runs, v_members = RM.walk(geo.NCELLS, v_agree, v_usable, min_agree_permille, max_run)
    continued = int(v > 0 and v_runs[v] >= 0 and v_runs[v] == v_runs[v - 1])
    first = (int(v_runs[v - 1]) if continued else int(v_runs[v - 1]) + 1) if v else 0      # the virtual id of this call's run 0
    runs = np.where(v_runs[v:] >= 0, v_runs[v:] - first, -1).astype(np.int32)
    members = [[j - v for j in m if j >= v] for m in v_members[first:]]
    assert all(members) and len(members) == (int(runs.max()) + 1 if n else 0)
    seg_p = [carry.P if (r == 0 and continued) else 0 for r in range(len(members))]
    list1 = [RM.representative(m) for m, p in zip(members, seg_p) if p != geo.FULL_MASK]
    return Plan(sigs, agree, runs, members, continued, seg_p, list1)


def fallback_list(mode, pl, rep_masks):
    """list 2: the other members, in capture order, of every segment with P | (its representative's mask) not full; rep_masks by list-1 position"""
    full = geometry.for_mode(mode).FULL_MASK
    out, j = [], 0
    for m, p in zip(pl.members, pl.seg_p):
        if p == full:
            continue
        if (p | int(rep_masks[j])) != full:
            out += [k for k in m if k != RM.representative(m)]
        j += 1
    return sorted(out)


def roles(n, pl, list2):
    return RM.roles(n, pl.runs, pl.list1, list2)


def run_fill(mode, n, pl, carry, chunks, masks):
    """the cumulative rows: RM.run_fill over the segments, then the carried row wherever the segment's P has the bit; rmasks |= P"""
    geo = geometry.for_mode(mode)
    rchunks, rmasks = RM.run_fill(mode, n, pl.members, chunks, masks)
    for r, p in enumerate(pl.seg_p):
        rmasks[r] |= np.uint32(p)
        for j in range(geo.CHUNKS_PER_FRAME):
            if (p >> j) & 1:
                rchunks[r, j] = carry.row[j]
    return rchunks, rmasks


def new_carry(n, pl, carry, usable, rchunks, rmasks):
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    r = int(pl.runs[n - 1])
    if r < 0:
        return Carry(pl.sigs[n - 1].copy(), False, 0, 0, None)
    assert usable[n - 1]
    length = (carry.length if (r == 0 and pl.continued) else 0) + len(pl.members[r])
    return Carry(pl.sigs[n - 1].copy(), True, length, int(rmasks[r]), rchunks[r].copy())


def boundaries(mode, sigs, cuts, usable=None, min_agree_permille=0, max_run=0):
    """bool (len(sigs),): capture k starts a run, over the calls sigs[cuts[i]:cuts[i + 1]] made one after the other from NOTHING. The chunks
    play no part in the walk, so the carry is stepped with P = 0."""
    geo = geometry.for_mode(mode)
    n = len(sigs)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    carry, out = NOTHING, np.zeros(n, bool)
    zc, zm = np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8), np.zeros(n, np.uint32)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m = hi - lo
        pl = plan(mode, carry, None, usable[lo:hi], min_agree_permille, max_run, sigs=sigs[lo:hi])
        for r, mem in enumerate(pl.members):
            if not (r == 0 and pl.continued):
                out[lo + mem[0]] = True
        rc, rm = run_fill(mode, m, pl, carry, zc[:m], zm[:m])
        carry = new_carry(m, pl, carry, usable[lo:hi], rc, rm)
    return out


def plain_boundaries(mode, sigs, usable=None, min_agree_permille=0, max_run=0):
    """... and what ONE plain once-call reports for the concatenation"""
    runs, members = RM.walk(geometry.for_mode(mode).NCELLS, RM.agreement(sigs), usable, min_agree_permille, max_run)
    out = np.zeros(len(sigs), bool)
    out[[m[0] for m in members]] = True
    return out
