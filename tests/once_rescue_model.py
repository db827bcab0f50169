"""The run rescue of the once-calls restated in numpy (include/cimbar_hip.h "Run rescue", libcimbar_amd/csrc/repeat.hip.inc "run rescue"),
and the inputs its tests share.

The rule, from the runs' members and the per-capture masks a once-call reports: which runs are tried, the word CIMBAR_HIP_TAP_ONCE_RESCUE
reports per run slot, and how a run row is put together from a group decode's chunks and the members' chunks. The group decode itself
(combined cells, Reed-Solomon, the erasure retry) is the combined call's and is not restated here: the GPU test takes it from
cimbar_hip_decode_batch_combined with groups_in = runs_out on a second context.

The inputs are the captures of tests/group_walk_cases.py: three rendered frames, the disjoint-disc pair of each (which the combined call is
shown to recover, group_walk_cases.RECOVERING), and the three-band triple of a frame. tests/test_once_rescue_model.py asserts on the CPU the
signature margins that make min_agree_permille = 500 join the pairs and the triples and split the frames.
"""
import functools

import numpy as np

from libcimbar_amd import geometry
from tests import group_walk_cases as GW
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

MIN_AGREE = 500        # joins a disc pair (823 .. 880) and the neighbours of a band triple (575 .. 595), splits two frames (254 .. 260)
MODES = (68, 67, 66)


# ------------------------------------------------------------------------------------------------ the rule
def tried(mode, members, masks):
    """per run: at least two members, all of them decoded -- the representative's mask is not full, so pass 2 took the rest -- and the OR
    of their masks is not full"""
    full = geometry.for_mode(mode).FULL_MASK
    out = []
    for m in members:
        rep = RM.representative(m)
        union = 0
        for k in m:
            union |= int(masks[k])
        out.append(len(m) >= 2 and int(masks[rep]) != full and union != full)
    return out


def tap_words(mode, n, members, masks, row_masks):
    """(n,) int32, CIMBAR_HIP_TAP_ONCE_RESCUE: -1 for a run that is not tried and for the slots at and above the run count, else the bits of
    the run's row mask (row_masks, by run) that no member's mask has"""
    out = np.full(n, -1, np.int32)
    for r, (m, t) in enumerate(zip(members, tried(mode, members, masks))):
        if t:
            union = 0
            for k in m:
                union |= int(masks[k])
            out[r] = int(row_masks[r]) & ~union
    return out


def compose_row(mode, m, chunks, masks, cchunks, cmask, emask=0):
    """the row of a tried run with members m (capture order): chunk j from the group decode (cchunks, after its retry) where cmask | emask
    has it, else from the lowest-index member that delivered it, else zeros; the mask is cmask | the members' masks | emask"""
    geo = geometry.for_mode(mode)
    row = np.zeros((geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    mask = (int(cmask) | int(emask)) & geo.FULL_MASK
    for j in range(geo.CHUNKS_PER_FRAME):
        if (mask >> j) & 1:
            row[j] = cchunks[j]
            continue
        for k in m:
            if (int(masks[k]) >> j) & 1:
                row[j] = chunks[k, j]
                break
    for k in m:
        mask |= int(masks[k])
    return row, mask


def run_rows(mode, n, members, chunks, masks, group_chunks, group_masks):
    """(rchunks, rmasks) of a once-call with the setting on: the group rows (by run, as a combined call with groups_in = runs_out reports
    them) for the tried runs, repeat_skip_model.run_fill's rows for all others"""
    rchunks, rmasks = RM.run_fill(mode, n, members, chunks, masks)
    for r, t in enumerate(tried(mode, members, masks)):
        if t:
            rchunks[r], rmasks[r] = group_chunks[r], group_masks[r]
    return rchunks, rmasks


# ------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def rendered(mode):
    """(captures by group_walk_cases.unique_index, payload (3, bytes)), read-only"""
    caps, payload = GW.rendered(mode)
    caps.setflags(write=False)
    return caps, payload


@functools.lru_cache(maxsize=None)
def bands(mode, frame=2):
    """the three-band triple of a frame: every member lacks another third of the frame's width"""
    caps, _ = rendered(mode)
    out = np.stack(GW.damaged_group(caps[3 * frame], 3, frame))
    out.setflags(write=False)
    return out


# the runs of sequence(), their representatives, and the runs the rescue tries
SEQUENCE_RUNS = [0, 0, 1, 1, 2, 2, 2, 3, 4, 4]
SEQUENCE_LIST1 = [0, 2, 5, 7, 8]
SEQUENCE_TRIED = [True, False, True, False, False]


@functools.lru_cache(maxsize=None)
def sequence(mode):
    """[disc pair of frame 0]           tried, the representative is member 0
    [frame 1 clean x 2]              the representative is complete: no pass 2, not tried
    [the three bands of frame 2]     tried, the representative is the MIDDLE member: a store slot between two pass-2 members
    [one disc capture of frame 0]    a run of one, incomplete, not tried
    [frame 1 wiped 8 %, frame 1]     pass 2 completes it: not tried"""
    caps, _ = rendered(mode)
    b = bands(mode)
    seq = [caps[1], caps[2], caps[3], caps[3], b[0], b[1], b[2], caps[1], RC.wipe8(mode, caps[3]), caps[3]]
    out = np.ascontiguousarray(np.stack(seq))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pairs(mode, count):
    """`count` disc pairs cycling the three frames: 2 * count captures, every run a tried pair"""
    caps, payload = rendered(mode)
    idx = []
    for i in range(count):
        idx += [3 * (i % GW.N_FRAMES) + 1, 3 * (i % GW.N_FRAMES) + 2]
    out = np.ascontiguousarray(caps[idx])
    out.setflags(write=False)
    return out, payload[[i % GW.N_FRAMES for i in range(count)]]
