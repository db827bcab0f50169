"""Inputs of the once-stream tests beyond tests/repeat_skip_cases.py (seeded, built once and shared): the signatures of RC.sequence, and the
long input that takes the walk past one 64-lane step. tests/test_repeat_stream_model.py asserts on the CPU what the GPU tests rely on."""
import functools

import numpy as np

from libcimbar_amd import geometry
from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

LONG_MODE, LONG_N = 68, 130
# run lengths 1..4 in a fixed irregular order, repeated until 130 captures are placed. Run i shows clean frame i % 5 of RC.clean, so neighbours
# differ; run 0 shows A and continues a carried [A]: with its 2 members that run has 3, below max_run 4.
LONG_PATTERN = (2, 3, 1, 4, 2, 4, 3, 1)
# the representatives that carry the 8 % wipe, by run. Run 21 is captures 52..55 (representative 53, all in the first 64-lane step); run 25
# is captures 62..64 (representative 63 in lane 63, member 64 in the second step); run 29 is captures 72..75 (all in the second step)
LONG_WIPED_RUNS = (21, 25, 29)


def wipe5(mode, frame):
    """RC.wipe8 with a square of 5 % of the cells: in mode 68 frame A then delivers some of its chunks and not others (a partial P)"""
    geo = geometry.for_mode(mode)
    side = int(round((0.05 * geo.DIM_X * geo.DIM_Y) ** 0.5 * geo.PITCH))
    cy, cx = geo.OFFSET + geo.DIM_Y * geo.PITCH // 2, geo.OFFSET + geo.DIM_X * geo.PITCH // 2
    return F.blank_region(frame, cy - side // 2, cy - side // 2 + side, cx - side // 2, cx - side // 2 + side)


@functools.lru_cache(maxsize=None)
def sequence_sigs(mode):
    s = RM.signatures(mode, RC.sequence(mode))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def long_layout():
    """(lengths, pool index of every capture): pool entry 4 f + v is variant v of clean frame f (0 clean, 1..3 noise 40 with seed 10 f + v),
    entry 20 + f is clean frame f with the 8 % wipe"""
    lengths, total, i = [], 0, 0
    while total < LONG_N:
        ln = min(LONG_PATTERN[i % len(LONG_PATTERN)], LONG_N - total)
        lengths.append(ln)
        total += ln
        i += 1
    index = []
    for r, ln in enumerate(lengths):
        f = r % 5
        rep = (ln - 1) // 2
        for m in range(ln):
            index.append(20 + f if (r in LONG_WIPED_RUNS and m == rep) else 4 * f + m)
    return tuple(lengths), np.array(index, np.int32)


@functools.lru_cache(maxsize=None)
def long_pool():
    _, f = RC.clean(LONG_MODE)
    pool = [f[k] if v == 0 else F.add_noise(f[k], 40, 10 * k + v) for k in range(5) for v in range(4)]
    pool += [RC.wipe8(LONG_MODE, f[k]) for k in range(5)]
    pool = np.ascontiguousarray(np.stack(pool))
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def long_pool_sigs():
    s = RM.signatures(LONG_MODE, long_pool())
    s.setflags(write=False)
    return s


def long_sigs():
    return long_pool_sigs()[long_layout()[1]]


def long_frames():
    """(130, H, W, 3): not cached -- 400 MB"""
    return np.ascontiguousarray(long_pool()[long_layout()[1]])


def long_runs():
    """the run of every capture, by construction"""
    lengths, _ = long_layout()
    return np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
