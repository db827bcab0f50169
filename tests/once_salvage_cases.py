"""Inputs of the tear-salvage tests (seeded, built once per mode and shared): tests/repeat_skip_cases.clean's frames A, B, C cut with
tests/stitch_cases.cut at tests/stitch_cases.tear_pixels' positions and damaged with tests/repeat_skip_cases.wipe8 (or the same square at
another centre, wipe_at). tests/test_once_salvage_model.py asserts on the CPU the margins, the records and the plans the GPU tests rely on.

Every case is (captures, settings): min_agree_permille and max_run of the once-call, line_permille of tear skipping (axis 0 throughout)."""
import functools

import numpy as np

from libcimbar_amd import geometry
from tests import frames as F
from tests import once_rescue_model as OM
from tests import repeat_skip_cases as RC
from tests import stitch_cases as SC

MODES = RC.MODES
# The lines through the wipe agree with the undamaged frame at 758 permille or more: thin against tear skipping's default 750, so 650.
# Consecutive captures of S1 agree at 1000 inside a run and at 887 or less across runs: 950 splits them.
MIN_AGREE, LINE = 950, 650


def _stack(seq):
    out = np.ascontiguousarray(np.stack(seq))
    out.setflags(write=False)
    return out


def wipe_at(mode, frame, fy, fx):
    """wipe8's black square (8 % of the grid's cells) centred at the fractions (fy, fx) of the grid"""
    geo = geometry.for_mode(mode)
    side = int(round((0.08 * geo.DIM_X * geo.DIM_Y) ** 0.5 * geo.PITCH))
    cy, cx = geo.OFFSET + int(fy * geo.DIM_Y * geo.PITCH), geo.OFFSET + int(fx * geo.DIM_X * geo.PITCH)
    return F.blank_region(frame, cy - side // 2, cy - side // 2 + side, cx - side // 2, cx - side // 2 + side)


# ------------------------------------------------------------------------------------------------ S1
@functools.lru_cache(maxsize=None)
def s1(mode):
    """wipe8(A) | cut(A, B, bottom p2) | B, B + noise 40 | cut(B, C, top p1) | wipe8(C) | B"""
    _, f = RC.clean(mode)
    A, B, C = f[0], f[1], f[2]
    return _stack([
        RC.wipe8(mode, A),                                                # 0     run 0: incomplete, a run of one
        SC.cut(A, B, 0, SC.tear_pixels(mode, 0, "bottom")[1]),            # 1     torn: A on nine lines of ten, its P side serves run 0
        B, F.add_noise(B, 40, 2),                                         # 2 3   run 2: complete
        SC.cut(B, C, 0, SC.tear_pixels(mode, 0, "top")[0]),               # 4     torn: C on nine lines of ten, its N side serves run 4
        RC.wipe8(mode, C),                                                # 5     run 4: incomplete, a run of one
        B,                                                                # 6     run 5
    ])


S1_RUNS = [0, 1, 2, 2, 3, 4, 5]
S1_AGREE = {68: [862, 332, 1000, 320, 872, 249], 67: [873, 324, 1000, 320, 877, 256], 66: [871, 328, 1000, 313, 887, 261]}
S1_RECORDS = {68: ((0, 100, 100, 12), (0, 11, 11, 101)), 67: ((0, 70, 70, 8), (0, 7, 7, 71)), 66: ((0, 62, 62, 7), (0, 6, 6, 63))}   # captures 1 and 4
S1_LIST1 = [0, 2, 5, 6]
S1_LIST2 = [1, 4]
S1_TRIED = [True, False, False, False, True, False]
S1_PAYLOAD = {0: 0, 4: 2}                                                 # tried run: the frame it shows


# ------------------------------------------------------------------------------------------------ three further cases
@functools.lru_cache(maxsize=None)
def both_sides(mode):
    """wipe(A, upper half) | cut(A, B, midcell p1) | wipe(B, lower half): one candidate between two incomplete runs of one, serving both.
    The tear runs at 45 % of the lines; the squares cover 8 % .. 36 % and 61 % .. 89 % of them, each inside the side that serves it."""
    _, f = RC.clean(mode)
    A, B = f[0], f[1]
    return _stack([wipe_at(mode, A, 0.22, 0.5), SC.cut(A, B, 0, SC.tear_pixels(mode, 0, "midcell")[0]), wipe_at(mode, B, 0.75, 0.5)])


BOTH_RUNS = [0, 1, 2]
BOTH_TRIED = [True, False, True]

# the disc pair of tests/once_rescue_model.py agrees at 823 permille or more, a capture torn at 45 % with either frame at about 700 or less
PAIR_MIN_AGREE, PAIR_LINE = 800, 550


@functools.lru_cache(maxsize=None)
def pair_and_partial(mode):
    """[disc pair of frame 0] | cut(frame 0, frame 1, midcell p1) | frame 1 x 2: a run the rescue tries anyway, with a torn capture behind
    it. The discs sit on the middle lines, so the lines of the candidate's P side agree with the damaged capture in front of it at about 620
    permille where they cross a disc: line_permille 550."""
    caps, _ = OM.rendered(mode)
    return _stack([caps[1], caps[2], SC.cut(caps[0], caps[3], 0, SC.tear_pixels(mode, 0, "midcell")[0]), caps[3], F.add_noise(caps[3], 40, 3)])


PAIR_RUNS = [0, 0, 1, 2, 2]
PAIR_TRIED = [True, False, False]


@functools.lru_cache(maxsize=None)
def full_run(mode):
    """wipe8(A) x 8 (noise apart) | cut(A, B, bottom p2) | B, with max_run 8: the run is tried, and GMAX is full, so it gets no partial"""
    _, f = RC.clean(mode)
    A, B = f[0], f[1]
    W = RC.wipe8(mode, A)
    return _stack([W] + [RC.wipe8(mode, F.add_noise(A, 40, 10 + j)) for j in range(7)] + [SC.cut(A, B, 0, SC.tear_pixels(mode, 0, "bottom")[1]), B])


FULL_RUNS = [0] * 8 + [1, 2]
FULL_TRIED = [True, False, False]


# ------------------------------------------------------------------------------------------------ the capture path
def capture_case(fmt):
    """[wipe8(A), cut(A, B, "bottom"), B, B] of mode 68 photographed at 1080p in `fmt`, as once_tear_cases.capture_case photographs its
    captures -> (captures (4, bytes) uint8, (w, h))"""
    from tests import capture_formats as CF
    frames, _ = SC.rendered(68)
    A, B = frames[0], frames[1]
    torn = SC.cut(A, B, 0, SC.tear_pixels(68, 0, "bottom")[0])
    cams = [F.camera_frame(f, background=30) for f in (RC.wipe8(68, A), torn, B, B)]
    h, w = cams[0].shape[:2]
    return np.stack([CF.rgb_to_format(c, fmt) for c in cams]), (w, h)
