"""Inputs of the tear-skipping tests (seeded, built once per mode and shared): tests/repeat_skip_cases.clean's frames A .. E, cut with
tests/stitch_cases.cut at tests/stitch_cases.tear_pixels' positions. tests/test_once_tear_model.py asserts on the CPU the per-line margins
and the plans the GPU tests rely on.

cut(X, Y, axis, p) shows X in front of pixel p and Y from it on. A camera that films A A A | B B catches the switch as cut(A, B): the earlier
frame on the low lines (orientation 0); a sensor read the other way round shows cut(B, A) (orientation 1)."""
import functools

import numpy as np

from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import stitch_cases as SC

MODES = RC.MODES


def _pos(mode, axis, name):
    return SC.tear_pixels(mode, axis, name)[0]


def _stack(seq):
    out = np.ascontiguousarray(np.stack(seq))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sequence1(mode):
    """[A x 3] T(A|B) [B x 2] T(C|B, the other way round) [C] T(C|D) [D x 3, the representative wiped] [E] [A x 2]"""
    _, f = RC.clean(mode)
    A, B, C, D, E = f[0], f[1], f[2], f[3], f[4]
    return _stack([
        A, F.add_noise(A, 40, 1), F.shift(A, 2, 1),                       # 0 1 2    run 0
        SC.cut(A, B, 0, _pos(mode, 0, "midcell")),                        # 3        torn: orientation 0, the tear in mid-cell
        B, F.add_noise(B, 40, 2),                                         # 4 5      run 2
        SC.cut(C, B, 0, _pos(mode, 0, "across")),                         # 6        torn: orientation 1
        C,                                                                # 7        run 4
        SC.cut(C, D, 0, _pos(mode, 0, "bottom")),                         # 8        a candidate the guard sends to pass 2
        F.add_noise(D, 40, 3), RC.wipe8(mode, D), D,                      # 9 10 11  run 6, its representative (10) incomplete
        E,                                                                # 12       a distinct frame between two runs: no candidate
        A, RC.blur(A, 1.5),                                               # 13 14    run 8
    ])


SEQ1_RUNS = [0, 0, 0, 1, 2, 2, 3, 4, 5, 6, 6, 6, 7, 8, 8]
SEQ1_CANDIDATES = {3: (0, "midcell"), 6: (1, "across"), 8: (0, "bottom")}   # capture: (orientation, tear)
SEQ1_LIST1 = [1, 4, 7, 10, 12, 13]
SEQ1_TORN = [3, 6]
SEQ1_LIST2 = [8, 9, 11]
SEQ1_PAYLOAD = [0, None, 1, None, 2, None, 3, 4, 0]                       # the frame (A = 0 ..) every run shows, None for a torn capture's run


@functools.lru_cache(maxsize=None)
def sequence2(mode):
    """T(A|B) first, [B x 2], T(B|C) along the other axis, [C x 5: max_run 4 leaves the fifth alone], T(C|D, "top": joins D's run) D,
    T(D|E) last"""
    _, f = RC.clean(mode)
    A, B, C, D, E = f[0], f[1], f[2], f[3], f[4]
    vc = RC.variants(C, 4)
    return _stack([
        SC.cut(A, B, 0, _pos(mode, 0, "midcell")),                        # 0        torn, but the first capture: not eligible
        B, F.add_noise(B, 40, 5),                                         # 1 2      run 1
        SC.cut(B, C, 1, _pos(mode, 1, "across")),                         # 3        torn along axis 1
        C, vc["noise40"], vc["cast"], vc["shift21"],                      # 4 .. 7   run 3
        vc["blur15"],                                                     # 8        the fifth repeat: a run of one by max_run, no candidate
        SC.cut(C, D, 0, _pos(mode, 0, "top")),                            # 9        shows D on nine lines of ten: joins D's run
        D,                                                                # 10       run 5 = [9, 10]
        SC.cut(D, E, 0, _pos(mode, 0, "midcell")),                        # 11       torn, but the last capture: not eligible
    ])


SEQ2_RUNS = [0, 1, 1, 2, 3, 3, 3, 3, 4, 5, 5, 6]
SEQ2_CANDIDATES_AXIS = {0: [], 1: [3], 2: [3]}                            # the setting's axis: the candidates


def capture_case(fmt):
    """[A, A, cut(A, B, "across"), B, B] of mode 68 photographed at 1080p in `fmt`, as stitch_cases.capture_pairs photographs its captures
    -> (captures (5, bytes) uint8, (w, h))"""
    from tests import capture_formats as CF
    frames, _ = SC.rendered(68)
    A, B = frames[0], frames[1]
    torn = SC.cut(A, B, 0, _pos(68, 0, "across"))
    cams = [F.camera_frame(f, background=30) for f in (A, A, torn, B, B)]
    h, w = cams[0].shape[:2]
    return np.stack([CF.rgb_to_format(c, fmt) for c in cams]), (w, h)
