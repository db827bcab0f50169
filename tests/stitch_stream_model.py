"""A plain-Python restatement of torn-capture stitching across calls (include/cimbar_hip.h, cimbar_hip_decode_batch_stitched_stream;
csrc/stitch.hip.inc "the stream calls"). The rule of a pair is tests/stitch_model.stitch_pair and is not restated here: this file only adds
what the calls carry.

StitchStreamModel(mode) keeps between calls what the device keeps: the last capture's symbols, colours and whether it is usable.

    call(symbols, colors, axis=0, min_agree_permille=0, min_band=0, usable=None) -> (tears (n, 4), cnt (n, L), cells (2n, NCELLS))
        row 0 is (the carried capture, capture 0), row r is (capture r - 1, capture r); row r, direction d is cells[2r + d].
        Without a usable carried capture (after the constructor or reset(), or the carried capture was unusable) row 0 is the
        non-candidate {-1, -1, -1, 0} with zero counts and zero cells.
        raises ValueError where the library returns CIMBAR_HIP_EINVAL (n == 0, axis outside {0, 1}, min_band above L); the carry stays.
    reset()   forget the carry
    carry     None, or (symbols, colours, usable) of the last capture of the last call
"""
import numpy as np

from libcimbar_amd import geometry
from tests import stitch_model as SM


class StitchStreamModel:
    def __init__(self, mode):
        self.mode = mode
        self.carry = None

    def reset(self):
        self.carry = None

    def call(self, symbols, colors, axis=0, min_agree_permille=0, min_band=0, usable=None):
        n = len(symbols)
        if n <= 0:
            raise ValueError("n <= 0")
        SM.resolve(self.mode, axis, min_agree_permille, min_band)
        usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
        geo = geometry.for_mode(self.mode)
        _, L, _ = SM.lines_of(self.mode, axis)
        tears, cnt, cells = np.zeros((n, 4), np.int32), np.zeros((n, L), np.uint16), np.zeros((2 * n, geo.NCELLS), np.uint8)
        prev = self.carry
        for r in range(n):
            if prev is None or (r == 0 and not prev[2]):
                tears[r] = (-1, -1, -1, 0)
            else:
                tears[r], cnt[r], cells[2 * r:2 * r + 2] = SM.stitch_pair(self.mode, prev[0], prev[1], symbols[r], colors[r], axis, min_agree_permille,
                                                                          min_band, bool(prev[2] and usable[r]))
            prev = (np.array(symbols[r], np.uint8), np.array(colors[r], np.uint8), bool(usable[r]))
        self.carry = prev
        return tears, cnt, cells


def run(mode, calls, axis=0, min_agree_permille=0, min_band=0):
    """calls = [(symbols, colors, usable or None), ...] -> the per-call results of one stream"""
    model = StitchStreamModel(mode)
    return [model.call(s, c, axis, min_agree_permille, min_band, u) for s, c, u in calls]
