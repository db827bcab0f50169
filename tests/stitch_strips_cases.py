"""Slanted and blended tears for the strip tests (tests/test_stitch_strips_model.py on the CPU, tests/test_gpu_stitch_strips.py on the GPU):
the frames of tests/stitch_cases.py, torn along a line that rises across the frame.

cut_slanted(X, Y, axis, p, rise, blend): the tear at across-pixel u (axis 0: the pixel column, axis 1: the pixel row) of A_px lies at
t(u) = p + rise * u / (A_px - 1) along the axis, p and rise in pixels. Y's weight at position pos along the axis is
clip((pos - t) / blend + 0.5, 0, 1) -- a transition `blend` pixels wide, centred on the tear -- and the step pos >= t for blend = 0; the
output is rint of the mix. rise = 0, blend = 0 is stitch_cases.cut.

SLANTS: (rise in grid lines, gap between the two tears in grid lines, blend in pixels). With p1 = OFFSET + (L // 3) * PITCH + 4 and
p2 = p1 + gap * PITCH the two tears lie fewer lines apart than 3/4 of the rise, so no whole line reaches 750 per mille, while every column
keeps `gap` shared lines. Pairs are built as stitch_cases.torn_pair builds them, in both directions.
"""
import numpy as np

from libcimbar_amd import geometry
from tests import stitch_cases as SC

SLANTS = [(10, 6, 0), (10, 6, 6), (16, 7, 6)]
STRIPS = (4, 8)


def cut_slanted(X, Y, axis, p, rise, blend):
    h, w = X.shape[:2]
    A_px = w if axis == 0 else h
    t = p + rise * np.arange(A_px, dtype=np.float64) / (A_px - 1)
    pos = np.arange(h if axis == 0 else w, dtype=np.float64)
    d = pos[:, None] - t[None, :] if axis == 0 else pos[None, :] - t[:, None]          # (h, w): position along the axis minus the tear there
    wy = (d >= 0).astype(np.float64) if blend == 0 else np.clip(d / blend + 0.5, 0.0, 1.0)
    mix = X.astype(np.float64) * (1.0 - wy[..., None]) + Y.astype(np.float64) * wy[..., None]
    return np.rint(mix).astype(np.uint8)


def slant_pixels(mode, axis, rise, gap):
    """(p1, p2, rise in pixels) of a parameter set given in grid lines"""
    geo = geometry.for_mode(mode)
    L = geo.DIM_Y if axis == 0 else geo.DIM_X
    p1 = geo.OFFSET + (L // 3) * geo.PITCH + 4
    return p1, p1 + gap * geo.PITCH, rise * geo.PITCH


def slanted_pair(A, B, C, axis, p1, p2, direction, rise, blend):
    if direction == 0:
        return cut_slanted(A, B, axis, p1, rise, blend), cut_slanted(B, C, axis, p2, rise, blend)
    return cut_slanted(B, A, axis, p2, rise, blend), cut_slanted(C, B, axis, p1, rise, blend)


_batches = {}


def slanted_batch(mode, axis, direction, slant):
    """[A, T1, T2, C] of `mode` with the pair torn by the parameter set `slant`, built once per process"""
    key = (mode, axis, direction, slant)
    if key not in _batches:
        frames, _ = SC.rendered(mode)
        rise, gap, blend = slant
        p1, p2, rise_px = slant_pixels(mode, axis, rise, gap)
        t1, t2 = slanted_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction, rise_px, blend)
        _batches[key] = np.stack([frames[0], t1, t2, frames[2]])
    return _batches[key]


def strip_pixels(mode, axis, S, j):
    """[lo, hi): the pixels across the lines that the cells of strip j of S cover"""
    geo = geometry.for_mode(mode)
    A = geo.DIM_X if axis == 0 else geo.DIM_Y
    across = [q for q in range(A) if q * S // A == j]
    return geo.OFFSET + across[0] * geo.PITCH, geo.OFFSET + across[-1] * geo.PITCH + 8


def noise_lines_in_strips(frame, mode, axis, lines, S, strips, seed):
    """stitch_cases.noise_lines restricted to the strips `strips` of S: the other strips keep the lines as they are"""
    noisy = SC.noise_lines(frame, mode, axis, lines, seed)
    out = frame.copy()
    for j in strips:
        lo, hi = strip_pixels(mode, axis, S, j)
        if axis == 0:
            out[:, lo:hi] = noisy[:, lo:hi]
        else:
            out[lo:hi] = noisy[lo:hi]
    return out


# a straight band of 12 lines [BAND_LO, BAND_LO + 12) as stitch_cases.damaged_band_batch has it; strips are of 4. Four damaged lines fail the
# 3/4 rule (4 * 8 < 3 * 12), so a strip that has them is not located.
def damaged_strips_batch(mode, axis):
    """[T1, T2 with strip 1 damaged, A, T1, T2 with strips 0, 1, 3 damaged] at S = 4 -- pair 0: three strips located, strip 1 takes strip 0's
    split; pair 3: one strip located of four, no candidate"""
    geo = geometry.for_mode(mode)
    frames, _ = SC.rendered(mode)
    p1, p2 = geo.OFFSET + SC.BAND_LO * geo.PITCH, geo.OFFSET + (SC.BAND_LO + 12) * geo.PITCH
    t1, t2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, 0)
    return np.stack([t1, noise_lines_in_strips(t2, mode, axis, SC.DAMAGED_4, 4, (1,), 7), frames[0], t1,
                     noise_lines_in_strips(t2, mode, axis, SC.DAMAGED_4, 4, (0, 1, 3), 8)])


# the capture path: mode 68, 1080p, (axis, direction) as stitch_cases.CAPTURE_CASES; the frame is torn first and photographed after
CAPTURE_SLANT = (10, 6, 6)
# the gap the capture test uses: the largest value, from CAPTURE_SLANT's 6 downwards, at which the whole-line rule finds no candidate on the
# photographed pair (tests/test_stitch_strips_model.py asserts that it does not)
CAPTURE_GAP = 6
CAPTURE_CASES = [(0, 0), (1, 1)]


def capture_pairs_slanted(axis, direction, fmt, gap=CAPTURE_GAP):
    """[A, T1, T2, C] photographed at 1080p in `fmt` -> (captures (4, bytes) uint8, (w, h))"""
    from tests import capture_formats as CF
    from tests import frames as F
    frames, _ = SC.rendered(68)
    rise, _, blend = CAPTURE_SLANT
    p1, p2, rise_px = slant_pixels(68, axis, rise, gap)
    t1, t2 = slanted_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction, rise_px, blend)
    cams = [F.camera_frame(f, background=30) for f in (frames[0], t1, t2, frames[2])]
    h, w = cams[0].shape[:2]
    return np.stack([CF.rgb_to_format(c, fmt) for c in cams]), (w, h)
