"""Torn captures for the stitching tests (tests/test_stitch_model.py on the CPU, tests/test_gpu_stitch.py on the GPU): the same frames, the
same tear positions.

A tear is a pixel position along the axis (axis 0: a pixel row, axis 1: a pixel column). cut(X, Y, axis, p) shows X in front of p and Y from
p on. With frames A, B, C and tears p1 < p2:
  direction 0 (the sensor reads from line 0 up):   T1 = cut(A, B, p1),  T2 = cut(B, C, p2)  -- T1 shows B from p1 on, T2 shows B up to p2
  direction 1 (the sensor reads the other way):    T1 = cut(B, A, p2),  T2 = cut(C, B, p1)  -- T1 shows B up to p2, T2 shows B from p1 on
Either way the two captures agree on the lines between p1 and p2, and the pair (T1, T2) stitched in that direction is B.
"""
import numpy as np

from libcimbar_amd import framegen, geometry

MODES = [68, 67, 66, 4, 8]

# name: (line of p1, pixels into that line, line of p2, pixels into that line), the lines as fractions of the axis' L. A cell line is 8 pixels
# of cell and one of gap; 4 pixels in is the middle of the cells.
TEARS = {
    "top": (0.10, 0, 0.40, 0),
    "across": (0.35, 0, 0.65, 0),
    "bottom": (0.60, 0, 0.90, 0),
    "midcell": (0.45, 4, 0.58, 4),
}


def tear_pixels(mode, axis, name):
    geo = geometry.for_mode(mode)
    L = geo.DIM_Y if axis == 0 else geo.DIM_X
    f1, sub1, f2, sub2 = TEARS[name]
    return geo.OFFSET + int(f1 * L) * geo.PITCH + sub1, geo.OFFSET + int(f2 * L) * geo.PITCH + sub2


def cut(X, Y, axis, p):
    out = X.copy()
    if axis == 0:
        out[p:] = Y[p:]
    else:
        out[:, p:] = Y[:, p:]
    return out


def torn_pair(A, B, C, axis, p1, p2, direction):
    if direction == 0:
        return cut(A, B, axis, p1), cut(B, C, axis, p2)
    return cut(B, A, axis, p2), cut(C, B, axis, p1)


_rendered = {}


def rendered(mode, n=3):
    """(frames (n, h, w, 3) uint8, payload (n, frame bytes)) of `mode`, rendered once per process"""
    if (mode, n) not in _rendered:
        payload = framegen.synth_payload(n, seed=4100 + mode, mode=mode)
        frames = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
        _rendered[(mode, n)] = (frames, payload.numpy().reshape(n, -1))
    return _rendered[(mode, n)]


# the capture path: mode 68, 1080p. Each entry: (axis, direction, tear name); the frame is torn first and photographed after
# (tests/frames.camera_frame), so the tear is a straight line of the screen, slanted in the capture like everything else.
CAPTURE_CASES = [(0, 0, "across"), (1, 1, "midcell")]
CAPTURE_FORMATS = (3, 12)


def capture_pairs(axis, direction, name, fmt):
    """[A, T1, T2, C] photographed at 1080p in `fmt` -> (captures (4, bytes) uint8, (w, h))"""
    from tests import capture_formats as CF
    from tests import frames as F
    frames, _ = rendered(68)
    p1, p2 = tear_pixels(68, axis, name)
    t1, t2 = torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction)
    cams = [F.camera_frame(f, background=30) for f in (frames[0], t1, t2, frames[2])]
    h, w = cams[0].shape[:2]
    return np.stack([CF.rgb_to_format(c, fmt) for c in cams]), (w, h)


def noise_lines(frame, mode, axis, lines, seed):
    """the cells of the given grid lines overwritten with noise (the gaps between the lines stay)"""
    geo = geometry.for_mode(mode)
    out = frame.copy()
    g = np.random.default_rng(seed)
    for l in lines:
        p = geo.OFFSET + l * geo.PITCH
        if axis == 0:
            out[p:p + 8] = g.integers(0, 256, out[p:p + 8].shape, dtype=np.uint8)
        else:
            out[:, p:p + 8] = g.integers(0, 256, out[:, p:p + 8].shape, dtype=np.uint8)
    return out


# a band of 12 lines, [BAND_LO, BAND_LO + 12) in every mode and on both axes: with three of its lines damaged 4 * 9 >= 3 * 12 still holds,
# with four 4 * 8 < 3 * 12
BAND_LO = 30
DAMAGED_3, DAMAGED_4 = (32, 35, 38), (32, 35, 38, 40)


def damaged_band_batch(mode, axis):
    """[T1, T2 with three band lines noised, A, T1, T2 with four] -- pair 0 is a candidate, pair 3 is not"""
    geo = geometry.for_mode(mode)
    frames, _ = rendered(mode)
    p1, p2 = geo.OFFSET + BAND_LO * geo.PITCH, geo.OFFSET + (BAND_LO + 12) * geo.PITCH
    t1, t2 = torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, 0)
    return np.stack([t1, noise_lines(t2, mode, axis, DAMAGED_3, 7), frames[0], t1, noise_lines(t2, mode, axis, DAMAGED_4, 8)])
