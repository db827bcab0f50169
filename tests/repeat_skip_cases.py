"""Inputs of the repeat-capture skipping tests (seeded, built once per mode and shared): clean frames and the variants a camera makes of
them. tests/test_repeat_skip_model.py asserts on the CPU the signature margins the GPU tests rely on."""
import functools

import numpy as np

from libcimbar_amd import framegen, geometry
from tests import frames as F

MODES = (68, 67, 66)


@functools.lru_cache(maxsize=None)
def clean(mode, n=5, seed=900):
    """(payload (n, FRAME_BYTES), frames (n, H, W, 3)): frames A, B, C, D, E of `mode`"""
    synth = framegen.FrameSynth("cpu", mode)
    payload, frames = F.clean_frames(synth, n, seed=seed + mode)
    frames.setflags(write=False)
    return payload, frames


def blur(frame, sigma):
    from PIL import Image, ImageFilter
    return np.array(Image.fromarray(frame).filter(ImageFilter.GaussianBlur(sigma)))


def cast(frame, gains=(1.0, 0.8, 0.6), lift=20):
    return np.clip(frame.astype(np.float32) * np.array(gains, np.float32) + lift, 0, 255).astype(np.uint8)


def torn(a, b):
    """the top half of a over the bottom half of b"""
    out = b.copy()
    out[:a.shape[0] // 2] = a[:a.shape[0] // 2]
    return out


def wipe8(mode, frame):
    """a black square over the centre of the grid that covers 8 % of its cells"""
    geo = geometry.for_mode(mode)
    side = int(round((0.08 * geo.DIM_X * geo.DIM_Y) ** 0.5 * geo.PITCH))
    cy, cx = geo.OFFSET + geo.DIM_Y * geo.PITCH // 2, geo.OFFSET + geo.DIM_X * geo.PITCH // 2
    return F.blank_region(frame, cy - side // 2, cy - side // 2 + side, cx - side // 2, cx - side // 2 + side)


def variants(frame, seed):
    """the near-identical captures of one displayed frame the tests use, by name"""
    return {"noise40": F.add_noise(frame, 40, seed), "shift21": F.shift(frame, 2, 1), "blur15": blur(frame, 1.5), "cast": cast(frame)}


@functools.lru_cache(maxsize=None)
def sequence(mode):
    """[A, A + noise, A + shift], [B], [torn A | C], [C, C + blur], [D x 5 variants]: the runs by construction (max_run 4 splits the last)"""
    _, f = clean(mode)
    A, B, C, D = f[0], f[1], f[2], f[3]
    vd = variants(D, 4)
    seq = [A, F.add_noise(A, 40, 1), F.shift(A, 2, 1), B, torn(A, C), C, blur(C, 1.5), D, vd["noise40"], vd["cast"], vd["shift21"], vd["blur15"]]
    out = np.ascontiguousarray(np.stack(seq))
    out.setflags(write=False)
    return out


SEQUENCE_RUNS = [0, 0, 0, 1, 2, 3, 3, 4, 4, 4, 4, 5]
SEQUENCE_LIST1 = [1, 3, 4, 5, 8, 11]


@functools.lru_cache(maxsize=None)
def fallback_run(mode):
    """a run of three whose representative (the second) carries the 8 % wipe: [A + noise, A wiped, A]"""
    _, f = clean(mode)
    out = np.ascontiguousarray(np.stack([F.add_noise(f[0], 40, 7), wipe8(mode, f[0]), f[0]]))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def signature_frames(mode):
    """about ten frames for the signature taps: clean, noise 40 / 120, shifts, rescale(+6), the cast, all black, all white (every cell ties:
    the strict comparisons decide), one bright cell on black"""
    geo = geometry.for_mode(mode)
    _, f = clean(mode)
    A = f[0]
    black = np.zeros(geo.FRAME_SHAPE, np.uint8)
    white = np.full(geo.FRAME_SHAPE, 255, np.uint8)
    one = black.copy()
    x, y = geo.cell_positions()[geo.NCELLS // 3]
    one[y:y + 8, x:x + 8] = (255, 40, 200)
    gray = np.full(geo.FRAME_SHAPE, 10, np.uint8)                       # ... and the same cell on dim gray: the only cell above the frame's shares
    gray[y:y + 8, x:x + 8] = (255, 40, 200)
    out = [A, F.add_noise(A, 40, 1), F.add_noise(A, 120, 2), F.shift(A, 2, 1), F.shift(A, -3, 4), F.rescale(A, 6), cast(A), black, white, one, gray]
    out = np.ascontiguousarray(np.stack(out))
    out.setflags(write=False)
    return out
