"""Inputs the colour vote's tests share (tests/test_group_colour_model.py on the CPU, tests/test_gpu_group_colour.py on the GPU).

- `pair_set`: per mode, frames captured twice with disjoint discs, capture 0 damaged on the left and capture 1 on the right. The kinds: the
  white, black and noise discs of the colour erasure tests, and "washed" discs -- every pixel's channels become its largest one, so the
  symbols survive and only the colour is lost. A washed cell is where counting heads has nothing to go by in a group of two: both members
  show the symbol equally well, and the tie goes to the lower member, damaged or not.
- `crafted_pair`: two captures of one frame in which chosen cyan cells of ONE colour block are washed in capture 0 (every term of the
  classifier equal: class 0, margin 0) and red in capture 1 (r > g = b: yellow and magenta tie at the top, class 2 or 3 with a margin of 0 or
  next to it under the matrix in force). A bright cell cannot have a small margin that is not 0 -- the classifier saturates every channel
  above 197 -- so two different near-ties are how a small GROUP margin comes about. Neither capture decodes the block, the vote's colour is
  wrong in every touched cell with a group margin far below the suggested threshold, and the group colour retry sees exactly those bytes.
  One cell per stream byte, so `count` cells are `count` wrong, flagged bytes. Further cells damaged in one capture only keep each capture's own
  colour retry from recovering the block alone.
"""
import numpy as np

from libcimbar_amd import framegen, geometry
from tests import colour_erasure_cases as K

MODES = K.MODES
MARGIN = K.MARGIN
PAIR_KINDS = ("washed", "white", "washed", "noise", "washed", "black")
PAIR_SIZES = (0.09, 0.07, 0.12, 0.06, 0.15, 0.08)
PAIR_SEED = 61


def disc(shape, cx, cy, r):
    h, w = shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * w) ** 2


def damage(frame, where, kind, seed):
    """in place"""
    if kind == "white":
        frame[where] = 255
    elif kind == "black":
        frame[where] = 0
    elif kind == "noise":
        frame[where] = np.random.default_rng(seed).integers(0, 256, (int(where.sum()), 3), dtype=np.uint8)
    else:
        frame[where] = frame[where].max(axis=1, keepdims=True)
    return frame


def pair_set(mode, n=len(PAIR_KINDS), seed=PAIR_SEED):
    """-> (captures (2n, h, w, 3), payload (n, FRAME_BYTES), groups (2n,)): group g = captures 2g (disc on the left) and 2g + 1 (on the right)"""
    fr, payload = K.frames(mode, n, seed + mode)
    g = np.random.default_rng(seed)
    caps = []
    for k in range(n):
        kind, size = PAIR_KINDS[k % len(PAIR_KINDS)], PAIR_SIZES[k % len(PAIR_SIZES)]
        for c, cx in enumerate((0.32, 0.68)):
            cy = 0.4 + 0.2 * g.random()
            caps.append(damage(fr[k].copy(), disc(fr[k].shape, cx, cy, size), kind, seed * 100 + 2 * k + c))
    return np.stack(caps), payload, np.repeat(np.arange(n), 2).astype(np.int32)


def true_colours(mode, payload):
    """(n, NCELLS) the colour every cell was rendered with"""
    import torch
    pay = torch.from_numpy(np.ascontiguousarray(np.asarray(payload, np.uint8).reshape(len(payload), -1)))
    return (framegen.FrameSynth("cpu", mode).cell_tiles(pay).numpy() >> 4).astype(np.uint8)


def crafted_pair(mode, frame, colours, count, block=0, extra=0):
    """-> (capture 0, capture 1, the byte positions touched in both captures in colour block `block`). extra: as many further cyan cells are
    washed in capture 0 alone and as many made red in capture 1 alone: each capture's own colour retry then sees count + extra flagged bytes,
    the group only the `count` both share -- where one member is clean its margin carries the vote, far above the threshold."""
    geo = geometry.for_mode(mode)
    il = geo.interleave_indices()
    xy = geo.cell_positions()
    a, b = frame.copy(), frame.copy()
    done = []
    for k in range(8, geo.RS_BLOCK):          # (the block's first six bytes hold the header-predicted cells the colour-correction matrix is derived from)
        if len(done) == count + 2 * extra:
            break
        cell = next((int(c) for c in il[(geo.RS_BLOCK * block + k) * 4:(geo.RS_BLOCK * block + k) * 4 + 4] if colours[c] == 1), None)
        if cell is None:
            continue
        x, y = (int(v) for v in xy[cell])
        v = frame[y:y + 8, x:x + 8].max(axis=2, keepdims=True)
        if len(done) < count or (len(done) - count) % 2 == 0:
            a[y:y + 8, x:x + 8] = v
        if len(done) < count or (len(done) - count) % 2 == 1:
            b[y:y + 8, x:x + 8] = v * np.array([1, 0, 0], np.uint8)
        done.append(k)
    assert len(done) == count + 2 * extra, "not enough cyan cells in the block"
    return a, b, done[:count]
