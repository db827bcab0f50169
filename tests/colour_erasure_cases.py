"""Inputs the colour erasure tests share (tests/test_colour_erasure_model.py on the CPU, tests/test_gpu_colour_erasure_decode.py on the GPU):
frames rendered from known payloads, the glare set and the overload patches.

The glare set: per frame a saturated white disc, a black disc or a random-noise disc, at four radii (fractions of the frame's width). A
colour-stream byte comes from four cells, so the 0.13 discs the symbol retry's tests use flag more bytes per colour block than parity - 8
allows and mostly stay lost; the smaller discs are the ones the colour retry can win back. The set was chosen with the model on the CPU
(test_colour_erasure_model.py::test_glare_model_recovers_more asserts what it has to deliver before anything runs on a GPU).
"""
import numpy as np

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen

MODES = [68, 67, 66]
MARGIN = D.COLOUR_MARGIN_SUGGESTED          # the one threshold every test uses (DESIGN_WIDENING.md "Colour erasure decoding")
GLARE_SIZES = (0.05, 0.07, 0.09, 0.13)
GLARE_N, GLARE_SEED, GLARE_DISC_SEED = 12, 21, 7


def frames(mode, n, seed):
    payload = framegen.synth_payload(n, seed=seed, mode=mode)
    fr = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
    return fr, payload.numpy().reshape(n, -1)


def glare(fr, seed, sizes=GLARE_SIZES):
    """in place; -> [(kind, size)] and the discs as boolean (h, w) arrays"""
    g = np.random.default_rng(seed)
    n, h, w, _ = fr.shape
    yy, xx = np.mgrid[0:h, 0:w]
    kinds, discs = [], []
    for f in range(n):
        kind, size = ("white", "black", "noise")[f % 3], sizes[(f // 3) % len(sizes)]
        cy, cx = h * (0.45 + 0.1 * g.random()), w * (0.45 + 0.1 * g.random())
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= (size * w) ** 2
        if kind == "white":
            fr[f][disc] = 255
        elif kind == "black":
            fr[f][disc] = 0
        else:
            fr[f][disc] = g.integers(0, 256, (int(disc.sum()), 3), dtype=np.uint8)
        kinds.append((kind, size))
        discs.append(disc)
    return kinds, discs


def glare_set(mode):
    """-> (frames, payload, kinds, discs)"""
    fr, payload = frames(mode, GLARE_N, GLARE_SEED)
    kinds, discs = glare(fr, GLARE_DISC_SEED)
    return fr, payload, kinds, discs


def overload(fr, seed=9):
    """in place: 6 .. 12 noise patches of 40 .. 90 px per frame, far more damage than a block's parity covers (the patches of
    tests/test_gpu_erasure_decode.py::test_overload_never_wrong)"""
    g = np.random.default_rng(seed)
    h, w = fr.shape[1:3]
    for f in range(len(fr)):
        for _ in range(int(g.integers(6, 13))):
            s = int(g.integers(40, 91))
            y, x = int(g.integers(60, h - 60 - s)), int(g.integers(60, w - 60 - s))
            fr[f, y:y + s, x:x + s] = g.integers(0, 256, (s, s, 3), dtype=np.uint8)


def chunk_ok(geo, chunks, payload, masks):
    """-> (chunk equals the payload, chunk is in the mask), both (n, CHUNKS_PER_FRAME) bool"""
    n = len(masks)
    c = np.asarray(chunks).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    p = np.asarray(payload).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    good = (c == p).all(axis=2)
    inmask = ((np.asarray(masks, np.uint32)[:, None] >> np.arange(geo.CHUNKS_PER_FRAME)) & 1).astype(bool)
    return good, inmask


def sym_chunks(geo):
    return geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)
