"""Inputs of tests/test_gpu_settings_matrix.py: the opt-in decode settings, a pool of a dozen rendered frames per mode that makes each of them
bite, and the sequences that put pool frames at the part boundaries of the split chain. Imports without a GPU and without the library
(tests/test_setting_cases.py checks sequence() on the CPU).

The pool is made of distortions other suites already use, one payload frame per pool frame (so that no two neighbours are captures of one
displayed frame): clean frames, the disc glare of the erasure suites, a small disc from the colour erasure suite's glare set, rigid shifts,
rescales, pixel noise over a shift, a tear, and a noise disc over a shifted frame.
"""
import functools

import numpy as np

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from tests import colour_erasure_cases as K
from tests import frames as F

T_SYM = 6                      # tests/test_gpu_erasure_decode.py
RF_ACCEPT, RF_FALLBACK = 12, 32    # tests/test_gpu_relaxed_flood.py: 32 is where frames of both kinds turn up
SEED = {68: 4168, 66: 4166}


# ------------------------------------------------------------------ the settings
def off(dec):
    pass


def sym(dec):
    dec.set_erasure_decode(T_SYM)


def col(dec):
    dec.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)


def rf_accept(dec):
    dec.set_relaxed_flood(RF_ACCEPT, fallback=False)


def rf_fallback(dec):
    dec.set_relaxed_flood(RF_FALLBACK, fallback=True)


def all(dec):          # noqa: A001 (the name the matrix uses)
    sym(dec)
    col(dec)
    rf_fallback(dec)


SETTINGS = [off, sym, col, rf_accept, rf_fallback, all]
NAMES = [s.__name__ for s in SETTINGS]
BY_NAME = {s.__name__: s for s in SETTINGS}
RELAXED = ("rf_accept", "rf_fallback", "all")


# ------------------------------------------------------------------ the pool
def tear(c, cut):
    """tests/test_gpu_relaxed_flood.py::tear"""
    return np.concatenate([F.shift(c, 1, 0)[:cut], F.shift(c, 0, 1)[cut:]], 0)


def disc(frame, kind, size, seed):
    """one frame of the erasure suites' glare (tests/test_gpu_erasure_decode.py::_glare): a white disc or a disc of noise, radius size * width,
    centred a little off the middle"""
    g = np.random.default_rng(seed)
    h, w, _ = frame.shape
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = h * (0.45 + 0.1 * g.random()), w * (0.45 + 0.1 * g.random())
    inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= (size * w) ** 2
    out = frame.copy()
    out[inside] = 255 if kind == "white" else g.integers(0, 256, (int(inside.sum()), 3), dtype=np.uint8)
    return out


# pool frames taken from the colour erasure suite's glare set as they are (tests/colour_erasure_cases.py::glare_set: frame k has disc kind
# k % 3, radius GLARE_SIZES[k // 3 % 4]) instead of made by the recipe below.
# colour_glare: the noise discs of radius 0.07 / 0.09, which gain colour chunks under `col` and leave the parallel path.
# white13 in mode 66: whether the certifying pass settles a frame with a white disc can depend on the order its lanes queue the disc's tied
# cells in (tests/test_gpu_settings_matrix.py); the set's white disc of radius 0.13 is one it declined in every run.
GLARE_FRAMES = {68: {"colour_glare": 5}, 66: {"colour_glare": 8, "white13": 9}}
# pool frames in pool order: (name, maker(c, h) on the pool's own payload frame c)
RECIPES = [
    ("clean0", lambda c, h: c),
    ("white13", lambda c, h: disc(c, "white", 0.13, 8)),
    ("shift+2+1", lambda c, h: F.shift(c, 2, 1)),
    ("rescale6", lambda c, h: F.rescale(c, 6)),
    ("noise10", lambda c, h: disc(c, "noise", 0.10, 9)),
    ("noise60_shift+1-2", lambda c, h: F.add_noise(F.shift(c, 1, -2), 60, 0)),
    ("colour_glare", None),
    ("shift-3+3", lambda c, h: F.shift(c, -3, 3)),
    ("rescale10", lambda c, h: F.rescale(c, 10)),
    ("tear", lambda c, h: tear(c, h * 500 // 1024)),
    ("noise10_shift", lambda c, h: disc(F.add_noise(F.shift(c, 1, -2), 60, 3), "noise", 0.10, 4)),
    ("clean1", lambda c, h: c),
]
POOL_NAMES = [r[0] for r in RECIPES]
CLEAN = (POOL_NAMES.index("clean0"), POOL_NAMES.index("clean1"))
# what tests/test_gpu_settings_matrix.py::test_baseline asserts of the pool on the device, per mode: a pool frame that takes the exact replay
# under rf_fallback (path 1) and one whose rounds are accepted (path 3). sequence() places them by these.
FALLS_BACK = {68: POOL_NAMES.index("rescale6"), 66: POOL_NAMES.index("rescale6")}
ACCEPTED = {68: POOL_NAMES.index("tear"), 66: POOL_NAMES.index("tear")}


@functools.lru_cache(maxsize=None)
def pool(mode):
    """-> (frames (12, h, w, 3) uint8, payload (12, FRAME_BYTES) uint8): the payload is the reference no kernel has touched"""
    geo = geometry.for_mode(mode)
    n = len(RECIPES)
    payload = framegen.synth_payload(n, seed=SEED[mode], mode=mode)
    clean = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy()
    payload = payload.numpy().reshape(n, -1).copy()
    frames = np.empty_like(clean)
    for k, (name, make) in enumerate(RECIPES):
        if name in GLARE_FRAMES[mode]:
            gf, gp, _, _ = K.glare_set(mode)
            frames[k], payload[k] = gf[GLARE_FRAMES[mode][name]], gp[GLARE_FRAMES[mode][name]]
        else:
            frames[k] = make(clean[k], geo.IMG_H)
    frames.setflags(write=False)
    payload.setflags(write=False)
    return frames, payload


def thrice(frames, payload):
    """every frame shown three times in a row, the second and third capture with light pixel noise (uniform in -8 .. 8: cheaper to draw than
    frames.add_noise's normal deviates, and the captures of a frame only have to differ)"""
    g = np.random.default_rng(100)
    out = np.repeat(frames, 3, axis=0)
    for k in range(len(out)):
        if k % 3:
            out[k] = np.clip(out[k].astype(np.int16) + g.integers(-8, 9, out[k].shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return out, np.repeat(payload, 3, axis=0)


# ------------------------------------------------------------------ the payload rule
def chunk_bits(geo, masks):
    return ((np.asarray(masks, np.uint32)[:, None] >> np.arange(geo.CHUNKS_PER_FRAME)) & 1).astype(bool)


def assert_payload_rule(geo, chunks, masks, payload, tag=""):
    """every chunk whose mask bit is set equals the payload's chunk, every slot outside the mask is zero"""
    n = len(masks)
    c = np.asarray(chunks).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    p = np.asarray(payload).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    inmask = chunk_bits(geo, masks)
    assert (np.asarray(masks, np.uint32) >> geo.CHUNKS_PER_FRAME == 0).all(), f"{tag}: mask bits past the last chunk"
    wrong = inmask & ~(c == p).all(axis=2)
    assert not wrong.any(), f"{tag}: chunks in the mask differ from the payload at (frame, chunk) {np.argwhere(wrong)[:8].tolist()}"
    dirty = ~inmask & c.any(axis=2)
    assert not dirty.any(), f"{tag}: slots outside the mask are not zero at (frame, chunk) {np.argwhere(dirty)[:8].tolist()}"


# ------------------------------------------------------------------ sequences for the split chain
def part_lo(n, parts, q):
    """host.hip.inc, enqueue(): part q of a split batch starts at frame n * q / parts"""
    return n * q // parts


def sequence(n, parts, mode=66):
    """the pool index per position of a batch of n frames that splits into `parts`: clean frames except
    - on both sides of every part boundary: before an odd boundary the frame that falls back and behind it the other distorted frames in turn,
      around an even one the other way round (with two parts the one boundary has the falling-back frame on both sides);
    - at positions 0 and n - 1;
    - and, while fewer than 15 and no more than one position in eight are distorted, in the middle of the parts, so that every distorted pool
      frame turns up. (15: a batch that hands 16 flagged frames on and certifies none of them switches the certifying pass off for the next
      batch, and the path of a frame would then depend on the batch before.)"""
    fb = FALLS_BACK[mode]
    others = [k for k in range(len(POOL_NAMES)) if k not in CLEAN and k != fb]
    seq = [CLEAN[p & 1] for p in range(n)]
    turn = iter(others * 4)
    distorted = set()

    def put(p, k):
        seq[p] = k
        distorted.add(p)

    put(0, next(turn))
    put(n - 1, next(turn))
    for q in range(1, parts):
        lo = part_lo(n, parts, q)
        if parts == 2:
            put(lo - 1, fb), put(lo, fb)
        elif q & 1:
            put(lo - 1, fb), put(lo, next(turn))
        else:
            put(lo - 1, next(turn)), put(lo, fb)
    budget = min(15, n // 8)
    q = 0
    while len(distorted) < budget and q < 4 * parts:
        p = (part_lo(n, parts, q // 4) + part_lo(n, parts, q // 4 + 1)) // 2 + 3 * (q % 4)
        if p not in distorted and 0 < p < n - 1:
            put(p, next(turn))
        q += 1
    return seq


def short_sequence(n=16):
    """the whole pool in pool order, then clean frames and the frame that falls back once more: for the unsplit shapes"""
    k = len(POOL_NAMES)
    return [p if p < k else (CLEAN[p & 1] if p & 2 else FALLS_BACK[66]) for p in range(n)]
