"""The case table of the deskew warp (Deskewer::deskew = getPerspectiveTransform + warpPerspective): captures of random bytes, hostile quads,
odd capture sizes, every capture format. Pure numpy and deterministic; shared by tests/test_warp_cases.py (oracle against the reference build,
and the coverage conditions below) and tests/test_gpu_warp_cases.py (device against oracle).

Capture content is uniform random bytes -- for formats 12 / 420 the Y, U and V planes independently, for format 4 the alpha byte too -- so that a
tap taken one column or row off, or a chroma pair from the wrong column, changes output bytes. Every case has a capture of its own.

A quad class is a function of the capture size (and of the mode's frame size for `identity`), so that it applies at every size. The corners are
(top-left, top-right, bottom-left, bottom-right) as Corners::all() returns them; what they map to are the anchor centres 30 px inside the frame,
so the frame's pre-image is about 3 % larger than the quad on every side.

Quad classes left out: none. The non-finite classes (`nan`, `inf`, `nanall`) are in: every load of k_warp / remap_bilinear sits behind the
INT_MAX clamp, the +-32768 clamp and the bounds tests (a non-finite position ends as INT_MAX, then sx = 32767, then no tap), k_roi_boxes takes the
whole-capture branch on any comparison that a NaN fails, and k_convert_roi's loads depend on the box and the capture size alone.

The reference build's ref_deskew truncates the corners to point<int>: a class whose corners are no integers that fit an int has no answer there
(REF_NO_ANSWER) and is checked device against oracle only."""
from collections import namedtuple

import numpy as np

from oracle import pyref

ANCHOR = 30
FORMATS = (3, 4, 12, 420)
BASE = (1920, 1080)
ODD8 = (1282, 978)           # w % 8 == 2, h % 4 == 2: the size at which every quad class runs in every format beside 1920x1080
# the sizes every format can hold: w % 8 in {4, 6} (722 % 4 == 2), then the tiny ones
EVEN_SIZES = ((1284, 722), (1286, 722), (2, 2), (4, 2), (8, 8), (10, 6), (64, 40))
ODD_SIZES = ((1283, 977), (3, 3))        # RGB and RGBA only
TINY = ((2, 2), (4, 2), (3, 3), (8, 8), (10, 6), (64, 40))

Case = namedtuple("Case", "name w h fmt quad corners mode")


def _r(v):
    return int(np.floor(v + 0.5))


def _inscribed(w, h):
    X, Y = w - 1, h - 1
    return [(_r(.2 * X), _r(.1 * Y)), (_r(.8 * X), _r(.12 * Y)), (_r(.18 * X), _r(.9 * Y)), (_r(.82 * X), _r(.88 * Y))]


def _perm(order):
    return lambda w, h, iw, ih: [_inscribed(w, h)[k] for k in order]


def _overhang(w, h, iw, ih):
    m = max(2, _r(0.03 * min(w, h)))          # 32 px at 1080p; the anchors' 30 px inset adds another 3 % of the capture
    return [(-m, -m - 1), (w - 1 + m + 2, -m), (-m - 3, h - 1 + m), (w - 1 + m, h - 1 + m + 2)]


def _far(w, h, iw, ih):
    q = _inscribed(w, h)
    q[0] = (q[0][0] - _r(1.5 * w), q[0][1] - _r(1.2 * h))
    return q


def _perspective(w, h, iw, ih):
    X, Y = w - 1, h - 1
    return [(_r(.47 * X), _r(.1 * Y)), (_r(.53 * X), _r(.1 * Y)), (_r(.2 * X), _r(.9 * Y)), (_r(.8 * X), _r(.9 * Y))]


def _nearcollinear(w, h, iw, ih):
    a, b = w // 10, h // 10
    return [(a, b), (4 * a, 4 * b + 1), (6 * a, 6 * b - 1), (9 * a, 9 * b)]


def _collinear(w, h, iw, ih):
    a, b = w // 5, h // 5
    return [(a, b), (2 * a, 2 * b), (3 * a, 3 * b), (4 * a, 4 * b)]


def _fractional(w, h, iw, ih):
    return [(x + fx, y + fy) for (x, y), (fx, fy) in zip(_inscribed(w, h), ((.25, .5), (.75, .25), (.5, .75), (.25, .25)))]


def _one_corner(k, value):
    def f(w, h, iw, ih):
        q = _inscribed(w, h)
        q[k] = value
        return q
    return f


def _all_corners(v):
    return lambda w, h, iw, ih: [(-v, -v), (v, -v), (-v, v), (v, v)]


def identity_offset(w, h, iw, ih):
    return max(0, w - iw), max(0, h - ih)


def _identity(w, h, iw, ih):
    ox, oy = identity_offset(w, h, iw, ih)
    return [(ox + ANCHOR, oy + ANCHOR), (ox + iw - ANCHOR, oy + ANCHOR), (ox + ANCHOR, oy + ih - ANCHOR), (ox + iw - ANCHOR, oy + ih - ANCHOR)]


NAN, INF = float("nan"), float("inf")
QUADS = {
    "inscribed": _perm((0, 1, 2, 3)),
    "overhang": _overhang,                    # the pre-image overhangs all four sides: columns -1, sw-2, sw-1 and rows -1, sh-1 along whole edges
    "far": _far,                              # one corner far outside
    "mirrored": _perm((1, 0, 3, 2)),          # tl <-> tr, bl <-> br
    "rot90": _perm((2, 0, 3, 1)),
    "rot180": _perm((3, 2, 1, 0)),
    "rot270": _perm((1, 3, 0, 2)),
    "bowtie": _perm((0, 1, 3, 2)),            # bl <-> br: self-intersecting, the denominator changes sign inside the frame
    "perspective": _perspective,              # the top edge a tenth of the bottom edge
    "nearcollinear": _nearcollinear,          # one pixel off a common line
    "collinear": _collinear,                  # singular system: all-zero matrix, the frame is source pixel (0, 0)
    "coincident": lambda w, h, iw, ih: [(w // 2, h // 2)] * 4,          # the same
    "fractional": _fractional,
    "huge7": _one_corner(1, (1e7, -1e7)),     # the +-32768 clamp of the source position
    "huge7all": _all_corners(1e7),
    "huge30": _one_corner(3, (1e30, 1e30)),   # the INT_MIN..INT_MAX clamp of the fixed-point position
    "huge30all": _all_corners(1e30),
    "identity": _identity,                    # the frame 1:1 onto the capture's bottom-right region: every fx = fy = 0
    "nan": _one_corner(0, (NAN, 100.0)),
    "inf": _one_corner(3, (INF, -INF)),
    "nanall": lambda w, h, iw, ih: [(NAN, NAN)] * 4,
}
SINGULAR = ("collinear", "coincident")
NONFINITE = ("nan", "inf", "nanall")
# what the oracle's frame must look like for the case to cover its path (check_coverage)
COVER = {"overhang": "overhang", "far": "far", "inscribed": "rows", "mirrored": "rows", "rot90": "rows", "rot180": "rows", "rot270": "rows",
         "collinear": "constant", "coincident": "constant", "identity": "identity", "nan": "black", "inf": "black", "nanall": "black"}
# quad classes the reference build gives no answer for, with the reason. (The degenerate integer quads -- bow-tie, collinear, coincident, 1e7 --
# were run through ref_deskew once in a child process while this table was written: it returns for all of them.)
REF_NO_ANSWER = {name: "ref_deskew truncates corners to point<int>: these are not integers that fit an int"
                 for name in ("fractional", "huge30", "huge30all", "nan", "inf", "nanall")}
MODE_QUADS = ("inscribed", "overhang", "mirrored", "bowtie", "collinear", "coincident")


def frame_size(mode):
    return pyref.GEOMETRY[mode][:2]


def make(quad, w, h, fmt, mode=68):
    iw, ih = frame_size(mode)
    corners = np.array([v for p in QUADS[quad](w, h, iw, ih) for v in p], np.float32)
    return Case(f"{quad}-{w}x{h}-f{fmt}" + ("" if mode == 68 else f"-m{mode}"), w, h, fmt, quad, corners, mode)


def formats_of(w, h):
    return FORMATS if w % 2 == 0 and h % 2 == 0 else (3, 4)


def table():
    """mode 68: every quad class at 1920x1080 and at 1282x978 in every format; every other size with the inscribed and the overhanging quad (the tiny
    ones also with the identity and the coincident quad) in every format it can hold"""
    out = [make(q, w, h, fmt) for (w, h) in (BASE, ODD8) for fmt in FORMATS for q in QUADS]
    for (w, h) in EVEN_SIZES + ODD_SIZES:
        quads = ("inscribed", "overhang") + (("identity", "coincident") if (w, h) in TINY else ())
        out += [make(q, w, h, fmt) for fmt in formats_of(w, h) for q in quads]
    return out


def mode_table(mode):
    """modes 67 and 66: the quads of MODE_QUADS in every format at 1920x1080 and 1282x978; modes 4 and 8 (mode 68's geometry): one case each"""
    if mode == 4:
        return [make("overhang", *ODD8, 12, mode)]
    if mode == 8:
        return [make("bowtie", *ODD8, 420, mode)]
    return [make(q, w, h, fmt, mode) for (w, h) in (BASE, ODD8) for fmt in FORMATS for q in MODE_QUADS]


def batches(cases):
    """{(w, h, fmt): [cases]} in table order: one deskew call each"""
    out = {}
    for c in cases:
        out.setdefault((c.w, c.h, c.fmt), []).append(c)
    return out


def capture_bytes(w, h, fmt):
    return w * h * 3 // 2 if fmt in (12, 420) else w * h * (4 if fmt == 4 else 3)


def capture(case, k=0):
    """the raw capture buffer of a case (k: its place in the batch, so that no two captures of a call are alike)"""
    rng = np.random.default_rng([case.w, case.h, case.fmt, k])
    return rng.integers(0, 256, capture_bytes(case.w, case.h, case.fmt), dtype=np.uint8)


def batch_captures(cases):
    return np.ascontiguousarray(np.stack([capture(c, k) for k, c in enumerate(cases)]))


def rgb_view(O, buf, w, h, fmt):
    """the capture as the oracle (and the reference's get_rgb) sees it"""
    if fmt == 3:
        return buf.reshape(h, w, 3)
    out = np.zeros((h, w, 3), np.uint8)
    assert O.co_capture_to_rgb(pyref.P(buf), w, h, fmt, pyref.P(out)) == 0
    return out


def oracle_frame(O, rgb, corners, mode=68):
    """co_deskew of the oracle library built for `mode`"""
    import ctypes
    iw, ih = frame_size(mode)
    h, w = rgb.shape[:2]
    out = np.zeros((ih, iw, 3), np.uint8)
    rgb = np.ascontiguousarray(rgb)
    corners = np.ascontiguousarray(corners, np.float32)
    O.co_deskew(pyref.P(rgb), w, h, corners.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), pyref.P(out))
    return out


def expected(cases):
    """the oracle's frames of one batch (cases of one size, format and mode)"""
    mode = cases[0].mode
    O = pyref.oracle_lib(mode)
    return np.stack([oracle_frame(O, rgb_view(O, capture(c, k), c.w, c.h, c.fmt), c.corners, mode) for k, c in enumerate(cases)])


def integer_corners(case):
    c = case.corners.astype(np.float64)
    return bool(np.isfinite(c).all() and (c == np.rint(c)).all() and (np.abs(c) < 2 ** 31).all())


def check_coverage(case, frame, rgb):
    """the condition under which `case` still covers the path it is in the table for; `frame` is the oracle's, `rgb` the capture as it sees it"""
    kind = COVER.get(case.quad)
    black = ~frame.any(axis=2)
    if kind == "overhang":
        assert black[0].all() and black[-1].all() and black[:, 0].all() and black[:, -1].all(), case.name
        cy, cx = frame.shape[0] // 2, frame.shape[1] // 2
        assert frame[cy - 8:cy + 8, cx - 8:cx + 8].any(), case.name
    elif kind == "far":
        assert 0.05 < black.mean() < 0.95, (case.name, black.mean())
    elif kind == "rows":
        assert not black.all(axis=1).any(), case.name
    elif kind == "constant":
        assert (frame == frame[0, 0]).all(), case.name
        assert (frame[0, 0] == rgb[0, 0]).all(), case.name          # (today's oracle: the all-zero matrix reads source pixel (0, 0))
    elif kind == "black":
        assert black.all(), case.name
    elif kind == "identity":
        ih, iw = frame.shape[:2]
        ox, oy = identity_offset(case.w, case.h, iw, ih)
        want = np.zeros_like(frame)
        hh, ww = min(ih, case.h - oy), min(iw, case.w - ox)
        want[:hh, :ww] = rgb[oy:oy + hh, ox:ox + ww]
        assert (frame == want).all(), (case.name, int((frame != want).sum()))
