"""Deterministic camera captures with lens distortion, for the undistortion tests: clean frames drawn as perspective quads (tests/frames.py), then a
forward radial distortion applied in numpy (the inverse of what Undistort removes: every output pixel samples the sharp capture at
p * (1 + kd * r^2), r measured in units of a quarter of the width / height from the centre). kd > 0 pulls the content inward: barrel; kd < 0:
pincushion. Test-side manufacture only."""
import numpy as np

from libcimbar_amd import framegen
from tests import frames as F

# (name, (w, h), kd, quad as fractions of the capture, seed)
_QUAD = ((0.27, 0.06), (0.75, 0.09), (0.25, 0.95), (0.77, 0.92))


def _quad(w, h, q=_QUAD):
    return tuple((int(round(x * w)), int(round(y * h))) for x, y in q)


def radial_distort(rgb, kd):
    """out(p) = bilinear sample of rgb at c + (p - c) * (1 + kd * r^2), r = |(p - c) / (w/4, h/4)|; outside: 0"""
    h, w = rgb.shape[:2]
    cx, cy, fx, fy = w // 2, h // 2, w // 4, h // 4
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (xx - cx) / fx, (yy - cy) / fy
    s = 1 + kd * (nx * nx + ny * ny)
    sx, sy = cx + nx * s * fx, cy + ny * s * fy
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = sx - x0, sy - y0
    src = rgb.astype(np.float64)
    out = np.zeros_like(src)
    for dx, dy, wt in ((0, 0, (1 - ax) * (1 - ay)), (1, 0, ax * (1 - ay)), (0, 1, (1 - ax) * ay), (1, 1, ax * ay)):
        X, Y = x0 + dx, y0 + dy
        inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        out += src[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)] * (wt * inside)[..., None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _frame(seed):
    synth = framegen.FrameSynth("cpu")
    return F.clean_frames(synth, 1, seed=seed)[1][0]


def distorted(w, h, kd, seed, quad=_QUAD, background=96):
    cam = F.camera_frame(_frame(seed), width=w, height=h, quad=_quad(w, h, quad), background=background)
    return radial_distort(cam, kd) if kd else cam


def axis_aligned(w=1920, h=1080, seed=5):
    """the frame pasted 1:1 without perspective: opposite sides exactly parallel -> calibration fails (line_intersection NONE)"""
    img = np.full((h, w, 3), 96, np.uint8)
    fr = _frame(seed)
    y0, x0 = (h - 1024) // 2, (w - 1024) // 2
    img[y0:y0 + 1024, x0:x0 + 1024] = fr
    return img


def blank(w=1920, h=1080):
    return np.full((h, w, 3), 128, np.uint8)


# name -> (maker, formats it is also checked in). The 1080p captures are ones the anchor search finds (a frame drawn smaller, as at 720p here, is
# not: those exercise the failed-calibration path and, with explicit parameters, the remap at other sizes).
CASES = [
    ("barrel_1080", lambda: distorted(1920, 1080, 0.006, 11), (3, 4, 12, 420)),
    ("mild_barrel_1080", lambda: distorted(1920, 1080, 0.002, 11), (3,)),
    ("pincushion_1080", lambda: distorted(1920, 1080, -0.006, 11), (3, 12)),
    ("barrel_odd", lambda: np.ascontiguousarray(distorted(1920, 1080, 0.004, 11)[:1079, :1919]), (3, 4)),
    ("barrel_720", lambda: distorted(1280, 720, 0.004, 13), (3, 420)),
    ("axis_aligned", lambda: axis_aligned(), (3,)),
    ("blank", lambda: blank(), (3,)),
]

# explicit parameters (set_distortion_params): camera[9] + distortion[5] (k1 k2 p1 p2 k3); the second pushes the corners' taps outside the source
# (border zeros), the third has every coefficient non-zero
PARAMS = [
    ("naive_k1", lambda w, h: [w // 4, 0, w // 2, 0, h // 4, h // 2, 0, 0, 1, 0.01, 0, 0, 0, 0]),
    ("border_zeros", lambda w, h: [w / 3.0, 0, w / 2.0 + 3.5, 0, h / 3.0, h / 2.0 - 2.25, 0, 0, 1, 0.08, 0.01, 0, 0, 0]),
    ("full", lambda w, h: [w * 0.3, 0, w * 0.49, 0, h * 0.31, h * 0.52, 0, 0, 1, -0.021, 0.0042, 0.0013, -0.0008, -0.0005]),
]


def case(name):
    for n, mk, fmts in CASES:
        if n == name:
            return mk()
    raise KeyError(name)
