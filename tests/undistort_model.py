"""Test-side restatement of `cimbar --undistort` (src/exe/cimbar/cimbar.cpp:135-145): Undistort<SimpleCameraCalibration>::undistort
(src/lib/extractor/Undistort.h:11-62) in numpy / plain Python floats, the double arithmetic in the reference's order (Python floats and element-wise
numpy float64 operations are single IEEE operations: nothing fuses).

  calibrate(rgb)            SimpleCameraCalibration::scan (SimpleCameraCalibration.h:30-58, SimpleCameraCalibration.cpp:1-75): the binary plane and
                            the corners come from the existing oracle (co_scan_preprocess, co_extract -- used read-only); then
                            Geometry::calculate_midpoints (Geometry.h:15-75), Scanner::scan_edges / find_edge / chase_edge (Scanner.cpp:204-276,
                            EdgeScanState.h) and calculate_distortion_factor
  undistort_maps(...)       cv::initUndistortRectifyMap(camera, dist, Mat(), camera, size, CV_32FC1) [assumed-OpenCV: the scalar per-row walk, the
                            column running sum serially]
  remap(rgb, mx, my)        cv::remap(INTER_LINEAR, BORDER_CONSTANT 0): cvRound(map * 32) in float, weights (32-fx)(32-fy)*32 ... summing to 2^15
  undistort(rgb, params)    the whole of Undistort::undistort with a fresh object: (image, ok, k1)

chase_edge reads outside the image without a check upstream (undefined behaviour); like the device, a tap that leaves the plane is inactive.
find_edge's abs() is taken as the double overload (the one real OpenCV's headers make visible; see tests/cpp/cvshim_undistort.hpp).
"""
import ctypes
import math

import numpy as np

from oracle import pyref
from oracle.pyref import P

INF = float("inf")
NONE_D = (INF, INF)                       # point<double>::NONE()
TARGET_RATIO = math.sqrt(729.0) / math.sqrt(929296.0)   # edge_to_anchor_ratio(1024, 30, 3), SimpleCameraCalibration.cpp:14-21,38-41
ANCHOR_SIZE = 30                          # Scanner::_anchorSize


def to_rgb(img, w, h, fmt):
    """a capture in the C ABI's `format` -> (h, w, 3) RGB8, through the oracle's get_rgb restatement"""
    if fmt in (3, 0) or fmt < 0:
        return np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 3))
    out = np.zeros((h, w, 3), np.uint8)
    src = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(-1))
    assert pyref.oracle_lib().co_capture_to_rgb(P(src), w, h, fmt, P(out)) == 0
    return out


def scan(rgb):
    """Scanner(img): (binary plane (h, w) of 0/255, status, corners [tl, tr, bl, br] as int pairs or None)"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    L = pyref.oracle_lib()
    binary = np.zeros((h, w), np.uint8)
    L.co_scan_preprocess(P(rgb), w, h, P(binary))
    frame = np.zeros((1024, 1024, 3), np.uint8)
    c8 = (ctypes.c_float * 8)()
    status = L.co_extract(P(rgb), w, h, P(frame), c8)
    if status <= 0:
        return binary, status, None
    c = [int(v) for v in c8]
    return binary, status, [(c[0], c[1]), (c[2], c[3]), (c[4], c[5]), (c[6], c[7])]


def line_intersection(a, b):
    """Geometry::line_intersection (Geometry.h:17-38)"""
    (p0, q0), (p1, q1) = a, b
    ax, ay, adet = q0[0] - p0[0], p0[1] - q0[1], q0[0] * p0[1] - p0[0] * q0[1]
    bx, by, bdet = q1[0] - p1[0], p1[1] - q1[1], q1[0] * p1[1] - p1[0] * q1[1]
    D = ay * bx - ax * by
    if abs(D) < 1e-8:
        return NONE_D
    Dx = adet * bx - ax * bdet
    Dy = ay * bdet - adet * by
    return (Dx / D, Dy / D)


def calculate_midpoints(tl, tr, bl, br):
    """Geometry::calculate_midpoints: [top, right, bottom, left], or [] (then Scanner::scan_edges returns no edges)"""
    f = lambda p: (float(p[0]), float(p[1]))
    tl, tr, bl, br = f(tl), f(tr), f(bl), f(br)
    center = line_intersection((tl, br), (tr, bl))
    if center == NONE_D:
        return []
    lr_inf = line_intersection((tr, br), (tl, bl))
    if lr_inf == NONE_D:
        return []
    tb_inf = line_intersection((tl, tr), (bl, br))
    if tb_inf == NONE_D:
        return []
    vertical, horizontal = (center, lr_inf), (center, tb_inf)
    return [line_intersection((tl, tr), vertical), line_intersection((tr, br), horizontal),
            line_intersection((bl, br), vertical), line_intersection((tl, bl), horizontal)]


class Plane:
    """Scanner::test_pixel on the binary plane (`pixel > 127`); outside the plane: inactive"""

    def __init__(self, binary):
        self.b = binary
        self.h, self.w = binary.shape

    def test(self, x, y):
        # (x, y) doubles, truncated as the reference's int conversions do
        if not (x > -1.0 and x < self.w and y > -1.0 and y < self.h):
            return False
        return self.b[int(y), int(x)] > 127


def chase_edge(pl, start, unit):
    success = 0
    for i in (-2, -1, 1, 2):
        x = math.trunc(start[0] + (unit[0] * i))
        y = math.trunc(start[1] + (unit[1] * i))
        if pl.test(x, y):
            success += 1
    return success >= 2


def find_edge(pl, u, v, mid):
    """Scanner::find_edge -> (x, y) ints or None (point<int>::NONE())"""
    dv = (float(v[0]) - float(u[0]), float(v[1]) - float(u[1]))
    dunit = (dv[0] / 512.0, dv[1] / 512.0)
    out_v = (dv[1] / 64, dv[0] / -64)
    in_v = (-out_v[0], -out_v[1])
    if mid == NONE_D:
        mid = (float(u[0]) + dv[0] / 2.0, float(u[1]) + dv[1] / 2.0)
    adj = ANCHOR_SIZE / 16.0
    mid = (mid[0] + out_v[0] * adj, mid[1] + out_v[1] * adj)
    for check in (out_v, in_v):
        max_check = max(abs(check[0]), abs(check[1]))
        unit = (check[0] / max_check, check[1] / max_check)
        state, run = 0, 0
        i = j = 0.0
        while abs(i) <= abs(check[0]) and abs(j) <= abs(check[1]):
            x, y = mid[0] + i, mid[1] + j
            if x < 0 or x >= pl.w or y < 0 or y >= pl.h:
                i += unit[0]
                j += unit[1]
                continue
            active = pl.test(x, y)
            size = -1
            if state == 0:
                if active:
                    state, run = 1, 1
            elif active:
                run += 1
            else:
                state, size = 0, run
            if size > 0:
                edge = (x - (unit[0] * size / 2), y - (unit[1] * size / 2))
                if chase_edge(pl, edge, dunit):
                    return (math.trunc(edge[0]), math.trunc(edge[1]))
            i += unit[0]
            j += unit[1]
    return None


def distortion_factor(corners, mids, edges):
    """SimpleCameraCalibration::calculate_distortion_factor"""
    tl, tr, bl, br = corners
    ratios = []
    for e, m, s, t in zip(edges, mids, (tl, tr, br, bl), (tr, br, bl, tl)):
        if e is None:
            continue
        num = math.sqrt((m[0] - e[0]) ** 2 + (m[1] - e[1]) ** 2) if m != NONE_D else INF
        den = math.sqrt(float((t[0] - s[0]) ** 2 + (t[1] - s[1]) ** 2))
        ratios.append(num / den)
    if not ratios:
        return 0.0
    total = 0.0
    for r in ratios:
        total += r
    smallest = TARGET_RATIO - total / len(ratios)
    for r in ratios:
        dist = TARGET_RATIO - r
        if abs(dist) < abs(smallest):
            smallest = dist
    return smallest


def calibrate(rgb):
    """SimpleCameraCalibration::scan -> (ok, k1)"""
    binary, status, corners = scan(rgb)
    if corners is None:
        return 0, 0.0
    tl, tr, bl, br = corners
    mids = calculate_midpoints(tl, tr, bl, br)
    if len(mids) < 4:
        return 0, 0.0
    pl = Plane(binary)
    edges = [find_edge(pl, tl, tr, mids[0]), find_edge(pl, tr, br, mids[1]), find_edge(pl, br, bl, mids[2]), find_edge(pl, bl, tl, mids[3])]
    return 1, distortion_factor(corners, mids, edges)


def naive_camera(w, h):
    """naive_radial_undistort (SimpleCameraCalibration.h:50-58), integer division"""
    return [float(w // 4), 0.0, float(w // 2), 0.0, float(h // 4), float(h // 2), 0.0, 0.0, 1.0]


def invert3x3(S):
    """[assumed-OpenCV] lapack.cpp invert(), 3x3 CV_64F closed form"""
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    assert d != 0.0
    d = 1.0 / d
    return [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
            (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
            (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]


def undistort_maps(w, h, camera, dist):
    """initUndistortRectifyMap(camera, dist (k1 k2 p1 p2 [k3]), Mat(), camera, (w, h), CV_32FC1) for a zero-skew camera -> (map1, map2) float32.
    [assumed-OpenCV] per row i: _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8], then _x += ir[0] (_y += ir[3], _w += ir[6]) per
    column, serially; here ir[1] = ir[3] = ir[6] = ir[7] = 0, so the columns' _x is one sequence for every row."""
    ir = invert3x3(camera)
    assert camera[1] == 0 and camera[3] == 0 and camera[6:] == [0.0, 0.0, 1.0]
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) >= 5 else 0.0
    fx, fy, u0, v0 = camera[0], camera[4], camera[2], camera[5]
    winv = 1.0 / ir[8]
    xs = np.empty(w, np.float64)
    _x = 0 * ir[1] + ir[2]
    for j in range(w):                    # the running sum: a plain sequential loop
        xs[j] = _x * winv
        _x += ir[0]
    ys = (np.arange(h, dtype=np.float64) * ir[4] + ir[5]) * winv
    x = np.broadcast_to(xs[None, :], (h, w))
    y = np.broadcast_to(ys[:, None], (h, w))
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2       # / (1 + ((k6*r2 + k5)*r2 + k4)*r2) = / 1 exactly
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
    return (fx * xd + u0).astype(np.float32), (fy * yd + v0).astype(np.float32)


def _cv_round32(m):
    """cvRound(float) of map * INTER_TAB_SIZE: round half to even, out of int range / NaN -> INT_MIN"""
    v = m * np.float32(32)
    okv = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    r = np.where(okv, np.rint(np.where(okv, v, 0)), 0).astype(np.int64)
    return np.where(okv, r, -2147483648).astype(np.int64)


def remap(rgb, map1, map2):
    """cv::remap(rgb, out, map1, map2, INTER_LINEAR, BORDER_CONSTANT) for RGB8 and CV_32FC1 maps"""
    src = np.asarray(rgb, np.uint8)
    sh, sw = src.shape[:2]
    X, Y = _cv_round32(map1), _cv_round32(map2)
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    w = [((32 - fx) * (32 - fy) * 32, 0, 0), (fx * (32 - fy) * 32, 1, 0), ((32 - fx) * fy * 32, 0, 1), (fx * fy * 32, 1, 1)]
    acc = np.zeros(map1.shape + (3,), np.int64)
    for wt, dx, dy in w:
        xx, yy = sx + dx, sy + dy
        inside = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        px = src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)].astype(np.int64)
        acc += px * np.where(inside, wt, 0)[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def undistort(rgb, params=None):
    """Undistort<SimpleCameraCalibration>().undistort(img, out) with a fresh object -> (out, ok, k1). params: camera[9] + distortion[5] or None.
    A failed calibration leaves the image as it was (cimbar.cpp:139-141): out = rgb."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    if params is None:
        ok, k1 = calibrate(rgb)
        if not ok:
            return rgb.copy(), 0, 0.0
        camera, dist = naive_camera(w, h), [k1, 0.0, 0.0, 0.0]
    else:
        p = [float(v) for v in params]
        camera, dist = p[:9], p[9:14]
        ok, k1 = 1, dist[0]
    m1, m2 = undistort_maps(w, h, camera, dist)
    return remap(rgb, m1, m2), ok, k1
