"""CPU: the capture formats of native receivers (NV21 21, YUYV 422, UYVY 4221, BGR 30, BGRA 40; include/cimbar_hip.h) -- what needs no device:
the byte counts, the test helper that says which RGB image such a capture is (tests/capture_formats_native.py) on known values, and what the
Python wrapper accepts."""
import ctypes

import numpy as np
import pytest

from libcimbar_amd import decoder as D
from oracle.pyref import P
from tests import capture_formats_native as CN


def test_capture_bytes_of_the_native_formats():
    lib = D.load_library()
    for (w, h) in ((1920, 1080), (64, 40), (2, 2)):
        for fmt in CN.NATIVE:
            assert lib.cimbar_hip_capture_bytes(w, h, fmt) == CN.capture_bytes(w, h, fmt), (w, h, fmt)
    # 4:2:2 needs an even width and takes any height; NV21 needs both even; BGR / BGRA take anything
    for fmt in (422, 4221):
        assert lib.cimbar_hip_capture_bytes(63, 64, fmt) == 0
        assert lib.cimbar_hip_capture_bytes(64, 63, fmt) == 64 * 63 * 2
    assert lib.cimbar_hip_capture_bytes(63, 64, 21) == 0 and lib.cimbar_hip_capture_bytes(64, 63, 21) == 0
    assert lib.cimbar_hip_capture_bytes(63, 61, 30) == 63 * 61 * 3 and lib.cimbar_hip_capture_bytes(63, 61, 40) == 63 * 61 * 4
    # their neighbours are none of the nine values: RGB8, as every other value (0, negatives, 5 and 7 among them)
    for fmt in (22, 31, 41, 423, 0, -3, 5, 7):
        assert lib.cimbar_hip_capture_bytes(63, 61, fmt) == 63 * 61 * 3, fmt


def test_format_constants():
    assert (D.FMT_RGB, D.FMT_RGBA, D.FMT_NV12, D.FMT_I420) == (3, 4, 12, 420)
    assert (D.FMT_NV21, D.FMT_YUYV, D.FMT_UYVY, D.FMT_BGR, D.FMT_BGRA) == CN.NATIVE


def test_known_yuv_triples_in_the_native_layouts(oracle):
    """the (Y, U, V) -> (R, G, B) triples of tests/test_capture_formats.py::test_known_yuv_triples as 2-pixel YUYV / UYVY rows and a 2x2 NV21 image"""
    cases = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (81, 90, 240): (254, 0, 0), (145, 54, 34): (0, 255, 1),
             (41, 240, 110): (0, 0, 255), (0, 128, 128): (0, 0, 0), (255, 128, 128): (255, 255, 255), (128, 0, 255): (255, 77, 0),
             (200, 255, 0): (10, 255, 255), (17, 129, 127): (0, 2, 3)}
    for (y, u, v), want in cases.items():
        for fmt, img, w, h in ((422, [y, u, y, v], 2, 1), (4221, [u, y, v, y], 2, 1), (21, [y] * 4 + [v, u], 2, 2)):
            out = CN.to_rgb(oracle, np.array(img, np.uint8), w, h, fmt)
            assert (out.reshape(-1, 3) == np.array(want, np.uint8)).all(), (fmt, (y, u, v), out.reshape(-1, 3)[0])


def test_the_422_rule_one_chroma_pair_per_group_and_row(oracle):
    """two rows, two groups, four different chroma pairs: every pixel takes the pair of its own group in its own row"""
    groups = [[(81, 90, 240), (145, 54, 34)], [(41, 240, 110), (128, 0, 255)]]          # [row][group] = (Y, U, V)
    want = [[(254, 0, 0), (0, 255, 1)], [(0, 0, 255), (255, 77, 0)]]
    for fmt in (422, 4221):
        img = [b for row in groups for (y, u, v) in row for b in ((y, u, y, v) if fmt == 422 else (u, y, v, y))]
        out = CN.to_rgb(oracle, np.array(img, np.uint8), 4, 2, fmt)
        for r in range(2):
            for g in range(2):
                assert (out[r, 2 * g: 2 * g + 2] == np.array(want[r][g], np.uint8)).all(), (fmt, r, g)


def test_manufactured_captures_come_back(oracle):
    """rgb_to_native and to_rgb are each other's inverse up to the chroma subsampling: a flat colour survives to within the BT.601 rounding"""
    rgb = np.zeros((6, 8, 3), np.uint8)
    rgb[:] = (200, 60, 30)
    for fmt in CN.NATIVE:
        back = CN.to_rgb(oracle, CN.rgb_to_native(rgb, fmt), 8, 6, fmt)
        assert np.abs(back.astype(int) - rgb.astype(int)).max() <= (0 if fmt in (30, 40) else 2), fmt
    odd = np.random.default_rng(2).integers(0, 256, (5, 8, 3), dtype=np.uint8)            # an odd height: 4:2:2 and BGR / BGRA only
    for fmt in CN.ANY_HEIGHT:
        assert CN.to_rgb(oracle, CN.rgb_to_native(odd, fmt), 8, 5, fmt).shape == (5, 8, 3)


def test_helper_bgr_equals_the_reference_builds_cvtcolor(oracle, ref):
    rng = np.random.default_rng(30)
    for (w, h) in ((16, 8), (71, 37)):
        img = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
        want = np.zeros((h, w, 3), np.uint8)
        assert ref.ref_cvtcolor(P(img), h, w, 3, CN.CV_CODE[30], P(want)) == h
        assert (CN.to_rgb(oracle, img, w, h, 30) == want).all()


def test_python_wrapper_takes_the_native_formats():
    lib = D.load_library()
    w, h, n = 16, 8, 2
    for fmt in CN.NATIVE:
        flat = np.zeros((n, CN.capture_bytes(w, h, fmt)), np.uint8)
        assert D._captures(lib, flat, (w, h), fmt)[1:] == (n, w, h, fmt)
        with pytest.raises(D.CimbarHipError):
            D._captures(lib, flat[:, :-1], (w, h), fmt)                 # no whole number of captures
    for fmt in (21, 422, 4221):
        with pytest.raises(D.CimbarHipError):
            D._captures(lib, np.zeros((n, 15 * 8 * 2), np.uint8), (15, 8), fmt)   # a width the layout cannot hold
    # without size=: what the array's shape describes, and nothing else
    bgr, bgra = np.zeros((n, h, w, 3), np.uint8), np.zeros((n, h, w, 4), np.uint8)
    assert D._captures(lib, bgr, None, 30)[1:] == (n, w, h, 30)
    assert D._captures(lib, bgra, None, 40)[1:] == (n, w, h, 40)
    assert D._captures(lib, bgr, None, 3)[1:] == (n, w, h, 3) and D._captures(lib, bgra, None, 4)[1:] == (n, w, h, 4)
    for bad_fmt, bad in ((30, bgra), (40, bgr), (21, bgr), (422, bgr), (4221, bgra), (422, np.zeros((n, w * h * 2), np.uint8)), (30, np.zeros((n, w * h * 3), np.uint8))):
        with pytest.raises(D.CimbarHipError):
            D._captures(lib, bad, None, bad_fmt)
