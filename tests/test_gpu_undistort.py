"""GPU: lens undistortion (`cimbar --undistort`, cimbar.cpp:135-145) -- cimbar_hip_undistort_calibrate_fmt, cimbar_hip_undistort_batch_fmt and
cimbar_hip_scan_undistort_extract_decode_batch_fmt -- bit for bit against the numpy restatement (tests/undistort_model.py) and, where the
capture is the one the golden file was made from, against the reference's own code (tests/golden/undistort.json)."""
import hashlib
import json
import os

import numpy as np
import pytest

from libcimbar_amd import decoder as D
from tests import capture_formats as CF
from tests import distorted_captures as DC
from tests import undistort_model as UM

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort.json")

_cache = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden():
    if "golden" not in _cache:
        _cache["golden"] = json.load(open(GOLDEN))["cases"] if os.path.exists(GOLDEN) else {}
    return _cache["golden"]


def capture(name):
    """(rgb capture, model (image, ok, k1)) of a case, computed once"""
    if name not in _cache:
        rgb = DC.case(name)
        _cache[name] = (rgb, UM.undistort(rgb))
    return _cache[name]


def in_format(rgb, fmt):
    """the capture in `fmt` and the RGB image the reference would see (get_rgb of it)"""
    h, w = rgb.shape[:2]
    img = CF.rgb_to_format(rgb, fmt)
    return img, (rgb if fmt == 3 else UM.to_rgb(img, w, h, fmt))


def case_params():
    return [(name, fmt) for name, _, fmts in DC.CASES for fmt in fmts]


@pytest.mark.parametrize("name,fmt", case_params())
def test_calibrate_and_undistort_match_model(hip_decoder, name, fmt):
    rgb, _ = capture(name)
    h, w = rgb.shape[:2]
    img, seen = in_format(rgb, fmt)
    want_img, want_ok, want_k1 = capture(name)[1] if fmt == 3 else UM.undistort(seen)
    ok, k1 = hip_decoder.undistort_calibrate(img[None], size=(w, h), fmt=fmt)
    assert ok[0] == want_ok and k1[0].tobytes() == np.float64(want_k1).tobytes(), (ok[0], k1[0], want_ok, want_k1)
    out, ok2, k2 = hip_decoder.undistort_batch(img[None], size=(w, h), fmt=fmt)
    assert ok2[0] == want_ok and k2[0].tobytes() == k1[0].tobytes()
    assert (out[0] == want_img).all(), f"{name} fmt {fmt}: {(out[0] != want_img).any(-1).sum()} pixels differ"
    g = golden().get(name)
    if g and fmt == 3 and g["capture_sha256"] == sha(rgb):
        assert g["ok"] == int(ok[0]) and g["k1_hex"] == float(k1[0]).hex()
        assert g["undistorted_sha256"] == sha(out[0])


@pytest.mark.parametrize("pname", [p for p, _ in DC.PARAMS])
@pytest.mark.parametrize("name,fmt", [("barrel_odd", 3), ("barrel_odd", 4), ("barrel_720", 420), ("barrel_1080", 12)])
def test_explicit_params_match_model(hip_decoder, name, fmt, pname):
    rgb, _ = capture(name)
    h, w = rgb.shape[:2]
    params = dict(DC.PARAMS)[pname](w, h)
    img, seen = in_format(rgb, fmt)
    want, _, _ = UM.undistort(seen, params)
    out, ok, k1 = hip_decoder.undistort_batch(img[None], params=params, size=(w, h), fmt=fmt)
    assert ok[0] == 1 and k1[0] == params[9]
    assert (out[0] == want).all(), f"{(out[0] != want).any(-1).sum()} pixels differ"
    g = golden().get(name + "+" + pname)
    if g and fmt == 3 and g["capture_sha256"] == sha(rgb):
        assert g["undistorted_sha256"] == sha(out[0])


def test_k1_zero_is_a_copy(hip_decoder):
    rgb, _ = capture("barrel_odd")
    h, w = rgb.shape[:2]
    out, ok, _ = hip_decoder.undistort_batch(rgb[None], params=[w // 4, 0, w // 2, 0, h // 4, h // 2, 0, 0, 1, 0, 0, 0, 0, 0])
    assert ok[0] == 1 and (out[0] == rgb).all()


@pytest.mark.parametrize("fmt", [3, 12])
def test_composite_equals_extract_decode_of_model_images(hip_decoder, fmt):
    """status, masks and chunks of the composite == cimbar_hip_scan_extract_decode_batch_fmt run on the model's undistorted images"""
    names = ["barrel_1080", "pincushion_1080", "mild_barrel_1080", "axis_aligned", "blank"]
    rgbs = [capture(n)[0] for n in names]
    imgs, seen = zip(*[in_format(r, fmt) for r in rgbs])
    models = [capture(n)[1] if fmt == 3 else UM.undistort(s) for n, s in zip(names, seen)]
    hip_decoder.reset_ccm()
    total, chunks, masks, status, ok = hip_decoder.scan_undistort_extract_decode_batch(np.stack(imgs), size=(1920, 1080), fmt=fmt)
    hip_decoder.reset_ccm()
    t2, c2, m2, s2 = hip_decoder.scan_extract_decode_batch(np.stack([m[0] for m in models]))
    assert list(ok) == [m[1] for m in models]
    assert (status == s2).all() and (masks == m2).all() and (chunks == c2).all() and total == t2
    # the golden file decodes every capture on its own (CCM reset): so does this check
    for k, n in enumerate(names):
        g = golden().get(n)
        if g and fmt == 3 and g["capture_sha256"] == sha(rgbs[k]):
            hip_decoder.reset_ccm()
            _, c1, m1, s1, _ = hip_decoder.scan_undistort_extract_decode_batch(imgs[k][None], size=(1920, 1080), fmt=fmt)
            assert g["extract_status"] == int(s1[0])
            if s1[0] > 0:
                assert g["mask"] == int(m1[0]) and g["chunks_sha256"] == sha(c1[0])


def test_batch_of_64_crosses_groups(hip_decoder):
    """64 1080p captures: more than one group of the undistortion scratch (43 at 1080p); every capture as the model says"""
    names = ["barrel_1080", "pincushion_1080", "mild_barrel_1080", "axis_aligned", "blank"]
    order = [names[(k * 3) % len(names)] for k in range(64)]
    batch = np.stack([capture(n)[0] for n in order])
    ok, k1 = hip_decoder.undistort_calibrate(batch)
    out, ok2, k2 = hip_decoder.undistort_batch(batch)
    for k, n in enumerate(order):
        want_img, want_ok, want_k1 = capture(n)[1]
        assert ok[k] == ok2[k] == want_ok and k1[k].tobytes() == k2[k].tobytes() == np.float64(want_k1).tobytes(), k
        assert (out[k] == want_img).all(), k
    hip_decoder.reset_ccm()
    total, chunks, masks, status, uok = hip_decoder.scan_undistort_extract_decode_batch(batch)
    hip_decoder.reset_ccm()
    t2, c2, m2, s2 = hip_decoder.scan_extract_decode_batch(out)
    assert (uok == ok).all() and (status == s2).all() and (masks == m2).all() and (chunks == c2).all() and total == t2


def test_malformed_calls_are_einval(hip_decoder):
    lib, ctx = hip_decoder._lib, hip_decoder._ctx
    rgb, _ = capture("barrel_odd")
    h, w = rgb.shape[:2]
    out = np.zeros_like(rgb)
    ok = np.zeros(1, np.int32)
    k1 = np.zeros(1, np.float64)
    p = lambda a: a.ctypes.data
    skew = np.array([w / 4, 0.5, w / 2, 0, h / 4, h / 2, 0, 0, 1, 0.01, 0, 0, 0, 0], np.float64)
    bottom = np.array([w / 4, 0, w / 2, 0, h / 4, h / 2, 0.001, 0, 1, 0.01, 0, 0, 0, 0], np.float64)
    singular = np.array([0, 0, w / 2, 0, h / 4, h / 2, 0, 0, 1, 0.01, 0, 0, 0, 0], np.float64)
    for params in (skew, bottom, singular):
        assert lib.cimbar_hip_undistort_batch_fmt(ctx, p(rgb), w, h, 3, 1, D.MEM_HOST, p(params), p(out), D.MEM_HOST, p(ok), p(k1), None) == -1
    assert lib.cimbar_hip_undistort_batch_fmt(ctx, p(rgb), w, h, 3, 0, D.MEM_HOST, None, p(out), D.MEM_HOST, p(ok), p(k1), None) == -1
    assert lib.cimbar_hip_undistort_calibrate_fmt(ctx, p(rgb), w, h, 3, -1, D.MEM_HOST, p(ok), p(k1), None) == -1
    chunks = np.zeros((1, 12, 625), np.uint8)
    masks = np.zeros(1, np.uint32)
    assert lib.cimbar_hip_scan_undistort_extract_decode_batch_fmt(ctx, p(rgb), w, h, 3, 0, D.MEM_HOST, -1, 2, p(chunks), p(masks), None, None,
                                                                  D.MEM_HOST, None) == -1
    # the context still works afterwards
    out2, ok2, _ = hip_decoder.undistort_batch(rgb[None])
    assert (out2[0] == capture("barrel_odd")[1][0]).all()
