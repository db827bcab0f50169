"""CPU: the undistortion restatement (tests/undistort_model.py) against the reference's own code (tests/golden/undistort.json, made by
tools/make_golden_undistort.py), and the C ABI's new entry points in libcimbar_hip.so."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from libcimbar_amd import decoder
from tests import distorted_captures as DC
from tests import undistort_model as UM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort.json")
SYMBOLS = ("cimbar_hip_undistort_calibrate_fmt", "cimbar_hip_undistort_batch_fmt", "cimbar_hip_scan_undistort_extract_decode_batch_fmt")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("name", [n for n, _, _ in DC.CASES])
def test_model_reproduces_golden(golden, name):
    rgb = DC.case(name)
    g = golden[name]
    assert g["capture_sha256"] == sha(rgb), "the generator no longer makes the capture the golden file was made from"
    out, ok, k1 = UM.undistort(rgb)
    assert (ok, float(k1).hex()) == (g["ok"], g["k1_hex"])
    if ok:
        h, w = rgb.shape[:2]
        assert UM.naive_camera(w, h) == g["camera"]
    assert sha(out) == g["undistorted_sha256"]


@pytest.mark.parametrize("pname", [p for p, _ in DC.PARAMS])
def test_model_reproduces_golden_with_explicit_params(golden, pname):
    rgb = DC.case("barrel_odd")
    h, w = rgb.shape[:2]
    g = golden["barrel_odd+" + pname]
    params = dict(DC.PARAMS)[pname](w, h)
    out, ok, k1 = UM.undistort(rgb, params)
    assert ok == g["ok"] == 1 and [float(v) for v in params[:9]] == g["camera"] and sha(out) == g["undistorted_sha256"]


def test_golden_covers_the_corner_cases(golden):
    assert golden["blank"]["ok"] == 0 and golden["blank"]["extract_status"] == 0                    # no anchors
    assert golden["axis_aligned"]["ok"] == 0 and golden["axis_aligned"]["extract_status"] > 0       # parallel sides: calibration fails, extraction works
    assert any(golden[n]["ok"] == 1 and golden[n]["extract_status"] > 0 for n in ("barrel_1080", "pincushion_1080"))


def test_k1_zero_with_the_naive_camera_is_a_copy():
    rgb = DC.case("barrel_odd")
    h, w = rgb.shape[:2]
    out, ok, k1 = UM.undistort(rgb, UM.naive_camera(w, h) + [0.0] * 5)
    assert ok == 1 and (out == rgb).all()


def test_border_taps_are_zero():
    rgb = DC.case("barrel_odd")
    h, w = rgb.shape[:2]
    out, _, _ = UM.undistort(rgb, dict(DC.PARAMS)["border_zeros"](w, h))
    assert (out[0, 0] == 0).all() and (out[-1, -1] == 0).all() and out[h // 2 - 40:h // 2 + 40, w // 2 - 40:w // 2 + 40].any()


def test_library_exports_the_undistort_entry_points():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    nm = shutil.which("nm") or "/usr/bin/nm"
    syms = subprocess.run([nm, "-D", "--defined-only", decoder.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for s in SYMBOLS:
        assert s in syms, s
        assert s in decoder.EXPORTS, s
