"""GPU: the lens-undistortion C++ adapter (libcimbar_amd/host/Undistort.h) built with g++ against libcimbar_hip.so only and driven like the
reference's decode loop drives Undistort<SimpleCameraCalibration> -- first-call calibration, cached parameters, reset, explicit parameters, then
Extractor::extract -- against tests/undistort_model.py."""
import os
import subprocess

import numpy as np
import pytest

from libcimbar_amd import decoder
from tests import distorted_captures as DC
from tests import undistort_model as UM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_undistort_adapter(tmp_path):
    exe = tmp_path / "test_undistort_adapter"
    libdir = os.path.dirname(decoder.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "test_undistort_adapter.cpp"),
                    "-L" + libdir, "-lcimbar_hip", "-Wl,-rpath," + libdir], check=True)
    a, b, blank = DC.case("barrel_1080"), DC.case("pincushion_1080"), DC.case("blank")
    h, w = a.shape[:2]
    want_a, ok_a, k1_a = UM.undistort(a)
    want_b, ok_b, _ = UM.undistort(b)
    assert ok_a and ok_b
    want_b_cached, _, _ = UM.undistort(b, UM.naive_camera(w, h) + [k1_a, 0.0, 0.0, 0.0, 0.0])
    params = np.array(dict(DC.PARAMS)["full"](w, h), np.float64)
    want_full, _, _ = UM.undistort(b, params)
    for name, arr in (("a", a), ("b", b), ("blank", blank), ("want_a", want_a), ("want_b", want_b), ("want_b_cached", want_b_cached),
                      ("want_full", want_full)):
        np.ascontiguousarray(arr).tofile(tmp_path / (name + ".rgb"))
    params.tofile(tmp_path / "params.bin")
    res = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("OK"), res.stdout + res.stderr
