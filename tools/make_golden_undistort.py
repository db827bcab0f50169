"""Writes tests/golden/undistort.json from the REFERENCE's own code (build machine only, like oracle/make_golden*.py): a small harness
(tests/cpp/undistort_golden_harness.cpp) is compiled in a temporary directory against the reference's Scanner.cpp, SimpleCameraCalibration.cpp,
Extractor.cpp, Deskewer.cpp and Undistort.h over oracle/cvshim + tests/cpp/cvshim_undistort.hpp, and run on every capture of
tests/distorted_captures.py (RGB8: the CLI converts to RGB before anything else, cimbar.cpp:133). Per case: the capture's SHA-256, ok, the camera,
k1 as a hex double, the SHA-256 of the undistorted image, Extractor::extract's status, and the chunk / mask after ref_decode_fountain
(oracle/_ref, preprocess where the status says NEEDS_SHARPEN, CCM reset) on the extracted frame. Hashes only.

    python tools/make_golden_undistort.py [--ref /root/reference]
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref                          # noqa: E402
from oracle.pyref import P                        # noqa: E402
from tests import distorted_captures as DC        # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def build(ref, tmp):
    ex = os.path.join(ref, "src", "lib", "extractor")
    exe = os.path.join(tmp, "harness")
    srcs = [os.path.join(ROOT, "tests", "cpp", "undistort_golden_harness.cpp")] + [os.path.join(ex, f) for f in
                                                                                   ("Scanner.cpp", "SimpleCameraCalibration.cpp", "Extractor.cpp", "Deskewer.cpp")]
    # the flags of oracle/Makefile's reference build (-O2, literal float order)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-mssse3", "-w", "-include", os.path.join(ROOT, "tests", "cpp", "cvshim_undistort.hpp"),
                    "-I" + os.path.join(ROOT, "oracle", "cvshim"), "-I" + os.path.join(ref, "src", "lib"), "-I" + os.path.join(ref, "src", "third_party_lib"),
                    "-o", exe, *srcs], check=True)
    return exe


def run_case(exe, tmp, rgb, params=None):
    h, w = rgb.shape[:2]
    cap, und, frm = (os.path.join(tmp, n) for n in ("cap.rgb", "und.rgb", "frame.rgb"))
    np.ascontiguousarray(rgb).tofile(cap)
    args = [exe, str(w), str(h), cap, und, frm] + ([repr(float(v)) for v in params] if params is not None else [])
    out = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
    ok, k1, cam, status = int(out[0]), float.fromhex(out[1]), [float.fromhex(v) for v in out[2:11]], int(out[11])
    rec = {"capture_sha256": sha(rgb), "size": [w, h], "ok": ok, "camera": cam, "k1_hex": k1.hex(),
           "undistorted_sha256": sha(np.fromfile(und, np.uint8)), "extract_status": status}
    if status > 0:
        frame = np.fromfile(frm, np.uint8).reshape(1024, 1024, 3)
        chunks = np.zeros((12, 625), np.uint8)
        mask = ctypes.c_uint32(0)
        pyref.ref_lib().ref_decode_fountain(P(frame), 1024, 1024, 1 if status == 2 else 0, 2, 1, P(chunks), ctypes.byref(mask))
        rec["mask"] = int(mask.value)
        rec["chunks_sha256"] = sha(chunks)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("CIMBAR_REF", "/root/reference"))
    a = ap.parse_args()
    assert pyref.ref_lib() is not None, "oracle/_ref/libcimbar_ref.so is not built (__graft_entry__.build() on a machine with the reference)"
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(a.ref, tmp)
        for name, mk, _ in DC.CASES:
            cases[name] = run_case(exe, tmp, mk())
            print(name, cases[name]["ok"], cases[name]["k1_hex"], cases[name]["extract_status"], flush=True)
        rgb = DC.case("barrel_odd")
        h, w = rgb.shape[:2]
        for pname, mk in DC.PARAMS:
            cases["barrel_odd+" + pname] = run_case(exe, tmp, rgb, mk(w, h))
    out = os.path.join(ROOT, "tests", "golden", "undistort.json")
    with open(out, "w") as f:
        json.dump({"source": "reference Undistort<SimpleCameraCalibration> + Extractor over oracle/cvshim + tests/cpp/cvshim_undistort.hpp; "
                             "decode: oracle/_ref ref_decode_fountain", "cases": cases}, f, indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    main()
