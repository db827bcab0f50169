"""GPU: what the stage in front of the anchor search produces -- the blurred gray plane, its histogram and the Otsu threshold -- read back through
CIMBAR_HIP_TAP_SCAN_GRAY / _HIST / _THRESHOLD after a call that runs the search, and held bit for bit against the oracle's co_gray_blur /
co_scan_preprocess on the cases of tests/scan_blur_cases.py: every size at which k_scan_gray_blur_rows (streaming) or k_scan_gray_blur (tiled)
starts another column block, strip, ring pass, tile or store width, every capture format through both, batches, captures that start off a
16-byte boundary, and the histograms at which k_scan_otsu's guards decide. tests/test_gpu_extract.py and tests/test_gpu_capture_formats.py see
this stage only through the binarised image, which hides a wrong gray value wherever it does not cross the threshold
(tests/test_scan_blur_cases.py shows which faults that lets through). No tolerances: the operation is integer arithmetic, and the Otsu step
is double arithmetic in one order on both sides."""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import scan_blur_cases as SB

pytestmark = pytest.mark.gpu


def hold_against_reference(dec, case, aligned=True):
    """the three taps of the search that just ran on `case`, against the oracle; returns the tapped (gray, hist, thr)"""
    _, want_gray, want_hist, want_thr = SB.reference(case.name)
    gray, hist, thr = dec.tap_scan(case.n, case.w, case.h)
    where = f"{case.name}: {SB.partition(case.w, case.h, aligned)}"
    diff = SB.differences(gray, want_gray)
    print(where, "pixels that differ:", int((gray != want_gray).sum()), "histogram bins that differ:", int((hist != want_hist).sum()),
          "thresholds:", list(thr), "want", list(want_thr))
    assert not diff, f"{where}: {int((gray != want_gray).sum())} pixels differ, first (frame, y, x, got, want): {diff}"
    own = np.stack([np.bincount(gray[k].reshape(-1), minlength=256) for k in range(case.n)])
    assert (hist == own).all(), f"{where}: histogram is not the plane's own, (frame, bin) {np.argwhere(hist != own)[:6].tolist()}: " \
                                f"got {hist[hist != own][:6].tolist()} want {own[hist != own][:6].tolist()}"
    assert (hist == want_hist).all(), where
    assert (thr == want_thr).all(), f"{where}: thresholds {list(thr)}, want {list(want_thr)}"
    return gray, hist, thr


@pytest.mark.parametrize("name", [c.name for c in SB.CASES])
def test_gray_histogram_and_threshold_match_the_oracle(hip_decoder, oracle, name):
    case = SB.BY_NAME[name]
    buf = SB.reference(name)[0]
    ok, _ = hip_decoder.undistort_calibrate(buf, size=(case.w, case.h), fmt=case.fmt)          # the cheapest call that runs the search
    assert ok.shape == (case.n,)
    gray, _, thr = hold_against_reference(hip_decoder, case)
    if name in SB.PREPROCESS_TIE:
        # the other way into the same kernels: cimbar_hip_scan_preprocess binarises its own plane in place
        binary, thr2 = hip_decoder.scan_preprocess(buf, size=(case.w, case.h), fmt=case.fmt)
        assert (thr2 == thr).all()
        assert (binary == 255 * (gray > thr[:, None, None]).astype(np.uint8)).all()


@pytest.mark.parametrize("offset", SB.MISALIGNED_OFFSETS)
def test_misaligned_device_capture_takes_the_tiled_kernel_and_gives_the_same_plane(hip_decoder, oracle, offset):
    """the capture in device memory `offset` bytes behind a 16-byte boundary: the streaming kernel's aligned loads are out, the tiled RGB kernel
    stages every row from the 16-byte piece in front of it"""
    case = SB.MISALIGNED
    buf = SB.reference(case.name)[0]
    dev = torch.device("cuda", 0)
    room = torch.zeros((buf.size + 64,), dtype=torch.uint8, device=dev)
    assert room.data_ptr() % 16 == 0
    room[offset:offset + buf.size] = torch.from_numpy(buf.reshape(-1).copy()).to(dev)
    torch.cuda.synchronize(dev)
    ok, k1 = np.zeros(case.n, np.int32), np.zeros(case.n, np.float64)
    lib = D.load_library()
    rc = lib.cimbar_hip_undistort_calibrate_fmt(hip_decoder._ctx, ctypes.c_void_p(room.data_ptr() + offset), case.w, case.h, case.fmt, case.n, D.MEM_DEVICE,
                                                ok.ctypes.data, k1.ctypes.data, None)
    assert rc == 0, lib.cimbar_hip_last_error(hip_decoder._ctx)
    hold_against_reference(hip_decoder, case, aligned=False)


def test_scan_taps_need_a_search():
    dec = D.HipDecoder(0)
    try:
        out = np.zeros(256, np.uint32)
        for what in (D.TAP_SCAN_GRAY, D.TAP_SCAN_HIST, D.TAP_SCAN_THRESHOLD):
            assert D.load_library().cimbar_hip_tap(dec._ctx, what, out.ctypes.data, out.nbytes) == -1
        dec.undistort_calibrate(np.zeros((1, 8, 8, 3), np.uint8))
        assert D.load_library().cimbar_hip_tap(dec._ctx, D.TAP_SCAN_GRAY, out.ctypes.data, 63) == -1          # buffer too small
        gray, hist, thr = dec.tap_scan(1, 8, 8)
        assert not gray.any() and hist[0, 0] == 64 and thr[0] == 0
    finally:
        dec.close()
