"""GPU: libcimbar_recv_hip.so's cimbard_hip_scan_extract_decode_auto (include/cimbar_recv_hip_auto.h), one capture per call, against the
reference's own loop over the web receiver's candidates [66, 68, 67, 4] (cimbard_configure_decode + cimbard_scan_extract_decode on one
thread, oracle/_ref) and the sequential model."""
import ctypes
import os

import numpy as np
import pytest

from oracle.pyref import P
from tests import automode_model as AM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEB = [66, 68, 67, 4]


def test_auto_call_equals_the_web_receivers_loop(ref):
    lib = ctypes.CDLL(os.path.join(ROOT, "libcimbar_amd", "libcimbar_recv_hip.so"))
    caps = [AM.capture(m, 900 + k) for k, m in enumerate([67, 68, 0, 4, 66, 68])]
    buf = np.zeros(7500, np.uint8)
    rbuf = np.zeros(8750, np.uint8)
    mode = ctypes.c_int(-1)
    ref.ref_reset_ccm()
    for k, cam in enumerate(caps):
        img = np.ascontiguousarray(cam)
        r = lib.cimbard_hip_scan_extract_decode_auto(P(img), 1920, 1080, 3, P(buf), buf.size, ctypes.byref(mode))
        want_r, want_m = 0, 0
        for m in WEB:
            ref.cimbard_configure_decode(m)
            rr = ref.cimbard_scan_extract_decode(P(img), 1920, 1080, 3, P(rbuf), rbuf.size)
            if rr == -3 or rr > 0:
                want_r, want_m = rr, (m if rr > 0 else 0)
                break
        assert r == want_r and (r < 0 or mode.value == want_m), (k, r, want_r, mode.value, want_m)
        if r > 0:
            assert (buf[:r] == rbuf[:r]).all(), k
    ref.ref_configure(68)
    assert lib.cimbard_hip_scan_extract_decode_auto(P(buf), 0, 1080, 3, P(buf), buf.size, ctypes.byref(mode)) == -1
    assert lib.cimbard_hip_scan_extract_decode_auto(P(buf), 1920, 1080, 3, P(buf), 7499, ctypes.byref(mode)) == -2
