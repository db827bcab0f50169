"""CPU: the mode auto-detection model (tests/automode_model.py) against the reference's own loop -- what web/recv.js does in auto mode:
ref_reset_ccm once, then per capture and candidate cimbard_configure_decode(m) + cimbard_scan_extract_decode on one thread, first mode with
bytes wins, the thread's one colour-correction matrix carried across modes."""
import numpy as np
import pytest

from oracle import pyref
from oracle.pyref import P
from tests import automode_model as AM

WEB = [66, 68, 67, 4]
TRUE_MODES = [68, 67, 0, 66, 4, 68]


@pytest.fixture(scope="module")
def cams():
    return [AM.capture(m, 300 + k) for k, m in enumerate(TRUE_MODES)]


@pytest.mark.parametrize("fmt", [3, 12])
@pytest.mark.parametrize("order", ["web", "68", "last"])
def test_model_equals_the_references_loop(ref, cams, fmt, order):
    imgs = AM.to_format(cams, fmt)
    h, w = cams[0].shape[:2]
    if order == "web":
        cand = [WEB] * len(imgs)
    elif order == "68":
        cand = [[68]] * len(imgs)
    else:                                   # each capture's true mode last
        cand = [[m for m in WEB if m != t] + ([t] if t else []) for t in TRUE_MODES]
    ref.ref_reset_ccm()
    ccm = pyref.CoCcm()
    buf = np.zeros(8750, np.uint8)
    for k, img in enumerate(imgs):
        m_ref, b_ref = 0, np.zeros(0, np.uint8)
        for m in cand[k]:
            ref.cimbard_configure_decode(m)
            r = ref.cimbard_scan_extract_decode(P(np.ascontiguousarray(img)), w, h, fmt, P(buf), buf.size)
            if r == -3:
                break
            if r > 0:
                m_ref, b_ref = m, buf[:r].copy()
                break
        mode, st, chunks, mask = AM.auto_decode(np.ascontiguousarray(img), w, h, fmt, cand[k], ccm, 1, 2)
        assert mode == m_ref, (k, mode, m_ref)
        assert (AM.packed(chunks, mask, mode) == b_ref).all(), k
        if TRUE_MODES[k] == 0:
            assert mode == 0 and st == 0
        elif TRUE_MODES[k] in cand[k]:
            assert mode == TRUE_MODES[k], (k, mode)
    ref.ref_configure(68)
