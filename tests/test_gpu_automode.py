"""GPU: mode auto-detection (cimbar_hip_auto_scan_extract_decode_batch_fmt / AutoDecoder) bit-exact against the sequential model
(tests/automode_model.py): accepted mode, chunks, mask, status per capture and the carried matrix after the call."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref
from tests import automode_model as AM
from tests import colour_cases as CC

pytestmark = pytest.mark.gpu

WEB = [66, 68, 67, 4]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cams():
    """mixed-mode 1080p captures: every mode, a blank one, a partly occluded mode-B one"""
    out = [AM.capture(m, 500 + k) for k, m in enumerate([68, 67, 66, 4, 8, 0, 68])]
    occl = out[-1].copy()
    occl[300:620, 700:1100] = 0
    out[-1] = occl
    return out


def check(dec, cams, fmt, cand, pre=1, cc=2, order=None, ccm=None):
    imgs = AM.to_format(cams, fmt)
    h, w = cams[0].shape[:2]
    want, ccm_after = AM.auto_batch(imgs, w, h, fmt, cand, ccm=ccm, preprocess=pre, cc=cc)
    total, slots, masks, modes, status = dec.scan_extract_decode_batch_raw(imgs, preprocess=pre, color_correction=cc, size=(w, h), fmt=fmt, order=order)
    expect_total = 0
    for f, (m, st, chunks, mask) in enumerate(want):
        assert modes[f] == m and masks[f] == mask and status[f] == st, (f, modes[f], m, masks[f], mask, status[f], st)
        fb = pyref.GEOMETRY[m][6] * pyref.GEOMETRY[m][3] if m else 0
        if m:
            assert (slots[f, :fb] == chunks.reshape(-1)).all(), f
            expect_total += bin(mask).count("1") * pyref.GEOMETRY[m][3]
        assert not slots[f, fb:].any(), f
    assert total == expect_total
    active, mat = dec.get_ccm()
    assert active == bool(ccm_after.active)
    if active:
        assert (mat.reshape(-1) == np.array(list(ccm_after.m), np.float32)).all()
    return want, ccm_after


@pytest.mark.parametrize("fmt", [3, 4, 12, 420])
def test_mixed_batch_every_format(cams, fmt):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    want, _ = check(dec, cams, fmt, WEB + [8])
    # (mode 8's eight colours do not survive 4:2:0 chroma: there the model and the device agree that nothing decodes)
    assert [w[0] for w in want][:5] == ([68, 67, 66, 4, 8] if fmt in (3, 4) else [68, 67, 66, 4, 0])


@pytest.mark.parametrize("cc", [0, 1, 2])
@pytest.mark.parametrize("pre", [1, -1])
def test_colour_correction_and_preprocess(cams, cc, pre):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    check(dec, cams, 3, WEB + [8], pre=pre, cc=cc)


@pytest.mark.parametrize("order", [[68], [8, 4, 66, 67, 68], [67, 4], [4, 66]])
def test_candidate_orders(cams, order):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    check(dec, cams, 12, order, order=order)


def test_batch_sizes_and_the_carry_across_calls(cams):
    from libcimbar_amd import AutoDecoder
    rng = np.random.default_rng(3)
    big = [cams[i] for i in rng.integers(0, len(cams), 33)]
    dec = AutoDecoder(0, WEB)
    check(dec, big[:1], 3, WEB)
    dec.reset_ccm()
    _, ccm = check(dec, big, 3, WEB)
    # two calls = one call on their concatenation: the matrix crosses the call boundary
    dec.reset_ccm()
    _, ccm1 = check(dec, big[:20], 3, WEB)
    check(dec, big[20:], 3, WEB, ccm=ccm1)
    assert dec.get_ccm()[0] == bool(ccm.active)


def test_hundreds_of_captures_on_a_caller_stream(cams):
    import ctypes
    import torch
    from libcimbar_amd import AutoDecoder
    n = 300
    idx = np.arange(n) % len(cams)
    imgs = AM.to_format(cams, 12)
    h, w = cams[0].shape[:2]
    # the model over the real sequence of 300; an attempt's result depends only on (capture, matrix carried in), so repeats are looked up
    ccm, memo, want = pyref.CoCcm(), {}, []
    for f in range(n):
        key = (int(idx[f]), bytes(ccm))
        if key not in memo:
            r = AM.auto_decode(np.ascontiguousarray(imgs[idx[f]]), w, h, 12, WEB, ccm)
            memo[key] = (r, bytes(ccm))
        r, after = memo[key]
        ctypes.memmove(ctypes.addressof(ccm), after, ctypes.sizeof(ccm))
        want.append(r)
    dec = AutoDecoder(0, WEB)
    d_in = torch.from_numpy(imgs[idx].reshape(n, -1)).cuda()
    slots = torch.zeros((n, dec.slot), dtype=torch.uint8, device="cuda")
    masks = torch.zeros(n, dtype=torch.int32, device="cuda")
    modes = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        total = dec.scan_extract_decode_device(d_in.data_ptr(), w, h, n, slots.data_ptr(), masks.data_ptr(), modes.data_ptr(), status.data_ptr(),
                                               preprocess=1, fmt=12, stream=st.cuda_stream)
    st.synchronize()
    modes, masks, status, slots = modes.cpu().numpy(), masks.cpu().numpy().view(np.uint32), status.cpu().numpy(), slots.cpu().numpy()
    for f in range(n):
        m, s, ch, mk = want[f]
        assert modes[f] == m and status[f] == s and masks[f] == mk, f
        if m:
            assert (slots[f, :ch.size] == ch.reshape(-1)).all(), f
    assert total == sum(bin(int(x)).count("1") * (pyref.GEOMETRY[int(m)][3] if m else 0) for x, m in zip(masks, modes))
    active, mat = dec.get_ccm()
    assert active == bool(ccm.active) and (not active or (mat.reshape(-1) == np.array(list(ccm.m), np.float32)).all())


@pytest.mark.parametrize("mode", [68, 67, 66, 4, 8])
def test_single_candidate_equals_the_per_mode_entry_point(cams, mode):
    from libcimbar_amd import AutoDecoder, HipDecoder
    imgs = AM.to_format(cams, 3)
    h, w = cams[0].shape[:2]
    dec = AutoDecoder(0, [mode])
    total, slots, masks, modes, status = dec.scan_extract_decode_batch_raw(imgs, preprocess=1, size=(w, h), fmt=3)
    t2, c2, m2, s2 = HipDecoder(0, mode).scan_extract_decode_batch(imgs, preprocess=1, size=(w, h), fmt=3)
    assert total == t2 and (masks == m2).all()
    fb = c2[0].size
    for f in range(len(imgs)):
        assert (slots[f, :fb] == c2[f].reshape(-1)).all(), f
        assert modes[f] == (mode if m2[f] else 0)
        assert status[f] == s2[f]


def test_the_carry_across_modes():
    """a mode-68 capture under a colour cast derives a matrix from its fountain header; a later mode-4 capture under the same cast (legacy: no
    matrix of its own, its whole result is the colour pass) decodes with that matrix in force -- and decodes nothing after reset_ccm"""
    from libcimbar_amd import AutoDecoder
    gain = np.array([0.6, 1.0, 0.45])
    c68 = AM.capture(68, 0, frame=CC.cast(AM.mode_frame(68, 700), np.eye(3), gain))
    c4 = AM.capture(4, 0, frame=CC.cast(AM.mode_frame(4, 701), np.eye(3), gain))
    dec = AutoDecoder(0, WEB)
    want, ccm = check(dec, [c68, c4], 3, WEB)
    assert ccm.active and [w[0] for w in want] == [68, 4] and want[1][3] != 0
    dec.reset_ccm()
    alone, _ = check(dec, [c4], 3, WEB)
    assert alone[0][0] == 0 and alone[0][3] == 0          # the same capture without the carried matrix: nothing
    # ... and a context per mode (no matrix crossing modes) would not have decoded it either
    from libcimbar_amd import HipDecoder
    _, _, m4, _ = HipDecoder(0, 4).scan_extract_decode_batch(c4[None], preprocess=1)
    assert m4[0] == 0


def test_convergence_from_a_wrong_guess():
    """CIMBAR_HIP_AUTO_GUESS_FIRST=1 starts the settling loop from 'every capture accepted at its first candidate': the result must be the same"""
    code = ("import sys; sys.path.insert(0, %r); from tests import test_gpu_automode as T, automode_model as AM; "
            "from libcimbar_amd import AutoDecoder; "
            "cams = [AM.capture(m, 500 + k) for k, m in enumerate([68, 67, 66, 4, 8, 0, 68])]; "
            "[T.check(AutoDecoder(0, T.WEB + [8]), cams, 3, T.WEB + [8], cc=cc) for cc in (1, 2)]; print('ok')") % ROOT
    env = dict(os.environ, CIMBAR_HIP_AUTO_GUESS_FIRST="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
