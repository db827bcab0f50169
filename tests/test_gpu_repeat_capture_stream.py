"""GPU: repeat-capture skipping across calls on the capture path (cimbar_hip_scan_extract_decode_batch_once_stream_fmt), mode 68, formats 3
(RGB8) and 12 (NV12), on the six 1080p captures of tests/test_gpu_repeat_capture.py (rebuilt here): [A q1, A q2, A q1 + noise], a blank
capture, [B q1, B q2] -- one per call, and as the split 3 | 3.

- The blank capture is unusable: run and role -1, mask 0, a zero slot. After it the carry is unusable, and the next capture starts a run with
  continued 0.
- status, chunks and masks equal cimbar_hip_scan_extract_decode_batch on the lists of tests/repeat_stream_model.py, on a second context
  created the same way, and so does the carried colour matrix; rchunks / rmasks equal the model's cumulative fill.
- The signature and agreement taps equal the model on cimbar_hip_extract_batch's frames of the same captures (where the captures concerned
  are usable), and CIMBAR_HIP_TAP_REPEAT_CARRY equals the model's carry after every call.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import capture_formats as CF
from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM
from tests import repeat_stream_model as SM

pytestmark = pytest.mark.gpu

MODE = 68
Q1 = ((500, 40), (1480, 70), (470, 1030), (1500, 1000))
Q2 = ((503, 42), (1478, 69), (472, 1027), (1497, 1002))
WANT_RUNS = [0, 0, 0, -1, 1, 1]


@pytest.fixture(scope="module")
def captures():
    """the six RGB captures, built once"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _, f = RC.clean(MODE)
    A, B = f[0], f[1]
    a1 = F.camera_frame(A, quad=Q1, background=30)
    return [a1, F.camera_frame(A, quad=Q2, background=30), F.add_noise(a1, 20, 5), np.zeros_like(a1),
            F.camera_frame(B, quad=Q1, background=30), F.camera_frame(B, quad=Q2, background=30)]


@pytest.mark.parametrize("cuts", [(0, 1, 2, 3, 4, 5, 6), (0, 3, 6)], ids=["one per call", "3 | 3"])
@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path_across_calls_equals_the_model_and_plain_calls(captures, fmt, cuts):
    geo = D.geometry.for_mode(MODE)
    h, w = captures[0].shape[:2]
    caps = np.stack([CF.rgb_to_format(c, fmt) for c in captures])
    once, ref, aux = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    # the model's signatures, from the frames the extractor makes of these captures (a third context: extraction carries no state into a decode,
    # but the colour matrix of `ref` is part of what is compared)
    all_status, _, frames = aux.extract_batch(caps, size=(w, h), fmt=fmt)
    all_usable = all_status > 0
    assert all_usable.tolist() == [True, True, True, False, True, True]
    all_sigs = RM.signatures(MODE, frames)
    assert RM.plan(MODE, frames, all_usable, sigs=all_sigs)[2].tolist() == WANT_RUNS       # (a condition on the input: the quads' frames agree)

    carry = SM.NOTHING
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part, n, usable, tag = caps[lo:hi], hi - lo, all_usable[lo:hi], f"captures {lo}..{hi - 1}"
        pl = SM.plan(MODE, carry, None, usable, sigs=all_sigs[lo:hi])
        n_runs, continued, chunks, masks, status, runs, roles, rchunks, rmasks = once.scan_extract_decode_batch_once_stream(part, size=(w, h), fmt=fmt)
        assert runs.tolist() == pl.runs.tolist() and n_runs == len(pl.members) and continued == pl.continued, tag
        assert status.tolist() == all_status[lo:hi].tolist(), tag
        sig = once.tap_repeat_sig(n)
        assert (sig[usable] == all_sigs[lo:hi][usable]).all(), tag
        agree = once.tap_repeat_agree(n, stream=True)
        prev_usable = np.concatenate([[carry.usable], usable[:-1]])
        both = usable & prev_usable
        assert agree[both].tolist() == pl.agree[both].tolist(), tag
        if not carry.usable:
            assert agree[0] == 0, tag

        # list 1, then list 2, as two plain calls
        want_chunks, want_masks = np.zeros_like(chunks), np.zeros_like(masks)
        m1 = []
        if pl.list1:
            _, c1, m1, s1 = ref.scan_extract_decode_batch(part[pl.list1], size=(w, h), fmt=fmt)
            want_chunks[pl.list1], want_masks[pl.list1] = c1, m1
            assert status[pl.list1].tolist() == s1.tolist(), tag
        list2 = SM.fallback_list(MODE, pl, m1)
        if list2:
            _, c2, m2, s2 = ref.scan_extract_decode_batch(part[list2], size=(w, h), fmt=fmt)
            want_chunks[list2], want_masks[list2] = c2, m2
            assert status[list2].tolist() == s2.tolist(), tag
        assert roles.tolist() == SM.roles(n, pl, list2).tolist(), tag
        assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want_masks], tag
        assert (chunks == want_chunks).all(), tag
        (a_on, a_m), (b_on, b_m) = once.get_ccm(), ref.get_ccm()
        assert a_on == b_on and (a_m == b_m).all(), tag
        want_rc, want_rm = SM.run_fill(MODE, n, pl, carry, want_chunks, want_masks)
        assert (rmasks == want_rm).all() and (rchunks == want_rc).all(), tag
        # the representatives decode (else the test would say little about pass 1)
        assert (masks[pl.list1] != 0).all(), tag

        carry = SM.new_carry(n, pl, carry, usable, want_rc, want_rm)
        got_sig, got_usable, got_len, got_p = once.tap_repeat_carry()
        assert (got_usable != 0, got_len, got_p) == (carry.usable, carry.length, carry.P), tag
        if carry.usable:
            assert (got_sig == carry.sig).all(), tag
        for k in range(n):
            if lo + k == 3:
                # the blank capture: unusable, in no run, and an unusable carry behind it
                assert runs[k] == -1 and roles[k] == RM.UNUSABLE and masks[k] == 0 and not chunks[k].any(), tag
            if lo + k == 4:
                # ... so the next capture starts a run, whichever call holds it
                assert roles[k] != RM.UNUSABLE and (k > 0 or continued == 0), tag
        if hi - 1 == 3:
            assert not carry.usable and (carry.length, carry.P) == (0, 0)
    # the boundaries over the calls are the plain call's
    starts = SM.boundaries(MODE, all_sigs, list(cuts), all_usable)
    assert starts.tolist() == [True, False, False, False, True, False]
    assert carry.usable and carry.length == 2 and carry.P & ~geo.FULL_MASK == 0
    once.close(); ref.close(); aux.close()
