"""GPU: repeat-capture skipping on the capture path (cimbar_hip_scan_extract_decode_batch_once_fmt), mode 68, 1080p captures of
tests/frames.py camera_frame under two slightly different quads, in formats 3 (RGB8) and 12 (NV12):
[A q1, A q2, A q1 + noise], a blank capture, [B q1, B q2].

- The blank capture is unusable: run and role -1, mask 0, a zero slot; it separates its neighbours and splits nothing further.
- The signature and the agreement (taps) equal tests/repeat_skip_model.py on cimbar_hip_extract_batch's frames of the same captures.
- chunks, masks and status equal cimbar_hip_scan_extract_decode_batch on the model's lists, on a second context created the same way, and so
  does the carried colour matrix; rchunks / rmasks equal the model's fill.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import capture_formats as CF
from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu

MODE = 68
Q1 = ((500, 40), (1480, 70), (470, 1030), (1500, 1000))
Q2 = ((503, 42), (1478, 69), (472, 1027), (1497, 1002))


@pytest.fixture(scope="module")
def captures():
    """the six RGB captures, built once"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _, f = RC.clean(MODE)
    A, B = f[0], f[1]
    a1 = F.camera_frame(A, quad=Q1, background=30)
    caps = [a1, F.camera_frame(A, quad=Q2, background=30), F.add_noise(a1, 20, 5), np.zeros_like(a1),
            F.camera_frame(B, quad=Q1, background=30), F.camera_frame(B, quad=Q2, background=30)]
    return caps


@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path_equals_the_model_and_plain_calls(captures, fmt):
    h, w = captures[0].shape[:2]
    caps = np.stack([CF.rgb_to_format(c, fmt) for c in captures])
    n = len(caps)
    once, ref = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    # the model's plan, from the frames the extractor makes of these captures
    status, _, frames = ref.extract_batch(caps, size=(w, h), fmt=fmt)
    usable = status > 0
    assert usable.tolist() == [True, True, True, False, True, True]
    sigs, agree, want_runs, members, list1 = RM.plan(MODE, frames, usable)
    assert want_runs.tolist() == [0, 0, 0, -1, 1, 1] and list1 == [1, 4]          # (a condition on the input: the quads' frames agree)

    n_runs, chunks, masks, got_status, runs, roles, rchunks, rmasks = once.scan_extract_decode_batch_once(caps, size=(w, h), fmt=fmt)
    assert n_runs == 2 and runs.tolist() == want_runs.tolist()
    sig = once.tap_repeat_sig(n)
    assert (sig[usable] == sigs[usable]).all()
    got_agree = once.tap_repeat_agree(n)
    both = usable[:-1] & usable[1:]
    assert got_agree[both].tolist() == agree[both].tolist()

    # list 1, then list 2, as two plain calls
    want_chunks, want_masks = np.zeros_like(chunks), np.zeros_like(masks)
    _, c1, m1, s1 = ref.scan_extract_decode_batch(caps[list1], size=(w, h), fmt=fmt)
    want_chunks[list1], want_masks[list1] = c1, m1
    list2 = RM.fallback_list(MODE, members, m1)
    if list2:
        _, c2, m2, s2 = ref.scan_extract_decode_batch(caps[list2], size=(w, h), fmt=fmt)
        want_chunks[list2], want_masks[list2] = c2, m2
        assert got_status[list2].tolist() == s2.tolist()
    assert got_status.tolist() == status.tolist() and got_status[list1].tolist() == s1.tolist()
    assert roles.tolist() == RM.roles(n, want_runs, list1, list2).tolist() and roles[3] == RM.UNUSABLE
    assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want_masks]
    assert (chunks == want_chunks).all() and masks[3] == 0 and not chunks[3].any()
    (a_on, a_m), (b_on, b_m) = once.get_ccm(), ref.get_ccm()
    assert a_on == b_on and (a_m == b_m).all()
    want_rc, want_rm = RM.run_fill(MODE, n, members, want_chunks, want_masks)
    assert (rmasks == want_rm).all() and (rchunks == want_rc).all()
    # the representatives decode (else the test would say little about pass 1)
    assert (masks[list1] != 0).all()
    once.close(); ref.close()
