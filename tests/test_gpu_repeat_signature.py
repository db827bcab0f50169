"""GPU: the ink signature and the agreement of repeat-capture skipping (CIMBAR_HIP_TAP_REPEAT_SIG / _AGREE after
cimbar_hip_decode_batch_once) equal tests/repeat_skip_model.py exactly, in modes 68 / 67 / 66:

- on the eleven frames of tests/repeat_skip_cases.py signature_frames: clean, noise 40 / 120, shifts, rescale(+6), the cast, an all-black and
  an all-white frame (S_c = 0 resp. every cell ties: the strict comparisons decide), one bright cell on black (it ties too) and on dim gray;
  n = 11, n = 1, n = 2;
- on 70 captures in runs of three, so that one run straddles captures 63 | 64 (the walk's step): runs, roles and the run count too.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=RC.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


@pytest.fixture(scope="module")
def dec(MODE):
    d = D.HipDecoder(0, MODE)
    yield d
    d.close()


@pytest.fixture(scope="module")
def want(MODE):
    """the model's signatures of the eleven frames, computed once"""
    return RM.signatures(MODE, RC.signature_frames(MODE))


def test_taps_equal_the_model_on_eleven_frames(MODE, dec, want):
    frames = RC.signature_frames(MODE)
    n = len(frames)
    dec.decode_batch_once(frames)
    sig, agree = dec.tap_repeat_sig(n), dec.tap_repeat_agree(n)
    bad = [(k, int((sig[k] != want[k]).sum())) for k in range(n) if (sig[k] != want[k]).any()]
    assert not bad, bad
    assert agree.tolist() == RM.agreement(want).tolist()
    # black, white: every cell ties, so every signature is 0; one bright cell on black: it alone makes the totals, so it ties too
    assert not sig[7].any() and not sig[8].any() and not sig[9].any()
    # ... and on dim gray it is the one cell redder and bluer than the frame
    cell = dec.geo.NCELLS // 3
    assert np.flatnonzero(sig[10]).tolist() == [cell] and sig[10][cell] == 3


@pytest.mark.parametrize("n", [1, 2])
def test_taps_of_one_and_two_frames(MODE, dec, want, n):
    frames = RC.signature_frames(MODE)[:n]
    n_runs, _, _, runs, roles, _, _ = dec.decode_batch_once(frames)
    assert (dec.tap_repeat_sig(n) == want[:n]).all()
    assert dec.tap_repeat_agree(n).tolist() == RM.agreement(want[:n]).tolist()
    _, _, want_runs, _, list1 = RM.plan(MODE, frames, sigs=want[:n])
    assert runs.tolist() == want_runs.tolist() and n_runs == len(list1)


def test_seventy_captures_with_a_run_across_the_walks_step(MODE, dec):
    _, f = RC.clean(MODE)
    base = [(k // 3) % 5 for k in range(70)]
    frames = f[base]
    sigs5 = RM.signatures(MODE, f)
    sigs, agree, want_runs, members, list1 = RM.plan(MODE, frames, sigs=sigs5[base])
    assert want_runs[63] == want_runs[64] == want_runs[65] == 21 and len(members) == 24       # the input is what it was built as
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = dec.decode_batch_once(frames)
    assert (dec.tap_repeat_sig(70) == sigs).all()
    assert dec.tap_repeat_agree(70).tolist() == agree.tolist()
    assert n_runs == 24 and runs.tolist() == want_runs.tolist()
    # clean frames decode completely, so nothing falls back
    assert roles.tolist() == RM.roles(70, want_runs, list1, []).tolist()
    assert (masks[list1] == dec.geo.FULL_MASK).all() and not np.delete(masks, list1).any()
    want_rc, want_rm = RM.run_fill(MODE, 70, members, chunks, masks)
    assert (rmasks == want_rm).all() and (rchunks == want_rc).all()
