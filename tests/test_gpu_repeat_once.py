"""GPU: repeat-capture skipping on frames (cimbar_hip_decode_batch_once) against tests/repeat_skip_model.py and against plain
cimbar_hip_decode_batch calls on a second context created the same way. The inputs are those of tests/repeat_skip_cases.py, whose signature
margins tests/test_repeat_skip_model.py asserts on the CPU. Mode 68 in full, modes 67 / 66 on the first sequence.

- The sequence [A, A + noise, A + shift], [B], [torn A | C], [C, C + blur], [D x 5 variants]: runs, roles and the run count equal the model;
  per-capture chunks / masks equal two plain decode_batch calls on the model's lists (skipped captures: mask 0, zero slots) and the carried
  colour matrix is equal afterwards; rchunks / rmasks equal the model's fill. The same with erasure decoding on, and with device outputs.
- Fallback: a run of three whose representative carries the 8 % wipe: roles (2, 1, 2) and a full rmask.
- Thresholds: min_agree_permille 1000 makes every noisy capture its own run, 1 joins everything up to max_run.
- Arguments: modes 4 / 8, max_run 9, permille 1001 and a null chunks are EINVAL; NULL optional outputs are accepted.
"""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL = -1   # CIMBAR_HIP_EINVAL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pair(mode, setup=None):
    """two contexts created the same way"""
    a, b = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    if setup:
        setup(a)
        setup(b)
    return a, b


def _check_against_plain_calls(mode, frames, once, ref, got, min_agree_permille=0, max_run=0):
    """`got` = once.decode_batch_once(frames, ...) -> the model's plan, two plain calls on `ref`, and every output compared; returns roles"""
    n = len(frames)
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = got
    _, _, want_runs, members, list1 = RM.plan(mode, frames, None, min_agree_permille, max_run)
    assert runs.tolist() == want_runs.tolist() and n_runs == len(members)
    want_chunks, want_masks = np.zeros_like(chunks), np.zeros_like(masks)
    _, c1, m1 = ref.decode_batch(frames[list1])
    want_chunks[list1], want_masks[list1] = c1, m1
    list2 = RM.fallback_list(mode, members, m1)
    if list2:
        _, c2, m2 = ref.decode_batch(frames[list2])
        want_chunks[list2], want_masks[list2] = c2, m2
    assert roles.tolist() == RM.roles(n, want_runs, list1, list2).tolist()
    assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want_masks]
    assert (chunks == want_chunks).all()
    (a_on, a_m), (b_on, b_m) = once.get_ccm(), ref.get_ccm()
    assert a_on == b_on and (a_m == b_m).all()
    want_rc, want_rm = RM.run_fill(mode, n, members, want_chunks, want_masks)
    assert (rmasks == want_rm).all() and (rchunks == want_rc).all()
    return roles


@pytest.mark.parametrize("mode", RC.MODES)
def test_the_sequence_equals_the_model_and_two_plain_calls(mode):
    frames = RC.sequence(mode)
    once, ref = _pair(mode)
    got = once.decode_batch_once(frames)
    assert got[3].tolist() == RC.SEQUENCE_RUNS and got[0] == 6
    _check_against_plain_calls(mode, frames, once, ref, got)
    # a second call on the same contexts: the carried matrix of the first is part of the state both start from
    _check_against_plain_calls(mode, frames, once, ref, once.decode_batch_once(frames))
    once.close(); ref.close()


def test_the_sequence_with_erasure_decoding_on():
    frames = RC.sequence(68)
    once, ref = _pair(68, lambda d: d.set_erasure_decode(12))
    _check_against_plain_calls(68, frames, once, ref, once.decode_batch_once(frames))
    once.close(); ref.close()


def test_device_outputs_equal_host_outputs_over_poisoned_buffers():
    mode, frames = 68, RC.sequence(68)
    geo = D.geometry.for_mode(mode)
    n = len(frames)
    once, ref = _pair(mode)
    host = ref.decode_batch_once(frames)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames.copy()).to(dev)
    mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
    chunks, masks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
    runs, roles, n_runs = mk((n,), torch.int32), mk((n,), torch.int32), mk((1,), torch.int32)
    rchunks, rmasks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
    st = torch.cuda.current_stream(dev).cuda_stream
    rc = once.decode_batch_once_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), runs.data_ptr(), roles.data_ptr(), rchunks.data_ptr(),
                                       rmasks.data_ptr(), n_runs.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    assert rc == 0 and int(n_runs.item()) == host[0]
    for got, want in zip((chunks, masks, runs, roles, rchunks, rmasks), host[1:]):
        assert (got.cpu().numpy().view(want.dtype) == want).all()
    # every optional output NULL: the per-capture results alone, the same bytes
    chunks2, masks2 = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
    once.reset_ccm(); ref.reset_ccm()
    host = ref.decode_batch_once(frames)
    assert once.decode_batch_once_device(d_in.data_ptr(), n, chunks2.data_ptr(), masks2.data_ptr(), stream=st) == 0
    torch.cuda.synchronize(dev)
    assert (chunks2.cpu().numpy() == host[1]).all() and (masks2.cpu().numpy().view(np.uint32) == host[2]).all()
    once.close(); ref.close()


def test_fallback_decodes_the_rest_of_a_run_whose_representative_is_incomplete():
    mode, frames = 68, RC.fallback_run(68)
    # from the model alone: the wiped capture joined its run and is its representative (its incomplete plain decode: the CPU test, by the oracle)
    _, _, runs, members, list1 = RM.plan(mode, frames)
    assert runs.tolist() == [0, 0, 0] and list1 == [1]
    once, ref = _pair(mode)
    got = once.decode_batch_once(frames)
    roles = _check_against_plain_calls(mode, frames, once, ref, got)
    full = once.geo.FULL_MASK
    assert roles.tolist() == [RM.FALLBACK, RM.REP, RM.FALLBACK]
    assert got[2][1] != full and got[2][2] == full
    assert got[0] == 1 and got[6][0] == full and not got[6][1:].any()
    payload, _ = RC.clean(mode)
    assert (got[5][0].reshape(-1) == payload[0]).all()
    once.close(); ref.close()


def test_the_thresholds_reach_the_walk():
    mode = 68
    _, f = RC.clean(mode)
    frames = np.stack([f[0], F.add_noise(f[0], 120, 1), F.add_noise(f[0], 120, 2), F.add_noise(f[1], 120, 3)])
    # from the model alone: noise 120 changes some cell's signature, and no two frames agree in fewer than 1 permille of the cells
    assert RM.plan(mode, frames, None, 1000, 0)[2].tolist() == [0, 1, 2, 3]
    assert RM.plan(mode, frames, None, 1, 8)[2].tolist() == [0, 0, 0, 0] and RM.plan(mode, frames, None, 1, 2)[2].tolist() == [0, 0, 1, 1]
    once, ref = _pair(mode)
    # every noisy capture its own run: pass 1 decodes the input in place
    got = once.decode_batch_once(frames, min_agree_permille=1000)
    _check_against_plain_calls(mode, frames, once, ref, got, min_agree_permille=1000)
    assert got[3].tolist() == [0, 1, 2, 3] and got[4].tolist() == [RM.REP] * 4
    # 1 joins everything up to max_run
    got = once.decode_batch_once(frames, min_agree_permille=1, max_run=8)
    _check_against_plain_calls(mode, frames, once, ref, got, min_agree_permille=1, max_run=8)
    assert got[3].tolist() == [0, 0, 0, 0] and got[0] == 1
    got = once.decode_batch_once(frames, min_agree_permille=1, max_run=2)
    _check_against_plain_calls(mode, frames, once, ref, got, min_agree_permille=1, max_run=2)
    assert got[3].tolist() == [0, 0, 1, 1] and got[0] == 2
    once.close(); ref.close()


def _raw_once(dec, frames, n, min_agree, max_run, chunks_ptr, masks):
    return dec._lib.cimbar_hip_decode_batch_once(dec._ctx, frames.ctypes.data, n, D.MEM_HOST, 0, 2, min_agree, max_run, chunks_ptr, masks.ctypes.data,
                                                 None, None, None, None, None, D.MEM_HOST, None)


def test_arguments():
    geo = D.geometry.for_mode(66)
    frames = RC.sequence(66)[:2]
    dec = D.HipDecoder(0, 66)
    chunks, masks = np.zeros((2, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8), np.zeros(2, np.uint32)
    assert _raw_once(dec, frames, 2, 0, 9, chunks.ctypes.data, masks) == EINVAL
    assert _raw_once(dec, frames, 2, 1001, 0, chunks.ctypes.data, masks) == EINVAL
    assert _raw_once(dec, frames, 2, 0, 0, None, masks) == EINVAL
    assert _raw_once(dec, frames, 0, 0, 0, chunks.ctypes.data, masks) == EINVAL
    # the limits themselves, and every optional output NULL
    assert _raw_once(dec, frames, 2, 1000, 8, chunks.ctypes.data, masks) >= 1
    assert _raw_once(dec, frames, 2, 0, 0, chunks.ctypes.data, masks) == 1 and masks[0] == geo.FULL_MASK and masks[1] == 0
    dec.close()
    for mode in (4, 8):
        g = D.geometry.for_mode(mode)
        d = D.HipDecoder(0, mode)
        f = np.zeros((1, *g.FRAME_SHAPE), np.uint8)
        c, m = np.zeros((1, g.CHUNKS_PER_FRAME, g.CHUNK), np.uint8), np.zeros(1, np.uint32)
        assert _raw_once(d, f, 1, 0, 0, c.ctypes.data, m) == EINVAL
        assert b"68 / 67 / 66" in d._lib.cimbar_hip_last_error(d._ctx)
        caps = np.zeros((1, 64, 64, 3), np.uint8)
        st = np.zeros(1, np.int32)
        assert d._lib.cimbar_hip_scan_extract_decode_batch_once_fmt(d._ctx, caps.ctypes.data, 64, 64, 3, 1, D.MEM_HOST, 0, 2, 0, 0, c.ctypes.data, m.ctypes.data,
                                                                    st.ctypes.data, None, None, None, None, None, D.MEM_HOST, None) == EINVAL
        d.close()
