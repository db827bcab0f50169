"""GPU: repeat-capture skipping across calls on frames (cimbar_hip_decode_batch_once_stream) against tests/repeat_stream_model.py and against
plain cimbar_hip_decode_batch calls on a second context created the same way. The inputs are those of tests/repeat_skip_cases.py and
tests/repeat_stream_cases.py; tests/test_repeat_stream_model.py asserts on the CPU the conditions on them that these tests rely on. Mode 68 in
full, modes 67 / 66 on the first item.

Every stream call goes through _Stream.call, which holds against the model, call by call: runs, roles, continued and the run count; the
per-capture chunks / masks against plain decode_batch calls on the model's lists in the same order (skipped captures: mask 0, zero slots); the
cumulative rchunks / rmasks; the signature and agreement taps; and CIMBAR_HIP_TAP_REPEAT_CARRY against the model's new carry.

- one capture per call over RC.sequence (12 calls), and every split of it into two calls: the carry on a run boundary, inside a run and on the
  max_run cut of the five D variants; the carried colour matrix is equal at the end
- one call after reset equals decode_batch_once in every output
- skipping and fallback through the carry; the precedence of the carried row; max_run across calls; reset; independence of other calls
- device outputs equal host outputs over poisoned buffers, with every optional output NULL as well
- ordering: two streams used in turn, host input and device outputs, equal one stream
- the walk past one 64-lane step: 130 captures behind a carried [A]
- arguments: modes 4 / 8, max_run 9, permille 1001, null chunks and n = 0 are EINVAL and leave the carry as it was
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import frames as F
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM
from tests import repeat_stream_cases as SC
from tests import repeat_stream_model as SM

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL = -1   # CIMBAR_HIP_EINVAL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _Stream:
    """a context that makes the stream calls, a second one created the same way for the plain calls, and the model's carry"""

    def __init__(self, mode):
        self.mode, self.geo = mode, D.geometry.for_mode(mode)
        self.once, self.ref = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
        self.carry = SM.NOTHING

    def reset(self):
        self.once.once_stream_reset()
        self.once.reset_ccm(); self.ref.reset_ccm()
        self.carry = SM.NOTHING

    def close(self):
        self.once.close(); self.ref.close()

    def same_ccm(self):
        (a_on, a_m), (b_on, b_m) = self.once.get_ccm(), self.ref.get_ccm()
        return a_on == b_on and (a_m == b_m).all()

    def expect(self, frames, sigs=None, **kw):
        """the model's plan for a call of `frames` behind self.carry, the plain calls on self.ref, and what the call has to report:
        (plan, chunks, masks, roles, rchunks, rmasks, new carry)"""
        n = len(frames)
        pl = SM.plan(self.mode, self.carry, frames, None, kw.get("min_agree_permille", 0), kw.get("max_run", 0), sigs=sigs)
        chunks, masks = np.zeros((n, self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), np.uint8), np.zeros(n, np.uint32)
        m1 = []
        if pl.list1:
            _, c1, m1 = self.ref.decode_batch(frames[pl.list1])
            chunks[pl.list1], masks[pl.list1] = c1, m1
        list2 = SM.fallback_list(self.mode, pl, m1)
        if list2:
            _, c2, m2 = self.ref.decode_batch(frames[list2])
            chunks[list2], masks[list2] = c2, m2
        rchunks, rmasks = SM.run_fill(self.mode, n, pl, self.carry, chunks, masks)
        return pl, chunks, masks, SM.roles(n, pl, list2), rchunks, rmasks, SM.new_carry(n, pl, self.carry, None, rchunks, rmasks)

    def hold(self, got, want, tag=""):
        """a host-output call's results against expect()'s; the taps; then the model's carry steps on"""
        n_runs, continued, chunks, masks, runs, roles, rchunks, rmasks = got
        pl, w_chunks, w_masks, w_roles, w_rchunks, w_rmasks, carry = want
        n = len(runs)
        assert runs.tolist() == pl.runs.tolist() and n_runs == len(pl.members) and continued == pl.continued, tag
        assert roles.tolist() == w_roles.tolist(), tag
        assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in w_masks], tag
        assert (chunks == w_chunks).all(), tag
        assert [hex(int(m)) for m in rmasks] == [hex(int(m)) for m in w_rmasks], tag
        assert (rchunks == w_rchunks).all(), tag
        assert (self.once.tap_repeat_sig(n) == pl.sigs).all(), tag
        assert self.once.tap_repeat_agree(n, stream=True).tolist() == pl.agree.tolist(), tag
        self.hold_carry(carry, tag)
        self.carry = carry

    def hold_carry(self, carry, tag=""):
        sig, usable, length, p = self.once.tap_repeat_carry()
        assert (sig == carry.sig).all() and (usable != 0, length, p) == (carry.usable, carry.length, carry.P), tag

    def call(self, frames, sigs=None, tag="", **kw):
        got = self.once.decode_batch_once_stream(frames, **kw)
        self.hold(got, self.expect(frames, sigs, **kw), tag)
        return got


@pytest.fixture(scope="module")
def s68():
    s = _Stream(68)
    yield s
    s.close()


@pytest.fixture(autouse=True)
def _fresh(request):
    if "s68" in request.fixturenames:
        request.getfixturevalue("s68").reset()


def _abc(mode=68):
    payload, f = RC.clean(mode)
    return payload, f[0], f[1]


@pytest.mark.parametrize("mode", RC.MODES)
def test_one_capture_per_call_over_the_sequence(mode):
    frames, sigs = RC.sequence(mode), SC.sequence_sigs(mode)
    s = _Stream(mode)
    starts, decoded = [], 0
    for k in range(len(frames)):
        got = s.call(frames[k:k + 1], sigs[k:k + 1], tag=f"call {k}")
        starts.append(got[1] == 0)
        decoded += int(got[5][0] != RM.SKIPPED)
    assert starts == (np.diff(np.array([-1] + RC.SEQUENCE_RUNS)) != 0).tolist()
    assert s.same_ccm()
    # every displayed frame but the torn one decodes in its first capture: one decode per run
    assert decoded == len(RC.SEQUENCE_LIST1)
    s.close()


def test_every_split_of_the_sequence_into_two_calls(s68):
    frames, sigs = RC.sequence(68), SC.sequence_sigs(68)
    for cut in range(1, len(frames)):
        s68.reset()
        a = s68.call(frames[:cut], sigs[:cut], tag=f"cut {cut}, call 1")
        b = s68.call(frames[cut:], sigs[cut:], tag=f"cut {cut}, call 2")
        assert a[4].tolist() == RC.SEQUENCE_RUNS[:cut]
        inside = RC.SEQUENCE_RUNS[cut] == RC.SEQUENCE_RUNS[cut - 1]
        assert b[1] == int(inside) and (b[4] + RC.SEQUENCE_RUNS[cut]).tolist() == RC.SEQUENCE_RUNS[cut:]
        assert s68.same_ccm(), cut


def test_one_call_after_reset_equals_the_plain_once_call(s68):
    frames = RC.sequence(68)
    for _ in range(2):                                    # (the second round: after a reset, with a carry to forget)
        got = s68.once.decode_batch_once_stream(frames)
        want = s68.ref.decode_batch_once(frames)
        assert got[1] == 0 and got[0] == want[0] == 6
        for g, w in zip(got[2:], want[1:]):
            assert (g == w).all()
        assert s68.same_ccm()
        s68.once.once_stream_reset()


def test_skipping_through_the_carry(s68):
    payload, A, _ = _abc()
    full = s68.geo.FULL_MASK
    a = s68.call(A[None])
    assert a[5].tolist() == [RM.REP] and a[1] == 0 and a[3][0] == full
    ccm = s68.once.get_ccm()
    for k, v in enumerate((F.add_noise(A, 40, 1), F.shift(A, 2, 1))):
        g = s68.call(v[None], tag=f"call {k + 2}")
        assert g[5].tolist() == [RM.SKIPPED] and g[1] == 1 and g[0] == 1
        assert g[3][0] == 0 and not g[2][0].any()
        assert g[7][0] == full and (g[6][0].reshape(-1) == payload[0]).all()
    after = s68.once.get_ccm()
    assert after[0] == ccm[0] and (after[1] == ccm[1]).all()
    assert s68.carry.length == 3


def test_fallback_through_the_carry(s68):
    payload, A, _ = _abc()
    full = s68.geo.FULL_MASK
    a = s68.call(RC.wipe8(68, A)[None])
    assert a[3][0] != full and a[7][0] == a[3][0]
    b = s68.call(F.add_noise(A, 40, 7)[None], tag="call 2")
    assert b[1] == 1 and b[5].tolist() == [RM.REP] and b[3][0] == full            # decoded: P is incomplete
    assert b[7][0] == full and (b[6][0].reshape(-1) == payload[0]).all()
    c = s68.call(A[None], tag="call 3")
    assert c[1] == 1 and c[5].tolist() == [RM.SKIPPED] and c[3][0] == 0 and c[7][0] == full
    assert (c[6][0].reshape(-1) == payload[0]).all()


def test_the_carried_row_comes_first(s68):
    payload, A, B = _abc()
    geo, full = s68.geo, s68.geo.FULL_MASK
    pa, pb = payload[0].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK), payload[1].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    # the 8 % wipe, and the 5 % wipe whose decode delivers some chunks and not others (the CPU test, by the oracle)
    for name, W in (("wipe8", RC.wipe8(68, A)), ("wipe5", SC.wipe5(68, A))):
        s68.reset()
        a = s68.call(W[None], tag=name, min_agree_permille=1)
        p = int(a[3][0])
        assert p != full and (name == "wipe8" or p != 0), (name, hex(p))
        b = s68.call(B[None], tag=name + ", call 2", min_agree_permille=1)
        assert b[1] == 1 and b[5].tolist() == [RM.REP] and b[3][0] == full and b[7][0] == full, name
        for j in range(geo.CHUNKS_PER_FRAME):
            assert (b[6][0, j] == (pa[j] if (p >> j) & 1 else pb[j])).all(), (name, j)
    s68.reset()
    s68.call(A[None], min_agree_permille=1)
    b = s68.call(B[None], tag="[A] | [B], call 2", min_agree_permille=1)
    assert b[1] == 1 and b[5].tolist() == [RM.SKIPPED] and b[3][0] == 0 and (b[6][0] == pa).all()


def test_max_run_counts_the_members_of_earlier_calls(s68):
    _, A, _ = _abc()
    kw = dict(min_agree_permille=1, max_run=2)
    a = s68.call(A[None], **kw)
    b = s68.call(F.add_noise(A, 40, 1)[None], tag="call 2", **kw)
    c = s68.call(F.add_noise(A, 40, 2)[None], tag="call 3", **kw)
    assert (a[1], b[1], c[1]) == (0, 1, 0)
    assert b[5].tolist() == [RM.SKIPPED] and c[5].tolist() == [RM.REP] and c[3][0] == s68.geo.FULL_MASK
    assert s68.carry.length == 1


def test_reset_forgets_the_carry(s68):
    _, A, _ = _abc()
    assert s68.call(A[None])[5].tolist() == [RM.REP]
    s68.once.once_stream_reset()
    s68.carry = SM.NOTHING
    with pytest.raises(D.CimbarHipError):
        s68.once.tap_repeat_carry()
    g = s68.call(A[None], tag="after the reset")
    assert g[1] == 0 and g[5].tolist() == [RM.REP] and g[3][0] == s68.geo.FULL_MASK


def test_other_calls_do_not_disturb_the_carry(s68):
    _, A, B = _abc()
    s68.call(A[None])
    before = s68.once.tap_repeat_carry()
    for dec in (s68.once, s68.ref):                       # (both contexts: the colour matrix they carry stays the same)
        dec.decode_batch(B[None])
        dec.decode_batch_once(RC.sequence(68)[3:6])
    after = s68.once.tap_repeat_carry()
    assert (before[0] == after[0]).all() and before[1:] == after[1:]
    g = s68.call(F.add_noise(A, 40, 1)[None], tag="call 2")
    assert g[1] == 1 and g[5].tolist() == [RM.SKIPPED]


def test_device_outputs_equal_host_outputs_over_poisoned_buffers(s68):
    frames = RC.sequence(68)
    geo, cut = s68.geo, 8                                 # (call 2 starts inside the D run: its run 0 is skipped behind a full P)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
    for optional in (True, False):
        s68.reset()
        s68.ref.once_stream_reset()
        for part in (frames[:cut], frames[cut:]):
            n = len(part)
            host = s68.ref.decode_batch_once_stream(part)
            d_in = torch.from_numpy(part.copy()).to(dev)
            chunks, masks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
            if not optional:
                assert s68.once.decode_batch_once_stream_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), stream=st) == 0
                torch.cuda.synchronize(dev)
                assert (chunks.cpu().numpy() == host[2]).all() and (masks.cpu().numpy().view(np.uint32) == host[3]).all()
                continue
            runs, roles, n_runs, cont = mk((n,), torch.int32), mk((n,), torch.int32), mk((1,), torch.int32), mk((1,), torch.int32)
            rchunks, rmasks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
            rc = s68.once.decode_batch_once_stream_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), runs.data_ptr(), roles.data_ptr(),
                                                          rchunks.data_ptr(), rmasks.data_ptr(), n_runs.data_ptr(), cont.data_ptr(), stream=st)
            torch.cuda.synchronize(dev)
            assert rc == 0 and int(n_runs.item()) == host[0] and int(cont.item()) == host[1]
            for got, want in zip((chunks, masks, runs, roles, rchunks, rmasks), host[2:]):
                assert (got.cpu().numpy().view(want.dtype) == want).all()
        a, b = s68.once.tap_repeat_carry(), s68.ref.tap_repeat_carry()
        assert (a[0] == b[0]).all() and a[1:] == b[1:] and a[2] == 1          # (the fifth D variant: the run max_run cut off)


def test_two_streams_in_turn_equal_one_stream(s68):
    """Consecutive stream calls are ordered against each other whatever their hip_stream. Host input and device outputs, one capture per call:
    every call stages its frame in the context's one staging buffer and returns with its decode (in place, out of that buffer) and its
    k_repeat_carry still enqueued, so the next call, on the other stream, has to wait before it overwrites either."""
    import ctypes
    vp = ctypes.c_void_p
    frames = RC.sequence(68)
    geo, n = s68.geo, len(RC.sequence(68))
    dev = torch.device("cuda", 0)
    fb = geo.CHUNKS_PER_FRAME * geo.CHUNK

    def run(dec, streams):
        mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
        chunks, rchunks = mk((n, fb), torch.uint8), mk((n, fb), torch.uint8)
        words = [mk((n,), torch.int32) for _ in range(6)]                 # masks, runs, roles, rmasks, n_runs, continued: one slot per call
        torch.cuda.synchronize(dev)
        for k in range(n):
            part = frames[k:k + 1]
            at = lambda t: vp(t.data_ptr() + 4 * k)
            rc = dec._lib.cimbar_hip_decode_batch_once_stream(
                dec._ctx, part.ctypes.data, 1, D.MEM_HOST, 0, 2, 0, 0, vp(chunks.data_ptr() + k * fb), at(words[0]), at(words[1]), at(words[2]),
                vp(rchunks.data_ptr() + k * fb), at(words[3]), at(words[4]), at(words[5]), D.MEM_DEVICE, vp(streams[k % len(streams)].cuda_stream))
            assert rc == 0, k
        torch.cuda.synchronize(dev)
        return [t.cpu().numpy() for t in (chunks, rchunks, *words)], dec.tap_repeat_carry()

    s68.ref.once_stream_reset()
    two, carry2 = run(s68.once, [torch.cuda.Stream(dev), torch.cuda.Stream(dev)])
    one, carry1 = run(s68.ref, [torch.cuda.Stream(dev)])
    s68.ref.once_stream_reset()
    for a, b in zip(two, one):
        assert (a == b).all()
    assert (carry2[0] == carry1[0]).all() and carry2[1:] == carry1[1:]
    assert s68.same_ccm()
    # ... and both are the sequence's runs: a call continues the run of the call before exactly inside a run
    assert two[7].tolist() == (np.diff(np.array([-1] + RC.SEQUENCE_RUNS)) == 0).astype(int).tolist()
    assert (two[2][np.array(RC.SEQUENCE_RUNS) != 2] != 0).sum() == len(RC.SEQUENCE_LIST1) - 1      # one decode per run (the torn capture aside), complete


def test_the_walk_past_one_64_lane_step(s68):
    _, A, _ = _abc()
    s68.call(A[None])
    frames, sigs = SC.long_frames(), SC.long_sigs()
    want = s68.expect(frames, sigs)
    pl, roles = want[0], want[3]
    assert pl.continued == 1 and pl.runs.tolist() == SC.long_runs().tolist()
    got = s68.once.decode_batch_once_stream(frames)
    s68.hold(got, want)
    assert got[5][:2].tolist() == [RM.SKIPPED, RM.SKIPPED]                       # run 0, behind the carried [A]'s full P
    # list 2 reaches past lane 63: the wiped A is capture 63, and its run's last member is capture 64
    assert roles[63] == RM.REP and roles[64] == RM.FALLBACK and (roles[:64] == RM.FALLBACK).any()
    assert got[0] == len(SC.long_layout()[0])


def _raw(dec, frames, n, min_agree, max_run, chunks_ptr, masks):
    return dec._lib.cimbar_hip_decode_batch_once_stream(dec._ctx, frames.ctypes.data, n, D.MEM_HOST, 0, 2, min_agree, max_run, chunks_ptr, masks.ctypes.data,
                                                        None, None, None, None, None, None, D.MEM_HOST, None)


def test_arguments():
    geo = D.geometry.for_mode(66)
    frames = RC.sequence(66)[:2]
    dec = D.HipDecoder(0, 66)
    chunks, masks = np.zeros((2, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8), np.zeros(2, np.uint32)
    # every optional output NULL; then a carry for the refused calls to leave alone
    assert _raw(dec, frames, 2, 0, 0, chunks.ctypes.data, masks) == 1 and masks[0] == geo.FULL_MASK and masks[1] == 0
    before = dec.tap_repeat_carry()
    assert before[1:] == (1, 2, geo.FULL_MASK)
    assert _raw(dec, frames, 2, 0, 9, chunks.ctypes.data, masks) == EINVAL
    assert _raw(dec, frames, 2, 1001, 0, chunks.ctypes.data, masks) == EINVAL
    assert _raw(dec, frames, 2, 0, 0, None, masks) == EINVAL
    assert _raw(dec, frames, 0, 0, 0, chunks.ctypes.data, masks) == EINVAL
    after = dec.tap_repeat_carry()
    assert (before[0] == after[0]).all() and before[1:] == after[1:]
    # the limits themselves
    assert _raw(dec, frames, 2, 1000, 8, chunks.ctypes.data, masks) >= 0
    dec.close()
    for mode in (4, 8):
        g = D.geometry.for_mode(mode)
        d = D.HipDecoder(0, mode)
        f = np.zeros((1, *g.FRAME_SHAPE), np.uint8)
        c, m = np.zeros((1, g.CHUNKS_PER_FRAME, g.CHUNK), np.uint8), np.zeros(1, np.uint32)
        assert _raw(d, f, 1, 0, 0, c.ctypes.data, m) == EINVAL
        assert b"68 / 67 / 66" in d._lib.cimbar_hip_last_error(d._ctx)
        caps = np.zeros((1, 64, 64, 3), np.uint8)
        st = np.zeros(1, np.int32)
        assert d._lib.cimbar_hip_scan_extract_decode_batch_once_stream_fmt(d._ctx, caps.ctypes.data, 64, 64, 3, 1, D.MEM_HOST, 0, 2, 0, 0, c.ctypes.data,
                                                                           m.ctypes.data, st.ctypes.data, None, None, None, None, None, None, D.MEM_HOST,
                                                                           None) == EINVAL
        with pytest.raises(D.CimbarHipError):             # nothing is carried, before and after
            d.tap_repeat_carry()
        assert d._lib.cimbar_hip_once_stream_reset(d._ctx) == 0
        d.close()
