"""GPU: the run rescue of the once-calls (cimbar_hip_set_once_rescue) against tests/once_rescue_model.py, against the same call with the
setting off, and against cimbar_hip_decode_batch_combined with groups_in = runs_out -- each on a second context created the same way.
Inputs: tests/once_rescue_model.py (the damaged captures of tests/group_walk_cases.py), min_agree_permille = 500, color_correction 0 or 1 so
that no capture's decode depends on what was decoded before it. tests/test_once_rescue_model.py asserts the inputs' margins on the CPU.

- The sequence (modes 68 / 67 / 66): [disc pair] tried, [clean x 2] no pass 2, [three bands] tried with the representative in the middle,
  [one disc capture] a run of one, [wiped, clean] completed by pass 2. Everything the setting must not change equals the setting-off call;
  the tried runs' rows and cells equal the combined call's, byte for byte; the tap equals the model; the disc pair's row is the payload,
  and with the setting off its mask is not full.
- The same with erasure decoding on (mode 68, color_correction 1).
- 70 disc pairs (mode 66): ranks and store slots pass the first walk step of 64.
- Outputs: device outputs over poisoned buffers, rmasks alone, rchunks alone, both NULL.
- The capture path: a damaged pair, a clean capture, a blank one, a clean one.
- Scope: the once-stream call ignores the setting; decode_batch and decode_batch_combined behind a rescue are unaffected.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import capture_formats as CF
from tests import frames as F
from tests import group_walk_cases as GW
from tests import once_rescue_model as OM
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL = -1   # CIMBAR_HIP_EINVAL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pair(mode, setup=None):
    """two contexts created the same way; the first with the rescue on"""
    on, off = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    if setup:
        setup(on)
        setup(off)
    assert on.get_once_rescue() is False
    on.set_once_rescue(True)
    assert on.get_once_rescue() is True and off.get_once_rescue() is False
    return on, off


def _members(runs):
    out = [[] for _ in range(int(max(runs)) + 1)]
    for k, r in enumerate(runs):
        if r >= 0:
            out[int(r)].append(k)
    return out


def _check_against_off_and_combined(mode, frames, on, off, cc):
    """the once-call with the setting on (`on`) against the setting-off call and the combined call on `off`; returns
    (the on-call's outputs, the off-call's outputs, which runs were tried)"""
    n = len(frames)
    got = on.decode_batch_once(frames, min_agree_permille=OM.MIN_AGREE, color_correction=cc)
    tap = on.tap_once_rescue(n)
    want = off.decode_batch_once(frames, min_agree_permille=OM.MIN_AGREE, color_correction=cc)
    with pytest.raises(D.CimbarHipError):
        off.tap_once_rescue(n)                          # the setting was off in that context's last once-call
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = got
    # what the setting leaves alone
    assert n_runs == want[0] and runs.tolist() == want[3].tolist() and roles.tolist() == want[4].tolist()
    assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want[2]] and (chunks == want[1]).all()
    (a_on, a_m), (b_on, b_m) = on.get_ccm(), off.get_ccm()
    assert a_on == b_on and (a_m == b_m).all()
    members = _members(runs)
    tried = OM.tried(mode, members, masks)
    for r, t in enumerate(tried):
        if not t:
            assert rmasks[r] == want[6][r] and (rchunks[r] == want[5][r]).all(), r
    assert not rmasks[n_runs:].any() and not rchunks[n_runs:].any()
    assert all(int(a) & int(b) == int(b) for a, b in zip(rmasks, want[6]))
    # the tried runs: the combined call's groups
    cells = on.tap_once_rescue_cells(sum(tried))
    ng, c_chunks, c_masks, groups, gchunks, gmasks = off.decode_batch_combined(frames, groups=runs, color_correction=cc)
    assert ng == n_runs and groups.tolist() == runs.tolist()
    dec = roles != RM.SKIPPED                                           # (the premise: the same per-capture decode in another order)
    assert (c_chunks[dec] == chunks[dec]).all() and (c_masks[dec] == masks[dec]).all()
    gcells = off.tap(D.TAP_GROUP_CELLS, ng)
    for i, r in enumerate(r for r, t in enumerate(tried) if t):
        assert hex(int(rmasks[r])) == hex(int(gmasks[r])), r
        assert (rchunks[r] == gchunks[r]).all(), r
        assert (cells[i] == gcells[r]).all(), r
    want_rc, want_rm = OM.run_rows(mode, n, members, chunks, masks, gchunks, gmasks)
    assert (rmasks == want_rm).all() and (rchunks == want_rc).all()
    assert tap.tolist() == OM.tap_words(mode, n, members, masks, rmasks).tolist()
    return got, want, tried


def _check_sequence(mode, on, off, cc):
    frames = OM.sequence(mode)
    got, want, tried = _check_against_off_and_combined(mode, frames, on, off, cc)
    full = on.geo.FULL_MASK
    assert got[3].tolist() == OM.SEQUENCE_RUNS and tried == OM.SEQUENCE_TRIED
    assert got[4].tolist() == [RM.REP, RM.FALLBACK, RM.REP, RM.SKIPPED, RM.FALLBACK, RM.REP, RM.FALLBACK, RM.REP, RM.REP, RM.FALLBACK]
    # the disc pair recovers with the setting on and does not with it off
    _, payload = OM.rendered(mode)
    assert got[6][0] == full and (got[5][0].reshape(-1) == payload[0]).all()
    assert want[6][0] != full
    # the run pass 2 completes is complete either way, the run of one is not
    assert got[6][4] == full and want[6][4] == full and got[6][3] != full


@pytest.mark.parametrize("mode", OM.MODES)
def test_the_sequence(mode):
    on, off = _pair(mode)
    try:
        _check_sequence(mode, on, off, 0)
    finally:
        on.close(); off.close()


def test_the_sequence_with_erasure_decoding_on():
    on, off = _pair(68, lambda d: d.set_erasure_decode(12))
    try:
        _check_sequence(68, on, off, 1)
    finally:
        on.close(); off.close()


def test_ranks_and_slots_past_one_walk_step():
    mode = 66
    frames, payload = OM.pairs(mode, 70)
    on, off = _pair(mode)
    try:
        got, want, tried = _check_against_off_and_combined(mode, frames, on, off, 0)
        assert got[0] == 70 and tried == [True] * 70
        assert (got[6][:70] == on.geo.FULL_MASK).all() and (want[6][:70] != on.geo.FULL_MASK).all()
        assert (got[5][:70].reshape(70, -1) == payload).all()
    finally:
        on.close(); off.close()


def test_outputs():
    mode, frames = 66, OM.sequence(66)
    geo = D.geometry.for_mode(mode)
    n = len(frames)
    on, off = _pair(mode)
    off.set_once_rescue(True)                           # (both with the setting on: host outputs against device outputs)
    try:
        host = off.decode_batch_once(frames, min_agree_permille=OM.MIN_AGREE, color_correction=0)
        host_tap = off.tap_once_rescue(n)
        assert host[6][0] == geo.FULL_MASK
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(frames.copy()).to(dev)
        mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        kw = dict(min_agree_permille=OM.MIN_AGREE, color_correction=0, stream=st)
        shape = (n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        for with_chunks, with_masks in ((True, True), (False, True), (True, False), (False, False)):
            chunks, masks = mk(shape, torch.uint8), mk((n,), torch.int32)
            runs, roles, n_runs = mk((n,), torch.int32), mk((n,), torch.int32), mk((1,), torch.int32)
            rchunks, rmasks = mk(shape, torch.uint8), mk((n,), torch.int32)
            rc = on.decode_batch_once_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), runs.data_ptr(), roles.data_ptr(),
                                             rchunks.data_ptr() if with_chunks else None, rmasks.data_ptr() if with_masks else None,
                                             n_runs.data_ptr(), **kw)
            torch.cuda.synchronize(dev)
            assert rc == 0 and int(n_runs.item()) == host[0]
            for got, want in zip((chunks, masks, runs, roles), host[1:5]):
                assert (got.cpu().numpy().view(want.dtype) == want).all()
            if with_chunks:
                assert (rchunks.cpu().numpy() == host[5]).all()
            else:
                assert (rchunks.cpu().numpy() == POISON).all()
            if with_masks:
                assert (rmasks.cpu().numpy().view(np.uint32) == host[6]).all()
            tap = on.tap_once_rescue(n)
            if with_chunks or with_masks:
                assert tap.tolist() == host_tap.tolist() and (tap != -1).sum() == 2
                assert on.tap_once_rescue_cells(2).shape == (2, geo.NCELLS)
            else:
                # no run row asked for: nothing is tried, the per-capture outputs are what they were
                assert (tap == -1).all() and on.tap_once_rescue_cells(0).shape == (0, geo.NCELLS)
    finally:
        on.close(); off.close()


def test_capture_path():
    mode = 66
    uniq, _ = GW.rendered(mode, kinds=("white",))
    w, h = GW.CAPTURE_SIZE
    cam = lambda f: F.camera_frame(f, width=w, height=h, quad=GW.CAPTURE_QUAD, background=96)
    clean1 = cam(uniq[3])
    cams = [cam(uniq[1]), cam(uniq[2]), clean1, np.full_like(clean1, 96), clean1]    # the blank capture splits the would-be run of frame 1
    raw = np.stack([CF.rgb_to_format(c, 3) for c in cams])
    n = len(raw)
    kw = dict(size=(w, h), fmt=3, preprocess=0, color_correction=0)
    on, off = _pair(mode)
    try:
        got = on.scan_extract_decode_batch_once(raw, min_agree_permille=OM.MIN_AGREE, **kw)
        tap = on.tap_once_rescue(n)
        want = off.scan_extract_decode_batch_once(raw, min_agree_permille=OM.MIN_AGREE, **kw)
        n_runs, chunks, masks, status, runs, roles, rchunks, rmasks = got
        assert runs.tolist() == [0, 0, 1, -1, 2] and n_runs == 3          # (a condition on the input: the pair's captures agree after the warp)
        for a, b in zip(got[:6], want[:6]):
            assert np.array_equal(a, b)
        assert (rmasks[1:] == want[7][1:]).all() and (rchunks[1:] == want[6][1:]).all()
        members = _members(runs)
        assert OM.tried(mode, members, masks) == [True, False, False]
        ng, c_chunks, c_masks, c_status, groups, gchunks, gmasks = off.scan_extract_decode_batch_combined(raw, groups=runs, **kw)
        assert groups.tolist() == runs.tolist() and (c_status == status).all()
        dec = roles != RM.SKIPPED
        assert (c_masks[dec] == masks[dec]).all() and (c_chunks[dec] == chunks[dec]).all()
        assert rmasks[0] == gmasks[0] and (rchunks[0] == gchunks[0]).all()
        assert (on.tap_once_rescue_cells(1)[0] == off.tap(D.TAP_GROUP_CELLS, ng)[0]).all()
        assert tap.tolist() == OM.tap_words(mode, n, members, masks, rmasks).tolist()
        assert int(rmasks[0]) & ~int(want[7][0]) != 0                      # the rescue added chunks the members' OR lacks
    finally:
        on.close(); off.close()


def test_scope():
    mode = 66
    frames = OM.sequence(mode)
    n = len(frames)
    on, off = _pair(mode)
    try:
        # the once-stream call: identical outputs with the setting on and off, and no rescue taps
        a = on.decode_batch_once_stream(frames, min_agree_permille=OM.MIN_AGREE, color_correction=0)
        b = off.decode_batch_once_stream(frames, min_agree_permille=OM.MIN_AGREE, color_correction=0)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert a[7][0] != on.geo.FULL_MASK
        with pytest.raises(D.CimbarHipError):
            on.tap_once_rescue(n)
        # plain and combined calls behind a once-call with the rescue: what a context that never ran one reports
        got = on.decode_batch_once(frames, min_agree_permille=OM.MIN_AGREE, color_correction=0)
        assert got[6][0] == on.geo.FULL_MASK
        assert all(np.array_equal(x, y) for x, y in zip(on.decode_batch(frames, color_correction=0), off.decode_batch(frames, color_correction=0)))
        x = on.decode_batch_combined(frames, min_agree_permille=GW.AGREE_3, color_correction=0)
        y = off.decode_batch_combined(frames, min_agree_permille=GW.AGREE_3, color_correction=0)
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
        assert (on.tap(D.TAP_GROUP_CELLS, x[0]) == off.tap(D.TAP_GROUP_CELLS, y[0])).all()
        # modes 4 and 8 refuse the setting, as they refuse the once-calls
        for m in (4, 8):
            d = D.HipDecoder(0, m)
            assert d._lib.cimbar_hip_set_once_rescue(d._ctx, 1) == EINVAL and d._lib.cimbar_hip_set_once_rescue(d._ctx, 0) == 0
            assert d.get_once_rescue() is False
            d.close()
    finally:
        on.close(); off.close()
