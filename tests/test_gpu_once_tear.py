"""GPU: tear skipping in the once-calls (cimbar_hip_set_once_tear_skip) against tests/once_tear_model.py, against the same call with the
setting off and against plain cimbar_hip_decode_batch calls, each on a further context created the same way. Inputs: tests/once_tear_cases.py,
whose margins and plans tests/test_once_tear_model.py asserts on the CPU.

- Both sequences in modes 68 / 67 / 66 on axes 0, 1 and 2: the tap equals the model evaluated on the tapped signatures, row for row; roles,
  runs_out, n_runs and the per-run rows equal the model's plan; runs_out and n_runs equal the setting-off call; list 1's and list 2's chunks
  and masks and the colour-correction carry equal two consecutive decode_batch calls on a fresh context; what deliver_chunks lets through
  from the per-run rows is the same set with the setting on and off, and every delivered chunk is the payload's.
- A torn capture has mask 0 and a zeroed slot over poisoned device outputs; the guard's case is decoded in pass 2.
- With run rescue on as well, the rescue's tap and every row but the torn captures' equal those of a context with the rescue alone.
- The setting switched off again: the outputs of a context that never had it on.
- EINVAL for every out-of-range argument and in modes 4 / 8; the once-stream call ignores the setting.
- The capture path: [A, A, cut(A, B), B, B] photographed at 1080p, formats 3 and 12.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import frames as F
from tests import once_tear_cases as TC
from tests import once_tear_model as TM
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL = -1   # CIMBAR_HIP_EINVAL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _contexts(mode, k, setup=None):
    out = [D.HipDecoder(0, mode) for _ in range(k)]
    for d in out:
        assert d.get_once_tear_skip() == (-1, 750, 2)
        if setup:
            setup(d)
    return out


def _model(mode, on, n, axis, **kw):
    """the model's records and plan on the signatures the last once-call of `on` tapped"""
    sigs = on.tap_repeat_sig(n)
    _, _, runs, members, _ = RM.plan(mode, None, sigs=sigs, **kw)
    rec = TM.records(mode, sigs, runs, members, axis)
    return sigs, runs, members, rec


def _check_plan(mode, on, got, axis):
    """tap, roles, runs and rows of one once-call against the model, the pass-1 masks taken from the call's own outputs"""
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = got
    n = len(masks)
    sigs, want_runs, members, rec = _model(mode, on, n, axis)
    assert on.tap_once_tear(n).tolist() == rec.tolist()
    assert runs.tolist() == want_runs.tolist() and n_runs == len(members)
    l1 = TM.list1(members, rec)
    l2, torn = TM.second(mode, want_runs, members, rec, {k: int(masks[k]) for k in l1})
    assert roles.tolist() == TM.roles(n, want_runs, l1, l2, torn).tolist()
    for k in range(n):
        if k not in l1 and k not in l2:
            assert masks[k] == 0 and not chunks[k].any(), k
    want_rc, want_rm = RM.run_fill(mode, n, members, chunks, masks)
    assert (rmasks == want_rm).all() and (rchunks == want_rc).all()
    for k in torn:
        assert rmasks[want_runs[k]] == 0 and not rchunks[want_runs[k]].any()
    return rec, l1, l2, torn


def _check_contract(frames, on, ref, got, l1, l2):
    """list 1's, then list 2's results: two consecutive plain calls on a fresh context; the carried matrix afterwards"""
    _, chunks, masks = got[:3]
    want_chunks, want_masks = np.zeros_like(chunks), np.zeros_like(masks)
    _, c1, m1 = ref.decode_batch(frames[l1])
    want_chunks[l1], want_masks[l1] = c1, m1
    if l2:
        _, c2, m2 = ref.decode_batch(frames[l2])
        want_chunks[l2], want_masks[l2] = c2, m2
    assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want_masks]
    assert (chunks == want_chunks).all()
    (a_on, a_m), (b_on, b_m) = on.get_ccm(), ref.get_ccm()
    assert a_on == b_on and (a_m == b_m).all()


def _delivered(dec, mode, rchunks, rmasks):
    packed, _ = dec.deliver_chunks(rchunks, rmasks, dedup=True)
    return {bytes(c) for c in packed}


def _payload_chunks(mode):
    geo = D.geometry.for_mode(mode)
    payload, _ = RC.clean(mode)
    return {bytes(c) for c in np.asarray(payload).reshape(-1, geo.CHUNK)}


@pytest.mark.parametrize("seq", ["one", "two"])
@pytest.mark.parametrize("mode", TC.MODES)
def test_the_sequences_equal_the_model_the_plain_calls_and_the_setting_off(mode, seq):
    frames = TC.sequence1(mode) if seq == "one" else TC.sequence2(mode)
    main_axis = 0 if seq == "one" else 2
    on, off, ref = _contexts(mode, 3)
    try:
        on.set_once_tear_skip(main_axis)
        assert on.get_once_tear_skip() == (main_axis, 750, 2)
        got = on.decode_batch_once(frames)
        rec, l1, l2, torn = _check_plan(mode, on, got, main_axis)
        if seq == "one":
            assert got[3].tolist() == TC.SEQ1_RUNS and (l1, l2, torn) == (TC.SEQ1_LIST1, TC.SEQ1_LIST2, TC.SEQ1_TORN)
            assert got[4][8] == RM.FALLBACK and got[2][8] != 0                 # the guard's case: decoded in pass 2 (and as the plain call: below)
        else:
            assert got[3].tolist() == TC.SEQ2_RUNS and TM.candidates(rec) == [3] and torn == [3]
        _check_contract(frames, on, ref, got, l1, l2)
        # the setting off on a second context: the same runs, and the same chunks reach a sink
        want = off.decode_batch_once(frames)
        assert got[0] == want[0] and got[3].tolist() == want[3].tolist()
        assert (want[4] != TM.TORN).all() and (got[4] == TM.TORN).sum() == len(torn)
        with pytest.raises(D.CimbarHipError):
            off.tap_once_tear(len(frames))
        d_on, d_off = _delivered(on, mode, got[5], got[6]), _delivered(off, mode, want[5], want[6])
        assert d_on == d_off and d_on <= _payload_chunks(mode) and len(d_on) >= 3 * on.geo.CHUNKS_PER_FRAME
        # the other axes on the same context
        for axis in (0, 1, 2):
            if axis == main_axis:
                continue
            on.set_once_tear_skip(axis)
            rec_a, _, _, _ = _check_plan(mode, on, on.decode_batch_once(frames), axis)
            if seq == "one":
                assert TM.candidates(rec_a) == ([] if axis == 1 else sorted(TC.SEQ1_CANDIDATES))
            else:
                assert TM.candidates(rec_a) == TC.SEQ2_CANDIDATES_AXIS[axis]
    finally:
        for d in (on, off, ref):
            d.close()


def test_a_second_line_permille_and_min_side_reach_the_kernel():
    mode, frames = 66, TC.sequence1(66)
    n = len(frames)
    (on,) = _contexts(mode, 1)
    try:
        for line_permille, min_side in ((1000, 2), (600, 2), (750, 30), (750, 34)):
            on.set_once_tear_skip(0, line_permille, min_side)
            assert on.get_once_tear_skip() == (0, line_permille, min_side)
            on.decode_batch_once(frames)
            sigs, runs, members, _ = _model(mode, on, n, 0)
            want = TM.records(mode, sigs, runs, members, 0, line_permille, min_side)
            assert on.tap_once_tear(n).tolist() == want.tolist(), (line_permille, min_side)
    finally:
        on.close()


def test_device_outputs_over_poisoned_buffers():
    mode, frames = 66, TC.sequence1(66)
    geo = D.geometry.for_mode(mode)
    n = len(frames)
    on, ref = _contexts(mode, 2, lambda d: d.set_once_tear_skip(0))
    try:
        host = ref.decode_batch_once(frames)
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(frames.copy()).to(dev)
        mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
        shape = (n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        chunks, masks = mk(shape, torch.uint8), mk((n,), torch.int32)
        runs, roles, n_runs = mk((n,), torch.int32), mk((n,), torch.int32), mk((1,), torch.int32)
        rchunks, rmasks = mk(shape, torch.uint8), mk((n,), torch.int32)
        st = torch.cuda.current_stream(dev).cuda_stream
        rc = on.decode_batch_once_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), runs.data_ptr(), roles.data_ptr(), rchunks.data_ptr(),
                                         rmasks.data_ptr(), n_runs.data_ptr(), stream=st)
        torch.cuda.synchronize(dev)
        assert rc == 0 and int(n_runs.item()) == host[0] == len(set(TC.SEQ1_RUNS))
        for got, want in zip((chunks, masks, runs, roles, rchunks, rmasks), host[1:]):
            assert (got.cpu().numpy().view(want.dtype) == want).all()
        assert on.tap_once_tear(n).tolist() == ref.tap_once_tear(n).tolist()
        r, m, c = roles.cpu().numpy(), masks.cpu().numpy(), chunks.cpu().numpy()
        assert np.flatnonzero(r == TM.TORN).tolist() == TC.SEQ1_TORN
        for k in TC.SEQ1_TORN:
            assert m[k] == 0 and not c[k].any()
            assert rmasks.cpu().numpy()[TC.SEQ1_RUNS[k]] == 0 and not rchunks.cpu().numpy()[TC.SEQ1_RUNS[k]].any()
    finally:
        on.close(); ref.close()


def _second_wipe(mode, frame):
    """RC.wipe8's square moved to the upper left of the grid"""
    geo = D.geometry.for_mode(mode)
    side = int(round((0.08 * geo.DIM_X * geo.DIM_Y) ** 0.5 * geo.PITCH))
    y0, x0 = geo.OFFSET + 8 * geo.PITCH, geo.OFFSET + 8 * geo.PITCH
    return F.blank_region(frame, y0, y0 + side, x0, x0 + side)


def test_run_rescue_composes():
    mode, agree = 66, 800
    _, f = RC.clean(mode)
    A, B, C, Dd = f[0], f[1], f[2], f[3]
    pos = lambda name: TC._pos(mode, 0, name)
    frames = np.stack([A, F.add_noise(A, 40, 1), TC.SC.cut(A, B, 0, pos("midcell")), RC.wipe8(mode, B), _second_wipe(mode, B),
                       C, F.add_noise(C, 40, 2), TC.SC.cut(C, Dd, 0, pos("across")), Dd, F.add_noise(Dd, 40, 3)])
    n = len(frames)
    both, resc = _contexts(mode, 2, lambda d: d.set_once_rescue(True))
    try:
        both.set_once_tear_skip(0)
        got = both.decode_batch_once(frames, min_agree_permille=agree, color_correction=0)
        sigs, runs, members, rec = _model(mode, both, n, 0, min_agree_permille=agree)
        assert both.tap_once_tear(n).tolist() == rec.tolist()
        assert got[3].tolist() == [0, 0, 1, 2, 2, 3, 3, 4, 5, 5] and TM.candidates(rec) == [2, 7]     # (conditions on the input)
        R = RM
        # capture 2's neighbour run [3, 4] is incomplete: the guard sends it to pass 2; capture 7 is torn
        assert got[4].tolist() == [R.REP, R.SKIPPED, R.FALLBACK, R.REP, R.FALLBACK, R.REP, R.SKIPPED, TM.TORN, R.REP, R.SKIPPED]
        tap = both.tap_once_rescue(n)
        want = resc.decode_batch_once(frames, min_agree_permille=agree, color_correction=0)
        want_tap = resc.tap_once_rescue(n)
        assert tap.tolist() == want_tap.tolist() and tap[2] != -1 and (tap != -1).sum() == 1        # the damaged pair is tried, and nothing else
        assert got[0] == want[0] and got[3].tolist() == want[3].tolist()
        keep = np.arange(n) != 7
        assert (got[2][keep] == want[2][keep]).all() and (got[1][keep] == want[1][keep]).all()
        rows = np.arange(n) != 4                                                                      # run 4 is the torn capture's
        assert (got[6][rows] == want[6][rows]).all() and (got[5][rows] == want[5][rows]).all()
        assert got[6][4] == 0 and not got[5][4].any()
        assert (both.tap_once_rescue_cells(1) == resc.tap_once_rescue_cells(1)).all()
    finally:
        both.close(); resc.close()


def test_the_setting_off_again_and_the_once_stream_call():
    mode, frames = 66, TC.sequence1(66)
    n = len(frames)
    on, never = _contexts(mode, 2)
    try:
        on.set_once_tear_skip(2, 800, 3)
        # the once-stream call: the outputs of the context without the setting, and no tear tap
        a, b = on.decode_batch_once_stream(frames), never.decode_batch_once_stream(frames)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[5] != TM.TORN).all() and (a[5] == RM.REP).sum() == a[0]
        with pytest.raises(D.CimbarHipError):
            on.tap_once_tear(n)
        got = on.decode_batch_once(frames)
        assert (got[4] == TM.TORN).sum() == 2 and on.tap_once_tear(n).shape == (n, 4)
        never.decode_batch_once(frames)
        on.set_once_tear_skip(-1, 123, 45)                                  # (off: the other two are not looked at)
        assert on.get_once_tear_skip() == (-1, 750, 2)
        on.reset_ccm(); never.reset_ccm()
        a, b = on.decode_batch_once(frames), never.decode_batch_once(frames)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[4] != TM.TORN).all()
        (a_on, a_m), (b_on, b_m) = on.get_ccm(), never.get_ccm()
        assert a_on == b_on and (a_m == b_m).all()
        with pytest.raises(D.CimbarHipError):
            on.tap_once_tear(n)
    finally:
        on.close(); never.close()


def test_arguments():
    d = D.HipDecoder(0, 67)                                                 # 78 grid rows, 112 grid columns
    f = d._lib.cimbar_hip_set_once_tear_skip
    try:
        assert f(d._ctx, 1, 0, 0) == 0 and d.get_once_tear_skip() == (1, 750, 2)
        for bad in ((-2, 0, 0), (3, 0, 0), (0, 1001, 0), (0, 0, 40), (2, 0, 40), (1, 0, 57)):
            assert f(d._ctx, *bad) == EINVAL, bad
            assert d.get_once_tear_skip() == (1, 750, 2)                    # a refused call changes nothing
        assert f(d._ctx, 0, 1000, 39) == 0 and d.get_once_tear_skip() == (0, 1000, 39)
        assert f(d._ctx, 1, 1, 56) == 0 and d.get_once_tear_skip() == (1, 1, 56)
        assert f(d._ctx, 2, -7, 39) == 0 and d.get_once_tear_skip() == (2, 750, 39)
        assert d._lib.cimbar_hip_get_once_tear_skip(d._ctx, None, None, None) == 0
        assert f(d._ctx, -1, 5000, 5000) == 0 and d.get_once_tear_skip() == (-1, 750, 2)
    finally:
        d.close()
    for mode in (4, 8):
        d = D.HipDecoder(0, mode)
        f = d._lib.cimbar_hip_set_once_tear_skip
        for axis in (0, 1, 2):
            assert f(d._ctx, axis, 0, 0) == EINVAL
        assert b"68 / 67 / 66" in d._lib.cimbar_hip_last_error(d._ctx)
        assert f(d._ctx, -1, 0, 0) == 0 and d.get_once_tear_skip() == (-1, 750, 2)
        d.close()


@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path(fmt):
    mode = 68
    raw, (w, h) = TC.capture_case(fmt)
    n = len(raw)
    (on,) = _contexts(mode, 1, lambda d: d.set_once_tear_skip(0))
    try:
        n_runs, chunks, masks, status, runs, roles, rchunks, rmasks = on.scan_extract_decode_batch_once(raw, size=(w, h), fmt=fmt)
        sigs = on.tap_repeat_sig(n)
        _, _, want_runs, members, _ = RM.plan(mode, None, usable=status > 0, sigs=sigs)
        rec = TM.records(mode, sigs, want_runs, members, 0)
        assert on.tap_once_tear(n).tolist() == rec.tolist()
        assert runs.tolist() == want_runs.tolist()
        vp, vn = TM.line_permilles(mode, 0, sigs[2], sigs[1]), TM.line_permilles(mode, 0, sigs[2], sigs[3])
        tl = int(0.35 * on.geo.DIM_Y)
        lo, hi = slice(0, tl - 1), slice(tl + 2, None)                     # (the three lines around the tear apart: the warp smears it)
        print("format", fmt, "record", rec[2].tolist(), "runs", runs.tolist(), "same side min", int(min(vp[lo].min(), vn[hi].min())), "max",
              int(max(vp[lo].max(), vn[hi].max())), "other side min", int(min(vn[lo].min(), vp[hi].min())), "max", int(max(vn[lo].max(), vp[hi].max())),
              "around the tear", vp[tl - 1:tl + 2].tolist(), vn[tl - 1:tl + 2].tolist())
        assert (status > 0).all() and runs.tolist() == [0, 0, 1, 2, 2]
        assert roles.tolist() == [RM.REP, RM.SKIPPED, TM.TORN, RM.REP, RM.SKIPPED]
        assert masks[2] == 0 and not chunks[2].any() and rmasks[0] == rmasks[2] == on.geo.FULL_MASK and rmasks[1] == 0
    finally:
        on.close()
