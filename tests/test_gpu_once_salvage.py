"""GPU: tear salvage of the once-calls (cimbar_hip_set_once_tear_salvage) against tests/once_salvage_model.py, against the same call with
the run rescue and tear skipping alone, and against contexts that never had the setting -- each created the same way. Inputs:
tests/once_salvage_cases.py, color_correction 0 or 1 so that no capture's decode depends on what was decoded before it;
tests/test_once_salvage_model.py asserts the inputs' margins and plans on the CPU.

- S1 (modes 68 / 67 / 66): with the setting off the rows of runs 0 and 4 are not full, with it on they are the payload of A and C.
- Every call checked here: the salvage tap equals the model; the tried runs' cells equal the model's participation vote over what a second
  context tapped after plain decode_batch calls over list 1, then list 2; everything the setting must leave alone equals the setting-off
  call, byte for byte; a tried run's row is compose_row of the full members with the reported group mask, every chunk the payload's.
- The setting not effective (rescue off, tear skipping off, no run row asked for) and switched off again: a context that never had it.
- The guard reaches the kernel; erasure decoding on; device outputs over poisoned buffers; EINVAL.
- One candidate serving both neighbours; a pair the rescue tries anyway plus a partial; a full run of eight, which gets none.
- The capture path: [wipe8(A), cut(A, B), B, B] photographed at 1080p, formats 3 and 12.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import once_rescue_model as OM
from tests import once_salvage_cases as SC
from tests import once_salvage_model as SM
from tests import once_tear_model as TM
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL = -1   # CIMBAR_HIP_EINVAL
NONE8 = list(SM.NO_PARTIAL) * 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _context(mode, rescue=True, line=SC.LINE, salvage=None, setup=None):
    """a context with the run rescue and tear skipping (axis 0) as given; salvage: None = never set, else (on, guard_lines)"""
    d = D.HipDecoder(0, mode)
    if setup:
        setup(d)
    assert d.get_once_tear_salvage() == (False, 1)
    if rescue:
        d.set_once_rescue(True)
    if line is not None:
        d.set_once_tear_skip(0, line)
    if salvage is not None:
        d.set_once_tear_salvage(*salvage)
        assert d.get_once_tear_salvage() == (bool(salvage[0]), SM.resolve(salvage[1]))
    return d


def _members(runs):
    out = [[] for _ in range(int(max(runs)) + 1)]
    for k, r in enumerate(runs):
        if r >= 0:
            out[int(r)].append(k)
    return out


def _tapped(aux, decode, tap_n, lists):
    """what a context taps after plain calls over list 1, then list 2: {capture: (plane, symbols, colours, drift, flood path, chunks, mask)}"""
    out = {}
    for lst in lists:
        if not lst:
            continue
        res = decode(aux, lst)
        chunks, masks = res[1], res[2]
        taps = [aux.tap(w, tap_n(lst)) for w in (D.TAP_BITPLANE, D.TAP_SYMBOLS, D.TAP_COLORS, D.TAP_DRIFT, D.TAP_FLOOD_PATH)]
        for j, k in enumerate(lst):
            out[k] = tuple(t[j].copy() for t in taps) + (chunks[j].copy(), int(masks[j]))
    return out


def _check_model(mode, n, got, on, tapped, guard, payload_of):
    """the on-call's outputs `got` = (n_runs, chunks, masks, runs, roles, rchunks, rmasks) against the model: the salvage tap, the tried runs'
    cells and rows. Returns (members, parts, tried)."""
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = got
    geo = on.geo
    rec = on.tap_once_tear(n)
    members = _members(runs)
    parts = SM.partials(mode, members, rec, roles, guard)
    tried = SM.tried(mode, members, rec, masks, parts)
    assert on.tap_once_salvage(n).tolist() == SM.tap_rows(n, members, tried, parts).tolist()
    rtap = on.tap_once_rescue(n)
    cells = on.tap_once_rescue_cells(sum(tried))
    # the premise of the cells' model: the once-call's per-capture results are those of the two plain calls
    for k, t in tapped.items():
        assert t[6] == int(masks[k]) and (t[5] == chunks[k]).all(), k
    field = lambda j: {k: t[j] for k, t in tapped.items()}
    i = 0
    for r, (m, t) in enumerate(zip(members, tried)):
        union = 0
        for k in m:
            union |= int(masks[k])
        if not t:
            assert rtap[r] == -1, r
            continue
        grp = SM.group(m, parts[r])
        mc, _, _ = SM.combine_cells(mode, field(0), field(1), field(2), field(3), field(4), grp)
        diff = np.flatnonzero(cells[i] != mc)
        assert diff.size == 0, (r, diff[:8].tolist(), cells[i][diff[:8]].tolist(), mc[diff[:8]].tolist())
        i += 1
        # the row: only the full members' masks and chunks enter it, beside what the group decode delivered
        assert int(rmasks[r]) & union == union and rtap[r] == int(rmasks[r]) & ~union, r
        if r in payload_of:
            want_row, want_mask = OM.compose_row(mode, m, chunks, masks, np.asarray(payload_of[r]).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK), int(rtap[r]))
            assert want_mask == int(rmasks[r]) and (rchunks[r] == want_row).all(), r
            have = [j for j in range(geo.CHUNKS_PER_FRAME) if (int(rmasks[r]) >> j) & 1]
            assert (rchunks[r][have] == np.asarray(payload_of[r]).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[have]).all(), r
    assert (rtap[len(members):] == -1).all()
    return members, parts, tried


def _check_unchanged(got, want, tried, on, off):
    """everything the setting leaves alone equals the call with the rescue and tear skipping alone"""
    n_runs = got[0]
    assert n_runs == want[0] and got[3].tolist() == want[3].tolist() and got[4].tolist() == want[4].tolist()
    assert (got[2] == want[2]).all() and (got[1] == want[1]).all()
    (a_on, a_m), (b_on, b_m) = on.get_ccm(), off.get_ccm()
    assert a_on == b_on and (a_m == b_m).all()
    for r, t in enumerate(tried):
        if not t:
            assert got[6][r] == want[6][r] and (got[5][r] == want[5][r]).all(), r
    assert not got[6][n_runs:].any() and not got[5][n_runs:].any()


def _run_frames(mode, frames, on, off, aux, cc, guard=1, payload_of=None, min_agree=SC.MIN_AGREE, max_run=0):
    n = len(frames)
    kw = dict(min_agree_permille=min_agree, max_run=max_run, color_correction=cc)
    got = on.decode_batch_once(frames, **kw)
    roles = got[4]
    lists = [[k for k in range(n) if roles[k] == RM.REP], [k for k in range(n) if roles[k] == RM.FALLBACK]]
    tapped = _tapped(aux, lambda d, lst: d.decode_batch(frames[lst], color_correction=cc), len, lists)
    members, parts, tried = _check_model(mode, n, got, on, tapped, guard, payload_of or {})
    want = off.decode_batch_once(frames, **kw)
    with pytest.raises(D.CimbarHipError):
        off.tap_once_salvage(n)                          # the setting was never set in that context
    assert on.tap_once_tear(n).tolist() == off.tap_once_tear(n).tolist()
    _check_unchanged(got, want, tried, on, off)
    return got, want, members, parts, tried


def _close(*ds):
    for d in ds:
        d.close()


def _payload(mode, k):
    return np.asarray(RC.clean(mode)[0][k]).reshape(-1)


def _check_s1(mode, cc, setup=None):
    on, off, aux = _context(mode, salvage=(1, -1), setup=setup), _context(mode, setup=setup), _context(mode, setup=setup)
    try:
        payload_of = {r: _payload(mode, f) for r, f in SC.S1_PAYLOAD.items()}
        got, want, members, parts, tried = _run_frames(mode, SC.s1(mode), on, off, aux, cc, payload_of=payload_of)
        full = on.geo.FULL_MASK
        assert got[3].tolist() == SC.S1_RUNS and tried == SC.S1_TRIED
        assert got[4].tolist() == [RM.REP, RM.FALLBACK, RM.REP, RM.SKIPPED, RM.FALLBACK, RM.REP, RM.REP]
        rec = on.tap_once_tear(7)
        assert (tuple(rec[1]), tuple(rec[4])) == SC.S1_RECORDS[mode]
        assert parts[0] == (None, (1, 0, 0, int(rec[1][1]) - 1)) and parts[4] == ((4, 0, int(rec[4][1]) + 1, on.geo.DIM_Y), None)
        print("mode", mode, "rmasks off", [hex(int(m)) for m in want[6][:6]], "on", [hex(int(m)) for m in got[6][:6]])
        # with the rescue and tear skipping alone the two wiped frames are lost; with the salvage they are whole
        assert want[6][0] != full and want[6][4] != full
        assert got[6][0] == full and got[6][4] == full
        assert (got[5][0].reshape(-1) == _payload(mode, 0)).all() and (got[5][4].reshape(-1) == _payload(mode, 2)).all()
    finally:
        _close(on, off, aux)


@pytest.mark.parametrize("mode", SC.MODES)
def test_s1(mode):
    _check_s1(mode, 0)


def test_s1_with_erasure_decoding_on():
    _check_s1(68, 1, setup=lambda d: d.set_erasure_decode(12))


def test_one_candidate_serves_both_neighbours():
    mode = 67
    on, off, aux = _context(mode, salvage=(1, 1)), _context(mode), _context(mode)
    try:
        payload_of = {0: _payload(mode, 0), 2: _payload(mode, 1)}
        got, want, members, parts, tried = _run_frames(mode, SC.both_sides(mode), on, off, aux, 0, payload_of=payload_of)
        assert got[3].tolist() == SC.BOTH_RUNS and tried == SC.BOTH_TRIED
        salv = on.tap_once_salvage(3)
        assert salv[0][4] == 1 and salv[2][0] == 1 and salv[1].tolist() == NONE8         # capture 1: run 0's following and run 2's preceding partial
        full = on.geo.FULL_MASK
        print("rmasks off", [hex(int(m)) for m in want[6]], "on", [hex(int(m)) for m in got[6]])
        # every wiped cell lies inside the range of the side that serves its run (asserted on the CPU), so it has a clean participant
        assert want[6][0] != full and want[6][2] != full and got[6][0] == full and got[6][2] == full
    finally:
        _close(on, off, aux)


def test_a_tried_pair_with_a_partial_behind_it():
    mode = 66
    mk = lambda salvage: _context(mode, line=SC.PAIR_LINE, salvage=salvage)
    on, off, aux = mk((1, -1)), mk(None), mk(None)
    try:
        _, payload = OM.rendered(mode)
        got, want, members, parts, tried = _run_frames(mode, SC.pair_and_partial(mode), on, off, aux, 0, payload_of={0: payload[0]}, min_agree=SC.PAIR_MIN_AGREE)
        assert got[3].tolist() == SC.PAIR_RUNS and tried == SC.PAIR_TRIED
        assert SM.group(members[0], parts[0]) == [(0, None), (1, None), (2, (0, 0, int(on.tap_once_tear(5)[2][1]) - 1))]
        assert on.tap_once_salvage(5)[0][:4].tolist() == NONE8[:4] and on.tap_once_salvage(5)[0][4] == 2
        # (the rescue alone tries this run too; no superset of its row is promised, only of the full members' OR -- _check_model)
        print("rmasks off", [hex(int(m)) for m in want[6][:3]], "on", [hex(int(m)) for m in got[6][:3]])
    finally:
        _close(on, off, aux)


def test_a_full_run_of_eight_gets_no_partial():
    mode = 66
    on, off, aux = _context(mode, salvage=(1, -1)), _context(mode), _context(mode)
    try:
        got, want, members, parts, tried = _run_frames(mode, SC.full_run(mode), on, off, aux, 0, payload_of={0: _payload(mode, 0)}, max_run=8)
        assert got[3].tolist() == SC.FULL_RUNS and tried == SC.FULL_TRIED
        assert parts[0][1] is not None and (on.tap_once_salvage(10) == np.array(NONE8)).all()
        # the same group as the rescue alone: the same row
        assert got[6][0] == want[6][0] and (got[5][0] == want[5][0]).all()
    finally:
        _close(on, off, aux)


@pytest.mark.parametrize("guard", [0, 3])
def test_the_guard_reaches_the_kernel(guard):
    mode = 66
    on, off, aux = _context(mode, salvage=(1, guard)), _context(mode), _context(mode)
    try:
        got, _, members, parts, tried = _run_frames(mode, SC.s1(mode), on, off, aux, 0, guard=guard)
        s1, s4 = SC.S1_RECORDS[mode][0][1], SC.S1_RECORDS[mode][1][1]
        salv = on.tap_once_salvage(7)
        assert salv[0].tolist() == NONE8[:4] + [1, 0, 0, s1 - guard] and salv[4].tolist() == [4, 0, s4 + guard, on.geo.DIM_Y] + NONE8[:4]
        assert tried == SC.S1_TRIED
    finally:
        _close(on, off, aux)


def test_not_effective_and_switched_off_again():
    mode = 66
    frames = SC.s1(mode)
    kw = dict(min_agree_permille=SC.MIN_AGREE, color_correction=0)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    for rescue, line in ((False, SC.LINE), (True, None), (False, None)):
        on, never = _context(mode, rescue=rescue, line=line, salvage=(1, 2)), _context(mode, rescue=rescue, line=line)
        try:
            assert same(on.decode_batch_once(frames, **kw), never.decode_batch_once(frames, **kw))
            with pytest.raises(D.CimbarHipError):
                on.tap_once_salvage(len(frames))
            if rescue:
                assert on.tap_once_rescue(len(frames)).tolist() == never.tap_once_rescue(len(frames)).tolist()
        finally:
            _close(on, never)
    on, never = _context(mode, salvage=(1, -1)), _context(mode)
    try:
        a = on.decode_batch_once(frames, **kw)
        assert a[6][0] == on.geo.FULL_MASK and on.tap_once_salvage(7)[0][4] == 1
        on.set_once_tear_salvage(False)
        assert on.get_once_tear_salvage() == (False, 1)
        b, c = on.decode_batch_once(frames, **kw), never.decode_batch_once(frames, **kw)
        assert same(b, c) and b[6][0] != on.geo.FULL_MASK
        assert on.tap_once_rescue(7).tolist() == never.tap_once_rescue(7).tolist()
        assert (on.tap_once_rescue_cells(0).shape, never.tap_once_rescue_cells(0).shape) == ((0, on.geo.NCELLS),) * 2
        with pytest.raises(D.CimbarHipError):
            on.tap_once_salvage(7)
        # the once-stream call ignores the setting, and leaves no salvage tap
        on.set_once_tear_salvage(True)
        assert same(on.decode_batch_once_stream(frames, **kw), never.decode_batch_once_stream(frames, **kw))
        with pytest.raises(D.CimbarHipError):
            on.tap_once_salvage(7)
    finally:
        _close(on, never)


def test_outputs():
    mode, frames = 66, SC.s1(66)
    geo = D.geometry.for_mode(mode)
    n = len(frames)
    on, ref = _context(mode, salvage=(1, -1)), _context(mode, salvage=(1, -1))
    try:
        host = ref.decode_batch_once(frames, min_agree_permille=SC.MIN_AGREE, color_correction=0)
        host_salv, host_tap = ref.tap_once_salvage(n), ref.tap_once_rescue(n)
        assert host[6][0] == geo.FULL_MASK and host[6][4] == geo.FULL_MASK
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(frames.copy()).to(dev)
        mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        kw = dict(min_agree_permille=SC.MIN_AGREE, color_correction=0, stream=st)
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
            assert (rchunks.cpu().numpy() == (host[5] if with_chunks else POISON)).all()
            if with_masks:
                assert (rmasks.cpu().numpy().view(np.uint32) == host[6]).all()
            if with_chunks or with_masks:
                assert on.tap_once_salvage(n).tolist() == host_salv.tolist() and on.tap_once_rescue(n).tolist() == host_tap.tolist()
            else:
                # no run row asked for: no rescue, so the setting is not effective
                with pytest.raises(D.CimbarHipError):
                    on.tap_once_salvage(n)
                assert (on.tap_once_rescue(n) == -1).all()
    finally:
        _close(on, ref)


def test_einval():
    d = D.HipDecoder(0, 66)
    try:
        lib, ctx = d._lib, d._ctx
        for on, guard in ((1, -2), (1, 17), (0, 17), (1, 1000), (0, -5)):
            assert lib.cimbar_hip_set_once_tear_salvage(ctx, on, guard) == EINVAL
            assert d.get_once_tear_salvage() == (False, 1)                 # a refused call changes nothing
        assert lib.cimbar_hip_set_once_tear_salvage(ctx, 1, 16) == 0 and d.get_once_tear_salvage() == (True, 16)
        assert lib.cimbar_hip_set_once_tear_salvage(ctx, 1, 99) == EINVAL and d.get_once_tear_salvage() == (True, 16)
        assert lib.cimbar_hip_set_once_tear_salvage(ctx, 1, 0) == 0 and d.get_once_tear_salvage() == (True, 0)
        assert lib.cimbar_hip_set_once_tear_salvage(ctx, 0, -1) == 0 and d.get_once_tear_salvage() == (False, 1)
        assert lib.cimbar_hip_get_once_tear_salvage(ctx, None, None) == 0   # each pointer may be NULL
        with pytest.raises(D.CimbarHipError):
            d.tap_once_salvage(4)                                           # no once-call yet
    finally:
        d.close()
    for m in (4, 8):
        d = D.HipDecoder(0, m)
        assert d._lib.cimbar_hip_set_once_tear_salvage(d._ctx, 1, -1) == EINVAL and d._lib.cimbar_hip_set_once_tear_salvage(d._ctx, 1, 3) == EINVAL
        assert d.get_once_tear_salvage() == (False, 1)
        assert d._lib.cimbar_hip_set_once_tear_salvage(d._ctx, 0, 3) == 0 and d.get_once_tear_salvage() == (False, 3)
        d.close()


@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path(fmt):
    mode = 68
    raw, (w, h) = SC.capture_case(fmt)
    n = len(raw)
    on, off, aux = _context(mode, salvage=(1, -1)), _context(mode), _context(mode)
    try:
        kw = dict(size=(w, h), fmt=fmt, color_correction=0)
        got = on.scan_extract_decode_batch_once(raw, **kw)
        n_runs, chunks, masks, status, runs, roles, rchunks, rmasks = got
        lists = [[k for k in range(n) if roles[k] == RM.REP], [k for k in range(n) if roles[k] == RM.FALLBACK]]
        tapped = _tapped(aux, lambda d, lst: d.scan_extract_decode_batch(raw[lst], **kw), len, lists)
        once = (n_runs, chunks, masks, runs, roles, rchunks, rmasks)
        members, parts, tried = _check_model(mode, n, once, on, tapped, 1, {})
        want = off.scan_extract_decode_batch_once(raw, **kw)
        for j in (0, 1, 2, 3, 4, 5):
            assert np.array_equal(got[j], want[j]), j
        for r, t in enumerate(tried):
            if not t:
                assert rmasks[r] == want[7][r] and (rchunks[r] == want[6][r]).all(), r
        assert all(int(a) & int(b) == int(b) for a, b in zip(rmasks, want[7]))   # a superset of the setting-off row's mask
        print("format", fmt, "runs", runs.tolist(), "roles", roles.tolist(), "record", on.tap_once_tear(n)[1].tolist(), "salvage", on.tap_once_salvage(n)[0].tolist(),
              "rmasks off", [hex(int(m)) for m in want[7][:n_runs]], "on", [hex(int(m)) for m in rmasks[:n_runs]], "complete", bool(rmasks[0] == on.geo.FULL_MASK))
        # (conditions on the input: the photographed torn capture is recognised and serves the wiped run)
        assert (status > 0).all() and runs.tolist() == [0, 1, 2, 2] and tried == [True, False, False]
        assert parts[0][1] is not None and parts[0][1][0] == 1
    finally:
        _close(on, off, aux)
