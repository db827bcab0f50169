"""GPU: torn-capture stitching across calls (cimbar_hip_decode_batch_stitched_stream / _scan_extract_decode_batch_stitched_stream_fmt,
cimbar_hip_stitch_stream_reset, CIMBAR_HIP_TAP_STITCH_CARRY) on the frames and tears of tests/stitch_cases.py, in every mode unless noted.
Every comparison is exact. Both sides of a comparison start from reset_ccm() and stitch_stream_reset().

- Split equivalence: [A, T1, T2, C] + the damaged-band batch, nine captures, on both axes, cut five ways: rows 1... of every call and row 0
  of every call behind the first are the pairs of ONE decode_batch_stitched call, byte for byte; the stream's first row is {-1, -1, -1, 0}
  with zero slots; chunks, masks and the carried matrix equal the one-shot's.
- Recovery: A, T1, T2, C one per call, both directions, both axes: the T2 call's slot 0 * 2 + direction is B's payload with the full mask,
  neither torn capture's own mask is full, every chunk in any smask is genuine, and decode_batch_stitched on the same single captures
  reports no pair.
- Model parity: tears and the n-row forms of TAP_STITCH_LINES / TAP_STITCH_CELLS equal tests/stitch_stream_model.py on the call's own
  TAP_SYMBOLS / TAP_COLORS; TAP_STITCH_CARRY is the call's last capture and EINVAL after create and after a reset.
- Parameters belong to the call that reports the row; other calls, refused calls included, leave the carry alone; a reset drops it.
- Device outputs equal host outputs over poisoned buffers, across two streams; tears may be NULL.
- Capture path (mode 68, 1080p, formats 3 and 12): recovery one capture per call, passthrough, blank captures.
- The 2n stitched slots go through deliver_chunks as they are.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import stitch_cases as SC
from tests import stitch_stream_model as SSM

pytestmark = pytest.mark.gpu

POISON = 0xA5
NONE = [-1, -1, -1, 0]
CUTS = [(1,) * 9, (2, 7), (8, 1), (3, 1, 5), (4, 5)]


@pytest.fixture(scope="module", params=SC.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


@pytest.fixture(scope="module")
def dec(MODE):
    d = D.HipDecoder(0, MODE)
    yield d
    d.close()


def _genuine(geo, schunks, smasks, payload):
    """every chunk in any smask is the payload chunk of one of the frames in that slot"""
    p = payload.reshape(len(payload), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    for slot in range(len(smasks)):
        for j in range(geo.CHUNKS_PER_FRAME):
            if (int(smasks[slot]) >> j) & 1:
                if not any((schunks[slot, j] == p[k, j]).all() for k in range(len(p))):
                    return False
            elif schunks[slot, j].any():
                return False
    return True


def _fresh(dec):
    dec.reset_ccm()
    dec.stitch_stream_reset()


def _torn(mode, axis, name="across", direction=0):
    frames, payload = SC.rendered(mode)
    p1, p2 = SC.tear_pixels(mode, axis, name)
    t1, t2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction)
    return frames, payload, t1, t2


def _same_ccm(a, b):
    return a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


_sequences = {}


def _sequence(mode, axis):
    """[A, T1, T2, C] + damaged_band_batch: candidates and non-candidates on both sides of the 3/4 rule"""
    if (mode, axis) not in _sequences:
        frames, _, t1, t2 = _torn(mode, axis)
        _sequences[(mode, axis)] = np.concatenate([np.stack([frames[0], t1, t2, frames[2]]), SC.damaged_band_batch(mode, axis)])
    return _sequences[(mode, axis)]


def _run_cut(dec, seq, cut, axis, **kw):
    """the stream calls of one cut -> per call (cand, chunks, masks, schunks, smasks, tears)"""
    assert sum(cut) == len(seq)
    out, at = [], 0
    for size in cut:
        out.append(dec.decode_batch_stitched_stream(seq[at:at + size], axis=axis, **kw))
        at += size
    return out


@pytest.mark.parametrize("axis", [0, 1])
def test_split_equivalence(MODE, dec, axis):
    geo = dec.geo
    seq = _sequence(MODE, axis)
    assert len(seq) == 9
    _fresh(dec)
    cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(seq, axis=axis)
    ccm = dec.get_ccm()
    assert cand == int((tears[:, 0] >= 0).sum()) and 0 < cand < 8       # candidates and non-candidates
    for cut in CUTS:
        _fresh(dec)
        calls = _run_cut(dec, seq, cut, axis)
        assert _same_ccm(dec.get_ccm(), ccm), cut
        at = 0
        for size, (c, ch, m, sc, sm, tr) in zip(cut, calls):
            what = (MODE, axis, cut, at)
            assert ch.shape[0] == m.shape[0] == tr.shape[0] == size and sc.shape[0] == sm.shape[0] == 2 * size
            assert (ch == chunks[at:at + size]).all() and (m == masks[at:at + size]).all(), what
            assert c == int((tr[:, 0] >= 0).sum()), what
            lo = at - 1 if at else 0        # the one-shot pair of this call's row 0 (none for the stream's first row)
            first = 0 if at else 1
            if not at:
                assert tr[0].tolist() == NONE and not sm[:2].any() and not sc[:2].any(), what
            assert (tr[first:] == tears[lo:at + size - 1]).all(), (what, tr.tolist())
            assert (sm[2 * first:] == smasks[2 * lo:2 * (at + size - 1)]).all(), what
            assert (sc[2 * first:] == schunks[2 * lo:2 * (at + size - 1)]).all(), what
            at += size


def test_recovery_one_capture_per_call(MODE, dec):
    geo = dec.geo
    for axis in (0, 1):
        for direction in (0, 1):
            for name in ("across", "midcell"):
                frames, payload, t1, t2 = _torn(MODE, axis, name, direction)
                _fresh(dec)
                calls = [dec.decode_batch_stitched_stream(f[None], axis=axis) for f in (frames[0], t1, t2, frames[2])]
                what = (MODE, axis, direction, name, [c[5].tolist() for c in calls], [[hex(int(m)) for m in c[4]] for c in calls])
                assert calls[0][5].tolist() == [NONE] and calls[0][0] == 0, what
                cand, _, _, sc, sm, tr = calls[2]
                assert cand == 1 and tr[0, 0] >= 0, what
                assert sm[direction] == geo.FULL_MASK and (sc[direction].reshape(-1) == payload[1]).all(), what
                assert calls[1][2][0] != geo.FULL_MASK and calls[2][2][0] != geo.FULL_MASK, what
                assert calls[0][2][0] == calls[3][2][0] == geo.FULL_MASK, what
                for c in calls:
                    assert _genuine(geo, c[3], c[4], payload), what
                # what the feature adds: the plain call sees no pair in a single capture
                for f in (frames[0], t1, t2, frames[2]):
                    pc, _, _, psc, psm, ptr = dec.decode_batch_stitched(f[None], axis=axis)
                    assert pc == 0 and psc.shape[0] == psm.shape[0] == ptr.shape[0] == 0


def _model_call(dec, model, batch, axis, **kw):
    """one stream call held to the model on the call's own taps; -> (tears, smasks)"""
    n = len(batch)
    cand, _, _, _, smasks, tears = dec.decode_batch_stitched_stream(batch, axis=axis, **kw)
    sym, col = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)
    want_tears, want_cnt, want_cells = model.call(sym, col, axis, kw.get("min_agree_permille", 0), kw.get("min_band", 0))
    assert tears.tolist() == want_tears.tolist()
    assert cand == int((want_tears[:, 0] >= 0).sum())
    assert (dec.tap_stitch_lines(n, axis, stream=True) == want_cnt).all()
    assert (dec.tap_stitch_cells(n, stream=True) == want_cells).all()
    csym, ccol = dec.tap_stitch_carry()
    assert (csym == sym[-1]).all() and (ccol == col[-1]).all()
    return tears, smasks


@pytest.mark.parametrize("axis", [0, 1])
def test_model_parity_on_the_devices_own_taps(MODE, axis):
    fresh = D.HipDecoder(0, MODE)
    try:
        with pytest.raises(D.CimbarHipError):
            fresh.tap_stitch_carry()                     # after create
        seq = _sequence(MODE, axis)
        for kw in ({}, dict(min_agree_permille=990, min_band=10)):
            _fresh(fresh)
            with pytest.raises(D.CimbarHipError):
                fresh.tap_stitch_carry()                 # after a reset
            model = SSM.StitchStreamModel(MODE)
            at, seen = 0, []
            for size in (3, 1, 5):
                tears, _ = _model_call(fresh, model, seq[at:at + size], axis, **kw)
                seen += tears[:, 0].tolist()
                at += size
            assert any(a >= 0 for a in seen) and any(a < 0 for a in seen[1:])
    finally:
        fresh.close()


def test_parameters_belong_to_the_reporting_call(MODE, dec):
    geo = dec.geo
    band = [SC.BAND_LO, SC.BAND_LO + 12, SC.BAND_LO + 6, 9]
    for axis in (0, 1):
        batch = SC.damaged_band_batch(MODE, axis)          # [T1, T2 with three of the twelve band lines damaged, ...]
        model = SSM.StitchStreamModel(MODE)
        _fresh(dec)
        _model_call(dec, model, batch[:1], axis)
        tears, smasks = _model_call(dec, model, batch[1:2], axis, min_band=13)
        assert tears.tolist() == [[-1, -1, -1, 9]] and not smasks.any()
        # the sequence again: the same carried capture, the default band
        model.reset()
        _fresh(dec)
        _model_call(dec, model, batch[:1], axis)
        tears, smasks = _model_call(dec, model, batch[1:2], axis)
        assert tears.tolist() == [band]       # (a candidate; what its three noise lines leave of the decode is not this test's)
        # the axis may switch: row 0 follows the call that reports it
        model.reset()
        _fresh(dec)
        _model_call(dec, model, batch[:1], 1 - axis, min_agree_permille=900, min_band=3)
        tears, _ = _model_call(dec, model, batch[1:2], axis)
        assert tears.tolist() == [band]


def _restore_ccm(dec, state):
    if state[0]:
        dec.set_ccm(state[1])
    else:
        dec.reset_ccm()


def test_other_calls_leave_the_carry_alone(MODE, dec):
    geo = dec.geo
    frames, payload, t1, t2 = _torn(MODE, 0)
    unrelated = np.stack([frames[2], frames[0], frames[1]])

    def upto_t1():
        _fresh(dec)
        dec.decode_batch_stitched_stream(frames[0][None], axis=0)
        dec.decode_batch_stitched_stream(t1[None], axis=0)

    def t2_call():
        return dec.decode_batch_stitched_stream(t2[None], axis=0)

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    upto_t1()
    want = t2_call()
    assert want[0] == 1 and want[4][0] == geo.FULL_MASK
    # other batches in between
    upto_t1()
    ccm = dec.get_ccm()
    dec.decode_batch(unrelated)
    dec.decode_batch_stitched(unrelated, axis=1)
    _restore_ccm(dec, ccm)
    assert same(t2_call(), want)
    # refused calls in between
    upto_t1()
    for bad in (dict(axis=2), dict(axis=0, min_band=geo.DIM_Y + 1)):
        with pytest.raises(D.CimbarHipError):
            dec.decode_batch_stitched_stream(unrelated, **bad)
    with pytest.raises(D.CimbarHipError):
        dec.decode_batch_stitched_stream(unrelated[:0], axis=0)
    assert same(t2_call(), want)
    # a reset in between
    upto_t1()
    dec.stitch_stream_reset()
    got = t2_call()
    assert got[0] == 0 and got[5].tolist() == [NONE] and not got[4].any() and not got[3].any()
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all()


def _device_call(dec, batch, stream, axis=0, tears=True):
    """decode_batch_stitched_stream_device over poisoned output buffers; the caller synchronises -> (rc, tensors)"""
    geo = dec.geo
    dev = torch.device("cuda", 0)
    n = len(batch)
    d_in = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
    bufs = [mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32), mk((2 * n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8),
            mk((2 * n,), torch.int32), mk((n, 4), torch.int32)]
    torch.cuda.synchronize(dev)         # the input and the poison are in place whatever stream the call takes
    rc = dec.decode_batch_stitched_stream_device(d_in.data_ptr(), n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                                 bufs[4].data_ptr() if tears else None, axis=axis, stream=stream)
    return rc, bufs + [d_in]


def _host(bufs):
    return (bufs[0].cpu().numpy(), bufs[1].cpu().numpy().view(np.uint32), bufs[2].cpu().numpy(), bufs[3].cpu().numpy().view(np.uint32),
            bufs[4].cpu().numpy())


def test_device_outputs_equal_host_outputs(MODE, dec):
    frames, _, t1, t2 = _torn(MODE, 0)
    first, second = np.stack([frames[0], t1]), np.stack([t2, frames[2], frames[2]])
    _fresh(dec)
    want = [dec.decode_batch_stitched_stream(b, axis=0) for b in (first, second)]
    assert want[0][5][0].tolist() == NONE and want[1][5][0, 0] >= 0 and want[1][5][2].tolist() == [-1, -1, -1, dec.geo.DIM_Y]
    side = torch.cuda.Stream(torch.device("cuda", 0))
    for with_tears in (True, False):
        _fresh(dec)
        rc1, b1 = _device_call(dec, first, side.cuda_stream, tears=with_tears)      # a stream of its own ...
        rc2, b2 = _device_call(dec, second, None, tears=with_tears)                 # ... then the null stream: ordered by the calls' event
        torch.cuda.synchronize()
        assert rc1 == 0 and rc2 == 0
        for got, w in ((_host(b1), want[0]), (_host(b2), want[1])):
            assert (got[0] == w[1]).all() and (got[1] == w[2]).all()
            assert (got[2] == w[3]).all() and (got[3] == w[4]).all()        # non-candidate rows: zeroes, never poison
            if with_tears:
                assert (got[4] == w[5]).all()
            else:
                assert (got[4] == -0x5A5A5A5B).all()


@pytest.mark.parametrize("fmt", SC.CAPTURE_FORMATS)
@pytest.mark.parametrize("case", SC.CAPTURE_CASES, ids=lambda c: "axis%d-dir%d-%s" % c)
def test_capture_path(case, fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    axis, direction, name = case
    geo = geometry.for_mode(68)
    _, payload = SC.rendered(68)
    caps, size = SC.capture_pairs(axis, direction, name, fmt)
    dec, ref = D.HipDecoder(0, 68), D.HipDecoder(0, 68)
    kw = dict(axis=axis, preprocess=1, size=size, fmt=fmt)
    try:
        calls = [dec.scan_extract_decode_batch_stitched_stream(caps[k:k + 1], **kw) for k in range(4)]
        what = ([c[6].tolist() for c in calls], [[hex(int(m)) for m in c[5]] for c in calls], [c[3].tolist() for c in calls])
        assert calls[0][6].tolist() == [NONE], what
        cand, _, _, _, sc, sm, tr = calls[2]
        assert cand == 1 and tr[0, 0] >= 0, what
        assert sm[direction] == geo.FULL_MASK and (sc[direction].reshape(-1) == payload[1]).all(), what
        assert calls[1][2][0] != geo.FULL_MASK and calls[2][2][0] != geo.FULL_MASK, what
        for c in calls:
            assert _genuine(geo, c[4], c[5], payload), what
        _, pc, pm, pst = ref.scan_extract_decode_batch(caps, preprocess=1, size=size, fmt=fmt)
        assert (np.concatenate([c[1] for c in calls]) == pc).all() and (np.concatenate([c[2] for c in calls]) == pm).all()
        assert (np.concatenate([c[3] for c in calls]) == pst).all() and (pst > 0).all()
        assert _same_ccm(dec.get_ccm(), ref.get_ccm())
        # a blank capture between T1 and T2, a call of its own: its row and the row behind it are no candidates
        blank = np.full_like(caps[:1], 16 if fmt == 12 else 0)
        _fresh(dec)
        dec.scan_extract_decode_batch_stitched_stream(caps[1:2], **kw)
        b = dec.scan_extract_decode_batch_stitched_stream(blank, **kw)
        assert b[3][0] <= 0 and b[0] == 0 and (b[6][0, :3] == -1).all() and not b[5].any() and not b[4].any(), (b[3].tolist(), b[6].tolist())
        t = dec.scan_extract_decode_batch_stitched_stream(caps[2:3], **kw)
        assert t[3][0] > 0 and t[0] == 0 and t[6].tolist() == [NONE] and not t[5].any() and not t[4].any(), (t[3].tolist(), t[6].tolist())
        assert (dec.tap_stitch_lines(1, axis, stream=True) == 0).all() and (dec.tap_stitch_cells(1, stream=True) == 0).all()
        # a blank capture last in a call of two
        _fresh(dec)
        two = dec.scan_extract_decode_batch_stitched_stream(np.concatenate([caps[1:2], blank]), **kw)
        assert two[3][0] > 0 and two[3][1] <= 0 and two[0] == 0 and two[6][0].tolist() == NONE and (two[6][1, :3] == -1).all(), two[6].tolist()
        t = dec.scan_extract_decode_batch_stitched_stream(caps[2:3], **kw)
        assert t[0] == 0 and t[6].tolist() == [NONE] and not t[5].any() and not t[4].any(), t[6].tolist()
        # ... and a usable one in its place is the partner
        _fresh(dec)
        dec.scan_extract_decode_batch_stitched_stream(np.concatenate([blank, caps[1:2]]), **kw)
        t = dec.scan_extract_decode_batch_stitched_stream(caps[2:3], **kw)
        assert t[0] == 1 and t[6][0, 0] >= 0, t[6].tolist()
    finally:
        dec.close()
        ref.close()


def test_stitched_slots_go_through_delivery(MODE, dec):
    geo = dec.geo
    frames, payload, t1, t2 = _torn(MODE, 0)
    _fresh(dec)
    cand, _, _, schunks, smasks, tears = dec.decode_batch_stitched_stream(np.stack([t1, t2, frames[2]]), axis=0)
    assert tears[0].tolist() == NONE and cand == 2
    packed, src = dec.deliver_chunks(schunks, smasks, dedup=True)
    p = payload.reshape(len(payload), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    for k in (1, 2):                    # B from (T1, T2), C from (T2, C): every chunk, once
        for j in range(geo.CHUNKS_PER_FRAME):
            assert int((packed == p[k, j]).all(axis=1).sum()) == 1, (MODE, k, j)
    assert len({bytes(c[:6]) for c in packed}) == len(packed)
    assert (src >= 2 * geo.CHUNKS_PER_FRAME).all()          # nothing from row 0
