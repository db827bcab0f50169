"""GPU: torn-capture stitching strip by strip (cimbar_hip_set_stitch_strips, CIMBAR_HIP_TAP_STITCH_STRIPS / _STRIP_LINES) on the slanted and
blended tears of tests/stitch_strips_cases.py (tests/test_stitch_strips_model.py vets them on the CPU), in every mode unless noted. Batches
are [A, T1, T2, C]. Every comparison is exact.

- Recovery: with strips 1 the slanted pair is no candidate and its slots are zero; with strips 4 and 8 the slot of the pair's direction has
  the full mask and B's payload byte for byte; every chunk in any smask is a genuine chunk. Three parameter sets, both axes, both directions.
- Model parity: tears, both strip taps, the line tap and the stitched cells equal tests/stitch_strips_model.py applied to the device's own
  TAP_SYMBOLS / TAP_COLORS, for every S in 2..8, on a slanted batch and on a batch whose band lines are noise-damaged in some strips only
  (located and unlocated strips, a candidate and a non-candidate).
- Strips 1 is the behaviour without the setting: every output of the four stitched calls equals that of a context that never called the
  setter, on the batches of tests/stitch_cases.py (capture calls: mode 68).
- Stream: the captures one per call with strips 4 report the rows, slots and taps of one plain call over all of them; the setting may
  change between calls, and row 0 follows the call that reports it.
- Interface: device outputs over poisoned buffers equal host outputs, non-candidates write zeroes; per-capture chunks, masks and the
  carried matrix equal decode_batch's; strips 0 and 9 are refused with nothing changed; the strip taps are EINVAL after a strips-1 batch.
- Capture path (mode 68, 1080p, formats 3 and 12): the CPU-vetted slanted pairs recover B with strips 4 and 8, and are no candidate with 1.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import stitch_cases as SC
from tests import stitch_strips_cases as XC
from tests import stitch_strips_model as XM

pytestmark = pytest.mark.gpu

POISON = 0xA5


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


def _same_ccm(a, b):
    return a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


def _fresh(dec, strips):
    dec.reset_ccm()
    dec.stitch_stream_reset()
    dec.set_stitch_strips(strips)


def test_recovery_of_slanted_and_blended_tears(MODE, dec):
    geo = dec.geo
    _, payload = SC.rendered(MODE)
    for axis in (0, 1):
        for direction in (0, 1):
            for slant in XC.SLANTS:
                batch = XC.slanted_batch(MODE, axis, direction, slant)
                slot = 2 * 1 + direction
                _fresh(dec, 1)
                cand, _, masks, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=axis)
                what = (MODE, axis, direction, slant, tears.tolist(), [hex(int(m)) for m in smasks], [hex(int(m)) for m in masks])
                assert tears[1].tolist() == [-1, -1, -1, 0] and not smasks[2:4].any() and not schunks[2:4].any(), what
                assert masks[1] != geo.FULL_MASK and masks[2] != geo.FULL_MASK and masks[0] == masks[3] == geo.FULL_MASK, what
                for S in XC.STRIPS:
                    _fresh(dec, S)
                    cand, _, masks, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=axis)
                    what = (MODE, axis, direction, slant, S, tears.tolist(), [hex(int(m)) for m in smasks])
                    assert tears[1, 0] >= 0 and cand == int((tears[:, 0] >= 0).sum()) >= 1, what
                    assert smasks[slot] == geo.FULL_MASK and (schunks[slot].reshape(-1) == payload[1]).all(), what
                    assert _genuine(geo, schunks, smasks, payload), what
    dec.set_stitch_strips(1)


def _parity(dec, mode, batch, axis, S, **kw):
    n = len(batch)
    _fresh(dec, S)
    cand, _, _, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=axis, **kw)
    sym, col = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)
    want_tears, want_rec, want_cnt, want_cells = XM.stitch_batch(mode, sym, col, axis, S, kw.get("min_agree_permille", 0), kw.get("min_band", 0))
    what = (mode, axis, S, kw)
    assert tears.tolist() == want_tears.tolist(), what
    assert dec.tap_stitch_strips(n, S).tolist() == want_rec.tolist(), what
    assert (dec.tap_stitch_strip_lines(n, S, axis) == want_cnt).all(), what
    assert (dec.tap_stitch_lines(n, axis) == want_cnt.sum(axis=1)).all(), what
    assert (dec.tap(D.TAP_STITCH_CELLS, n) == want_cells).all(), what
    assert cand == int((tears[:, 0] >= 0).sum())
    for k in range(n - 1):
        if tears[k, 0] < 0:
            assert not smasks[2 * k:2 * k + 2].any() and not schunks[2 * k:2 * k + 2].any(), what
    return tears, want_rec


@pytest.mark.parametrize("axis", [0, 1])
def test_model_parity(MODE, dec, axis):
    damaged = XC.damaged_strips_batch(MODE, axis)
    slanted = XC.slanted_batch(MODE, axis, 0, XC.SLANTS[2])
    for S in range(2, 9):
        tears, rec = _parity(dec, MODE, damaged, axis, S)
        if S == 4:
            # pair 0: strip 1 is damaged past the 3/4 rule and takes strip 0's split; pair 3: one strip of four is left
            assert tears[0, 0] >= 0 and (rec[0, :, 0] >= 0).tolist() == [True, False, True, True] and rec[0, 1, 2] == rec[0, 0, 2], rec[0].tolist()
            assert tears[3, 0] == -1 and (rec[3, :, 0] >= 0).tolist() == [False, False, True, False] and (rec[3, :, 2] == -1).all(), rec[3].tolist()
        tears, rec = _parity(dec, MODE, slanted, axis, S)
    # the caller's threshold and band reach the kernel
    _parity(dec, MODE, damaged, axis, 4, min_agree_permille=990, min_band=10)
    _parity(dec, MODE, slanted, axis, 8, min_agree_permille=600, min_band=1)
    dec.set_stitch_strips(1)


def _stitched_calls(d, batch, axis, caps=None):
    """every output of the stitched calls on one context, taps included"""
    out = []
    n = len(batch)
    d.reset_ccm()
    d.stitch_stream_reset()
    out += list(d.decode_batch_stitched(batch, axis=axis))
    out += [d.tap_stitch_lines(n, axis), d.tap(D.TAP_STITCH_CELLS, n), d.get_ccm()[0], np.asarray(d.get_ccm()[1])]
    d.reset_ccm()
    for part in (batch[:2], batch[2:]):
        out += list(d.decode_batch_stitched_stream(part, axis=axis))
        out += [d.tap_stitch_lines(len(part), axis, stream=True), d.tap_stitch_cells(len(part), stream=True)]
    if caps is not None:
        raw, size, fmt = caps
        d.reset_ccm()
        d.stitch_stream_reset()
        out += list(d.scan_extract_decode_batch_stitched(raw, axis=axis, preprocess=1, size=size, fmt=fmt))
        out += [d.tap_stitch_lines(len(raw), axis), d.tap(D.TAP_STITCH_CELLS, len(raw))]
        d.reset_ccm()
        for part in (raw[:1], raw[1:]):
            out += list(d.scan_extract_decode_batch_stitched_stream(part, axis=axis, preprocess=1, size=size, fmt=fmt))
            out += [d.tap_stitch_lines(len(part), axis, stream=True), d.tap_stitch_cells(len(part), stream=True)]
    return out


def test_strips_1_is_the_behaviour_without_the_setting(MODE, dec):
    frames, _ = SC.rendered(MODE)
    never = D.HipDecoder(0, MODE)               # never calls the setter
    try:
        assert never.get_stitch_strips() == 1
        dec.set_stitch_strips(4)                # ... this one did, ran with it, and went back
        dec.decode_batch_stitched(XC.slanted_batch(MODE, 0, 0, XC.SLANTS[0]), axis=0)
        dec.set_stitch_strips(1)
        assert dec.get_stitch_strips() == 1
        cases = []
        for axis in (0, 1):
            for name in SC.TEARS:
                p1, p2 = SC.tear_pixels(MODE, axis, name)
                t1, t2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, axis)
                cases.append((axis, np.stack([frames[0], t1, t2, frames[2]]), None))
            cases.append((axis, SC.damaged_band_batch(MODE, axis), None))
        if MODE == 68:
            for (axis, direction, name), fmt in zip(SC.CAPTURE_CASES, SC.CAPTURE_FORMATS):
                raw, size = SC.capture_pairs(axis, direction, name, fmt)
                cases.append((axis, cases[0][1], (raw, size, fmt)))
        for axis, batch, caps in cases:
            got, want = _stitched_calls(dec, batch, axis, caps), _stitched_calls(never, batch, axis, caps)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (MODE, axis, k)
    finally:
        never.close()


@pytest.mark.parametrize("axis", [0, 1])
def test_stream_one_capture_per_call(MODE, dec, axis):
    geo = dec.geo
    S = 4
    seq = np.concatenate([XC.slanted_batch(MODE, axis, 0, XC.SLANTS[1]), XC.damaged_strips_batch(MODE, axis)])
    n = len(seq)
    _fresh(dec, S)
    cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(seq, axis=axis)
    rec, cnt = dec.tap_stitch_strips(n, S), dec.tap_stitch_strip_lines(n, S, axis)
    lines, cells = dec.tap_stitch_lines(n, axis), dec.tap(D.TAP_STITCH_CELLS, n)
    ccm = dec.get_ccm()
    assert 0 < cand < n - 1 and tears[1, 0] >= 0
    _fresh(dec, S)
    for k in range(n):
        c, ch, m, sc, sm, tr = dec.decode_batch_stitched_stream(seq[k:k + 1], axis=axis)
        what = (MODE, axis, k, tr.tolist())
        assert (ch[0] == chunks[k]).all() and m[0] == masks[k], what
        srec, scnt = dec.tap_stitch_strips(1, S, stream=True), dec.tap_stitch_strip_lines(1, S, axis, stream=True)
        if k == 0:
            assert tr[0].tolist() == [-1, -1, -1, 0] and not sm.any() and not sc.any() and c == 0, what
            assert srec[0].tolist() == [[-1, -1, -1, 0]] * S and not scnt.any() and not dec.tap_stitch_lines(1, axis, stream=True).any(), what
            continue
        assert tr[0].tolist() == tears[k - 1].tolist() and c == int(tears[k - 1, 0] >= 0), what
        assert (sm == smasks[2 * k - 2:2 * k]).all() and (sc == schunks[2 * k - 2:2 * k]).all(), what
        assert srec[0].tolist() == rec[k - 1].tolist() and (scnt[0] == cnt[k - 1]).all(), what
        assert (dec.tap_stitch_lines(1, axis, stream=True)[0] == lines[k - 1]).all(), what
        assert (dec.tap_stitch_cells(1, stream=True) == cells[2 * k - 2:2 * k]).all(), what
    assert _same_ccm(dec.get_ccm(), ccm)
    # the setting may change between the calls of a stream: row 0 is judged with the setting of the call that reports it
    a, t1, t2 = seq[0:1], seq[1:2], seq[2:3]
    for first, second, candidate in ((1, S, True), (S, 1, False)):
        _fresh(dec, first)
        dec.decode_batch_stitched_stream(np.concatenate([a, t1]), axis=axis)
        dec.set_stitch_strips(second)
        c, _, _, sc, sm, tr = dec.decode_batch_stitched_stream(t2, axis=axis)
        if candidate:
            assert c == 1 and tr[0].tolist() == tears[1].tolist() and (sm == smasks[2:4]).all() and (sc == schunks[2:4]).all(), tr.tolist()
        else:
            assert c == 0 and tr[0].tolist() == [-1, -1, -1, 0] and not sm.any() and not sc.any(), tr.tolist()
            with pytest.raises(D.CimbarHipError):
                dec.tap_stitch_strips(1, S, stream=True)
    dec.set_stitch_strips(1)


def _device_call(dec, batch, axis, stream_call=False, tears=True):
    """the plain or the stream stitched call with device pointers over poisoned output buffers -> (rc, chunks, masks, schunks, smasks, tears)"""
    geo = dec.geo
    dev = torch.device("cuda", 0)
    n = len(batch)
    rows = n if stream_call else n - 1
    d_in = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
    chunks, masks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
    schunks, smasks = mk((2 * rows, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((2 * rows,), torch.int32)
    d_tears = mk((rows, 4), torch.int32)
    st = torch.cuda.current_stream(dev).cuda_stream
    call = dec.decode_batch_stitched_stream_device if stream_call else dec.decode_batch_stitched_device
    rc = call(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(), d_tears.data_ptr() if tears else None,
              axis=axis, stream=st)
    torch.cuda.synchronize(dev)
    return (rc, chunks.cpu().numpy(), masks.cpu().numpy().view(np.uint32), schunks.cpu().numpy(), smasks.cpu().numpy().view(np.uint32),
            d_tears.cpu().numpy())


def test_interface(MODE, dec):
    geo = dec.geo
    S = 8
    slanted = XC.slanted_batch(MODE, 0, 0, XC.SLANTS[1])
    batch = np.concatenate([slanted, slanted[3:]])          # ... and (C, C): every strip over the whole frame, no candidate
    n = len(batch)
    ref = D.HipDecoder(0, MODE)
    try:
        _, rchunks, rmasks = ref.decode_batch(batch)
        _fresh(dec, S)
        cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=0)
        assert (chunks == rchunks).all() and (masks == rmasks).all() and _same_ccm(dec.get_ccm(), ref.get_ccm())
        assert tears[1, 0] >= 0 and tears[3].tolist() == [-1, -1, -1, S * geo.DIM_Y] and cand == int((tears[:, 0] >= 0).sum())
        assert dec.tap_stitch_strips(n, S)[3].tolist() == [[0, geo.DIM_Y, -1, geo.DIM_Y]] * S
    finally:
        ref.close()
    # device outputs over poisoned buffers == host outputs; the non-candidate's slots are written with zeroes
    _fresh(dec, S)
    rc, dchunks, dmasks, dschunks, dsmasks, dtears = _device_call(dec, batch, 0)
    assert rc == 0 and (dchunks == chunks).all() and (dmasks == masks).all() and (dtears == tears).all()
    assert (dschunks == schunks).all() and (dsmasks == smasks).all() and not dsmasks[6:8].any() and not dschunks[6:8].any()
    _fresh(dec, S)
    rc, _, _, dschunks, dsmasks, _ = _device_call(dec, batch, 0, tears=False)       # tears may be NULL
    assert rc == 0 and (dschunks == schunks).all() and (dsmasks == smasks).all()
    _fresh(dec, S)
    rc, dchunks, dmasks, dschunks, dsmasks, dtears = _device_call(dec, batch, 0, stream_call=True)
    assert rc == 0 and (dchunks == chunks).all() and (dmasks == masks).all()
    assert dtears[0].tolist() == [-1, -1, -1, 0] and not dsmasks[:2].any() and not dschunks[:2].any()
    assert (dtears[1:] == tears).all() and (dschunks[2:] == schunks).all() and (dsmasks[2:] == smasks).all()
    assert dec.tap_stitch_strips(n, S, stream=True)[0].tolist() == [[-1, -1, -1, 0]] * S
    # what the setter refuses, with nothing changed
    for bad in (0, 9, -1, 100):
        with pytest.raises(D.CimbarHipError):
            dec.set_stitch_strips(bad)
        assert dec.get_stitch_strips() == S
    assert dec.decode_batch_stitched(batch, axis=0)[5].tolist() == tears.tolist()
    # every mode accepts 1 .. 8
    for s in range(1, 9):
        dec.set_stitch_strips(s)
        assert dec.get_stitch_strips() == s
    # n == 1: no pair, no rows in the taps
    dec.set_stitch_strips(S)
    cand, _, masks1, schunks1, smasks1, tears1 = dec.decode_batch_stitched(batch[:1], axis=1)
    assert cand == 0 and masks1[0] == geo.FULL_MASK and schunks1.shape[0] == smasks1.shape[0] == tears1.shape[0] == 0
    assert dec.tap_stitch_strips(1, S).shape == (0, S, 4)
    # the strip taps describe a batch that ran with strips above 1
    dec.set_stitch_strips(1)
    dec.decode_batch_stitched(batch, axis=0)
    for tap in (dec.tap_stitch_strips, dec.tap_stitch_strip_lines):
        with pytest.raises(D.CimbarHipError):
            tap(n, 1)
    dec.decode_batch(batch)
    dec.set_stitch_strips(S)
    with pytest.raises(D.CimbarHipError):
        dec.tap_stitch_strips(n, S)
    dec.set_stitch_strips(1)


@pytest.mark.parametrize("fmt", SC.CAPTURE_FORMATS)
@pytest.mark.parametrize("case", XC.CAPTURE_CASES, ids=lambda c: "axis%d-dir%d" % c)
def test_capture_path_recovers_the_shared_frame(case, fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    axis, direction = case
    geo = geometry.for_mode(68)
    _, payload = SC.rendered(68)
    caps, size = XC.capture_pairs_slanted(axis, direction, fmt)
    dec, ref = D.HipDecoder(0, 68), D.HipDecoder(0, 68)
    try:
        slot = 2 * 1 + direction
        _, pc, pm, pst = ref.scan_extract_decode_batch(caps, preprocess=1, size=size, fmt=fmt)
        cand, chunks, masks, status, schunks, smasks, tears = dec.scan_extract_decode_batch_stitched(caps, axis=axis, preprocess=1, size=size, fmt=fmt)
        what = (tears.tolist(), [hex(int(m)) for m in smasks], [hex(int(m)) for m in masks], status.tolist())
        assert (status > 0).all() and tears[1, 0] == -1 and not smasks[2:4].any() and not schunks[2:4].any(), what
        assert masks[1] != geo.FULL_MASK and masks[2] != geo.FULL_MASK, what
        assert (pc == chunks).all() and (pm == masks).all() and (pst == status).all()
        for S in XC.STRIPS:
            dec.reset_ccm()
            dec.set_stitch_strips(S)
            cand, chunks, masks, status, schunks, smasks, tears = dec.scan_extract_decode_batch_stitched(caps, axis=axis, preprocess=1, size=size, fmt=fmt)
            what = (S, tears.tolist(), dec.tap_stitch_strips(4, S)[1].tolist(), [hex(int(m)) for m in smasks], status.tolist())
            assert (status > 0).all() and tears[1, 0] >= 0 and cand >= 1, what
            assert smasks[slot] == geo.FULL_MASK and (schunks[slot].reshape(-1) == payload[1]).all(), what
            assert _genuine(geo, schunks, smasks, payload), what
            assert (pc == chunks).all() and (pm == masks).all() and (pst == status).all()
            assert _same_ccm(dec.get_ccm(), ref.get_ccm())
    finally:
        dec.close()
        ref.close()
