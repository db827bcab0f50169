"""GPU: torn-capture stitching (cimbar_hip_decode_batch_stitched / _scan_extract_decode_batch_stitched_fmt) on the frames and tear positions
of tests/stitch_cases.py (tests/test_stitch_model.py vets them on the CPU), in every mode unless noted.

- Recovery: A, T1, T2, C and the direction-1 mirror, on both axes: the slot of (T1, T2) in the pair's direction has the full mask and B's
  payload byte for byte, neither torn capture's own mask is full, and every chunk in any smask is the payload chunk of A, B or C in that slot.
- Model parity: tears, TAP_STITCH_LINES and TAP_STITCH_CELLS equal tests/stitch_model.py applied to the device's own TAP_SYMBOLS / TAP_COLORS,
  bit for bit, on a batch whose band lines are noise-damaged on both sides of the 3/4 rule.
- Non-candidates (copies of one frame, two different frames, a one-line band with min_band 2; capture path: a blank capture): a = -1, mask 0
  and zero slots written over a poisoned buffer.
- Passthrough: the per-capture chunks, masks and the carried matrix equal decode_batch's (capture path: scan_extract_decode_batch's).
- Device outputs equal host outputs; n == 1 returns 0; a bad axis or min_band is EINVAL.
- Capture path (mode 68, 1080p, formats 3 and 12): the CPU-vetted pairs recover B.
"""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import stitch_cases as SC
from tests import stitch_model as SM

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


def _device_call(dec, batch, axis=0, min_agree_permille=0, min_band=0, tears=True):
    """decode_batch_stitched_device over poisoned output buffers -> (rc, chunks, masks, schunks, smasks, tears) as numpy"""
    geo = dec.geo
    dev = torch.device("cuda", 0)
    n = len(batch)
    d_in = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
    chunks, masks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
    schunks, smasks = mk((2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((2 * (n - 1),), torch.int32)
    d_tears = mk((n - 1, 4), torch.int32)
    st = torch.cuda.current_stream(dev).cuda_stream
    rc = dec.decode_batch_stitched_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(),
                                          d_tears.data_ptr() if tears else None, axis=axis, min_agree_permille=min_agree_permille,
                                          min_band=min_band, stream=st)
    torch.cuda.synchronize(dev)
    return (rc, chunks.cpu().numpy(), masks.cpu().numpy().view(np.uint32), schunks.cpu().numpy(), smasks.cpu().numpy().view(np.uint32),
            d_tears.cpu().numpy())


def test_recovery_on_both_axes_and_in_both_directions(MODE, dec):
    geo = dec.geo
    frames, payload = SC.rendered(MODE)
    for axis in (0, 1):
        for direction in (0, 1):
            for name in SC.TEARS:
                p1, p2 = SC.tear_pixels(MODE, axis, name)
                t1, t2 = SC.torn_pair(frames[0], frames[1], frames[2], axis, p1, p2, direction)
                cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(np.stack([frames[0], t1, t2, frames[2]]), axis=axis)
                what = (MODE, axis, direction, name, tears.tolist(), [hex(int(m)) for m in smasks], [hex(int(m)) for m in masks])
                assert tears[1, 0] >= 0 and cand == int((tears[:, 0] >= 0).sum()) >= 1, what
                slot = 2 * 1 + direction
                assert smasks[slot] == geo.FULL_MASK, what
                assert (schunks[slot].reshape(-1) == payload[1]).all(), what
                assert masks[1] != geo.FULL_MASK and masks[2] != geo.FULL_MASK, what
                assert masks[0] == masks[3] == geo.FULL_MASK, what
                assert _genuine(geo, schunks, smasks, payload), what


@pytest.mark.parametrize("axis", [0, 1])
def test_model_parity_with_damaged_band_lines(MODE, dec, axis):
    batch = SC.damaged_band_batch(MODE, axis)
    n = len(batch)
    cand, _, _, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=axis)
    sym, col = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)
    want_tears, want_cnt, want_cells = SM.stitch_batch(MODE, sym, col, axis)
    assert tears.tolist() == want_tears.tolist()
    assert (dec.tap_stitch_lines(n, axis) == want_cnt).all()
    assert (dec.tap(D.TAP_STITCH_CELLS, n) == want_cells).all()
    # three damaged lines of twelve pass the 3/4 rule, four do not
    assert tears[0].tolist() == [SC.BAND_LO, SC.BAND_LO + 12, SC.BAND_LO + 6, 9] and tears[3].tolist() == [-1, -1, -1, 8]
    assert cand == int((tears[:, 0] >= 0).sum())
    assert not smasks[6:8].any() and not schunks[6:8].any()
    # the caller's threshold and band reach the kernel: parity again
    # (the taps again: the colour-correction matrix this call inherits may settle a noise cell's colour differently)
    _, _, _, _, _, tears = dec.decode_batch_stitched(batch, axis=axis, min_agree_permille=990, min_band=10)
    sym, col = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)
    want_tears, want_cnt, want_cells = SM.stitch_batch(MODE, sym, col, axis, 990, 10)
    assert tears.tolist() == want_tears.tolist()
    assert (dec.tap_stitch_lines(n, axis) == want_cnt).all()
    assert (dec.tap(D.TAP_STITCH_CELLS, n) == want_cells).all()


def test_non_candidates_write_zeroes_over_a_poisoned_buffer(MODE, dec):
    geo = dec.geo
    frames, _ = SC.rendered(MODE)
    L = geo.DIM_Y
    one_line = SC.torn_pair(frames[0], frames[1], frames[2], 0, geo.OFFSET + 40 * geo.PITCH, geo.OFFSET + 41 * geo.PITCH, 0)
    cases = {
        "copies of one frame": (np.stack([frames[0]] * 3), [L, L]),
        "two different frames": (np.stack([frames[0], frames[1]]), [0]),
        "a one-line band": (np.stack(one_line), [1]),
    }
    for name, (batch, flagged) in cases.items():
        rc, chunks, masks, schunks, smasks, tears = _device_call(dec, batch, axis=0, min_band=2)
        assert rc == 0
        assert tears.tolist() == [[-1, -1, -1, f] for f in flagged], (name, tears.tolist())
        assert not smasks.any() and not schunks.any(), name
        assert (dec.tap(D.TAP_STITCH_CELLS, len(batch)) == 0).all(), name
    # ... and the one-line band is a candidate once min_band allows it
    assert dec.decode_batch_stitched(np.stack(one_line), axis=0, min_band=1)[5].tolist() == [[40, 41, 40, 1]]


def test_passthrough_and_device_outputs(MODE, dec):
    geo = dec.geo
    frames, payload = SC.rendered(MODE)
    p1, p2 = SC.tear_pixels(MODE, 0, "across")
    t1, t2 = SC.torn_pair(frames[0], frames[1], frames[2], 0, p1, p2, 0)
    batch = np.stack([frames[0], t1, t2, frames[2], frames[2]])
    ref = D.HipDecoder(0, MODE)
    try:
        dec.reset_ccm()
        _, rchunks, rmasks = ref.decode_batch(batch)
        rccm = ref.get_ccm()
        cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(batch, axis=0)
        assert (chunks == rchunks).all() and (masks == rmasks).all()
        assert dec.get_ccm()[0] == rccm[0] and np.array_equal(np.asarray(dec.get_ccm()[1]), np.asarray(rccm[1]))
        assert cand == 3 and tears[3].tolist() == [-1, -1, -1, geo.DIM_Y]       # (A, T1) and (T2, C) share a band too: A's and C's chunks again
        # the erasure settings do not reach the stitched decode
        if not geo.LEGACY:
            ref.reset_ccm()
            ref.set_erasure_decode(6)
            ref.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)
            _, _, _, eschunks, esmasks, etears = ref.decode_batch_stitched(batch, axis=0)
            assert (eschunks == schunks).all() and (esmasks == smasks).all() and (etears == tears).all()
    finally:
        ref.close()
    # device outputs over poisoned buffers == host outputs
    dec.reset_ccm()
    rc, dchunks, dmasks, dschunks, dsmasks, dtears = _device_call(dec, batch, axis=0)
    assert rc == 0
    assert (dchunks == chunks).all() and (dmasks == masks).all() and (dschunks == schunks).all() and (dsmasks == smasks).all()
    assert (dtears == tears).all()
    rc, _, _, dschunks, dsmasks, _ = _device_call(dec, batch, axis=0, tears=False)       # tears may be NULL
    assert rc == 0 and (dschunks == schunks).all() and (dsmasks == smasks).all()
    # n == 1: no pair
    cand, chunks1, masks1, schunks1, smasks1, tears1 = dec.decode_batch_stitched(batch[:1], axis=1)
    assert cand == 0 and masks1[0] == geo.FULL_MASK and (chunks1[0].reshape(-1) == payload[0]).all()
    assert schunks1.shape[0] == smasks1.shape[0] == tears1.shape[0] == 0
    # what the library refuses, before anything is enqueued
    for bad in (dict(axis=2), dict(axis=-1), dict(axis=0, min_band=geo.DIM_Y + 1), dict(axis=1, min_band=geo.DIM_X + 1)):
        with pytest.raises(D.CimbarHipError):
            dec.decode_batch_stitched(batch, **bad)
    lib, vp = dec._lib, ctypes.c_void_p
    c, m = np.zeros_like(chunks), np.zeros_like(masks)
    assert lib.cimbar_hip_decode_batch_stitched(dec._ctx, batch.ctypes.data, len(batch), D.MEM_HOST, 0, 2, 0, 0, 0, c.ctypes.data, m.ctypes.data,
                                                vp(None), vp(None), vp(None), D.MEM_HOST, None) == -1
    assert dec.decode_batch_stitched(batch, axis=1, min_band=geo.DIM_X)[0] == 0


@pytest.mark.parametrize("fmt", SC.CAPTURE_FORMATS)
@pytest.mark.parametrize("case", SC.CAPTURE_CASES, ids=lambda c: "axis%d-dir%d-%s" % c)
def test_capture_path_recovers_the_shared_frame(case, fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    axis, direction, name = case
    geo = geometry.for_mode(68)
    _, payload = SC.rendered(68)
    caps, size = SC.capture_pairs(axis, direction, name, fmt)
    dec, ref = D.HipDecoder(0, 68), D.HipDecoder(0, 68)
    try:
        cand, chunks, masks, status, schunks, smasks, tears = dec.scan_extract_decode_batch_stitched(caps, axis=axis, preprocess=1, size=size, fmt=fmt)
        what = (tears.tolist(), [hex(int(m)) for m in smasks], [hex(int(m)) for m in masks], status.tolist())
        assert (status > 0).all() and tears[1, 0] >= 0 and cand >= 1, what
        slot = 2 * 1 + direction
        assert smasks[slot] == geo.FULL_MASK and (schunks[slot].reshape(-1) == payload[1]).all(), what
        assert masks[1] != geo.FULL_MASK and masks[2] != geo.FULL_MASK, what
        assert _genuine(geo, schunks, smasks, payload), what
        _, pc, pm, pst = ref.scan_extract_decode_batch(caps, preprocess=1, size=size, fmt=fmt)
        assert (pc == chunks).all() and (pm == masks).all() and (pst == status).all()
        assert dec.get_ccm()[0] == ref.get_ccm()[0] and np.array_equal(np.asarray(dec.get_ccm()[1]), np.asarray(ref.get_ccm()[1]))
        # a blank capture between the torn ones: in no pair, zeroes over a poisoned buffer
        blank = np.full_like(caps[:1], 16 if fmt == 12 else 0)
        raw = np.ascontiguousarray(np.concatenate([caps[:2], blank, caps[2:3]]))
        n = len(raw)
        c, m, st = np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.int32)
        sc = np.full((2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK), POISON, np.uint8)
        sm, tr = np.full(2 * (n - 1), 0xA5A5A5A5, np.uint32), np.full((n - 1, 4), 0x5A5A5A5A, np.int32)
        rc = dec._lib.cimbar_hip_scan_extract_decode_batch_stitched_fmt(dec._ctx, raw.ctypes.data, size[0], size[1], fmt, n, D.MEM_HOST, 1, 2, axis, 0, 0,
                                                                        c.ctypes.data, m.ctypes.data, st.ctypes.data, sc.ctypes.data, sm.ctypes.data,
                                                                        tr.ctypes.data, D.MEM_HOST, None)
        assert rc >= 0 and st[2] <= 0 and (st[[0, 1, 3]] > 0).all(), (rc, st.tolist())
        assert (tr[1:, :3] == -1).all() and not sm[2:].any() and not sc[2:].any(), (tr.tolist(), sm.tolist())
        assert rc == int((tr[:, 0] >= 0).sum())
    finally:
        dec.close()
        ref.close()
