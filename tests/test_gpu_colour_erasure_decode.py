"""GPU: colour erasure decoding inside the decode chain (cimbar_hip_set_colour_erasure_decode -> k_colour_erasure_frame), modes 68 / 67 / 66,
on frames rendered from known payloads. One threshold everywhere: decoder.COLOUR_MARGIN_SUGGESTED.

- Settings: get reflects set; off by default; max_erasures above the parity and modes 4 / 8 are refused; decode_plain_batch is refused while it
  is on and works again after; the symbol setting and the colour setting do not touch each other; the margin tap is EINVAL while off.
- Off and clean: never set, set then unset, and on with clean frames give total, chunks and masks byte-identical to a fresh context.
- Margin tap: equals the model on every cell of every frame the retry worked on, flooded frames (a one-pixel shift) and not flooded ones both
  present; 0xFFFFFFFF for the frames it skipped.
- Glare: the new mask is a superset of the old, bytes equal on the old mask, every chunk in the new mask equals the payload, the symbol bits
  are unchanged with only the colour setting on, more colour chunks are delivered over the set; both settings on give the union of the two
  single-setting masks.
- Model: the device's chunks and masks equal tests/colour_erasure_model.py chunk for chunk on the glare set and its shifted copies.
- Overload: 240 frames damaged far beyond repair: no chunk that differs from the payload is ever in the mask.
- Pipelined, decode_frame_async and the capture path give what decode_batch gives.
- Combined: gmask is a superset of every member's mask and every group chunk equals the payload; the members' colour retry reaches the group.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import colour_erasure_cases as K
from tests import colour_erasure_model as M
from tests import frames as F

pytestmark = pytest.mark.gpu

T_SYM = 6                      # the symbol retry's threshold in tests/test_gpu_erasure_decode.py


@pytest.fixture(scope="module", params=K.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


def _decode(mode, frames, colour=None, sym=None, pre=False):
    dec = D.HipDecoder(0, mode)
    try:
        if colour is not None:
            dec.set_colour_erasure_decode(*colour)
        if sym is not None:
            dec.set_erasure_decode(*sym)
        total, chunks, masks = dec.decode_batch(frames, pre)
    finally:
        dec.close()
    return total, chunks.reshape(len(frames), -1), masks.astype(np.uint32)


def _colour_count(geo, masks):
    return int(sum(bin(int(m) >> K.sym_chunks(geo)).count("1") for m in masks))


def _with_shifted(frames):
    """the frames, then one-pixel shifted copies of every second one (those go through the flood pass)"""
    return np.concatenate([frames, np.stack([F.shift(frames[k], 1, 0) for k in range(0, len(frames), 2)])])


def _washed(mode, n, seed):
    """frames with a disc whose colour is washed out -- every pixel's channels become its largest one -- at radii 0.07 .. 0.11 of the width.
    Bright pixels stay bright and dark ones dark, so the symbols survive and the frame does not go through the flood pass; the colour
    stream loses the disc (white cells: margin 0)."""
    fr, _ = K.frames(mode, n, seed)
    g = np.random.default_rng(seed)
    h, w = fr.shape[1:3]
    yy, xx = np.mgrid[0:h, 0:w]
    for f in range(n):
        cy, cx = h * (0.45 + 0.1 * g.random()), w * (0.45 + 0.1 * g.random())
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= ((0.07, 0.09, 0.11)[f % 3] * w) ** 2
        fr[f][disc] = fr[f][disc].max(axis=1, keepdims=True)
    return fr


def test_settings(MODE):
    dec = D.HipDecoder(0, MODE)
    try:
        geo = dec.geo
        assert dec.get_colour_erasure_decode() == (False, 0, geo.RS_PARITY - 8)
        dec.set_colour_erasure_decode(K.MARGIN)
        assert dec.get_colour_erasure_decode() == (True, K.MARGIN, geo.RS_PARITY - 8)
        assert dec.get_erasure_decode() == (False, 0, -1, geo.RS_PARITY - 8)          # the symbol setting is untouched
        dec.set_colour_erasure_decode(777, 12)
        assert dec.get_colour_erasure_decode() == (True, 777, 12)
        dec.set_erasure_decode(T_SYM, 3, 9)
        assert dec.get_erasure_decode() == (True, T_SYM, 3, 9)
        assert dec.get_colour_erasure_decode() == (True, 777, 12)                     # ... and the other way round
        dec.set_erasure_decode(0)
        dec.set_colour_erasure_decode(777, geo.RS_PARITY)
        with pytest.raises(D.CimbarHipError):
            dec.set_colour_erasure_decode(777, geo.RS_PARITY + 1)
        assert dec.get_colour_erasure_decode() == (True, 777, geo.RS_PARITY)
        frames, _ = K.frames(MODE, 1, 5)
        with pytest.raises(D.CimbarHipError):
            dec.decode_plain_batch(frames)
        dec.set_colour_erasure_decode(0)
        assert dec.get_colour_erasure_decode()[0] is False
        dec.decode_plain_batch(frames)
        dec.decode_batch(frames)
        with pytest.raises(D.CimbarHipError):
            dec.tap(D.TAP_COLOUR_MARGIN, 1)                                           # the last batch ran with the setting off
    finally:
        dec.close()


@pytest.mark.parametrize("legacy", [4, 8])
def test_refused_in_legacy_modes(legacy):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dec = D.HipDecoder(0, legacy)
    try:
        with pytest.raises(D.CimbarHipError):
            dec.set_colour_erasure_decode(K.MARGIN)
        dec.set_colour_erasure_decode(0)
        assert dec.get_colour_erasure_decode()[0] is False
    finally:
        dec.close()


def test_off_and_clean_identical(MODE):
    frames, payload = K.frames(MODE, 6, 11)
    glare = frames.copy()
    K.glare(glare, 3)
    for fr in (frames, glare):
        base = _decode(MODE, fr)
        dec = D.HipDecoder(0, MODE)
        try:
            dec.set_colour_erasure_decode(K.MARGIN)
            dec.set_colour_erasure_decode(0)
            got = dec.decode_batch(fr)
        finally:
            dec.close()
        assert got[0] == base[0] and (got[1].reshape(len(fr), -1) == base[1]).all() and (got[2] == base[2]).all()
    on = _decode(MODE, frames, (K.MARGIN,))
    base = _decode(MODE, frames)
    assert on[0] == base[0] and (on[1] == base[1]).all() and (on[2] == base[2]).all()
    assert (base[1] == payload).all()


def _device_and_model(mode, frames):
    """-> (device chunks, masks with the colour retry on), (the model's, from the device's own colours / drift / matrix taps and the result
    without the retry), the margin tap, the model's margins, the flood tap, which frames the model worked on"""
    geo = geometry.for_mode(mode)
    n = len(frames)
    _, c0, m0 = _decode(mode, frames)
    dec = D.HipDecoder(0, mode)
    try:
        dec.set_colour_erasure_decode(K.MARGIN)
        _, c1, m1 = dec.decode_batch(frames)
        col, drift, ccm = dec.tap(D.TAP_COLORS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_CCM, n)
        flood, rs_ok, tap = dec.tap(D.TAP_FLOOD, n), dec.tap(D.TAP_RS_OK, n), dec.tap(D.TAP_COLOUR_MARGIN, n)
    finally:
        dec.close()
    xy = geo.cell_positions().astype(np.int64)
    want_c, want_m, want_mg, worked = [], [], [], []
    for f in range(n):
        mg = M.margins(M.cell_means(frames[f], xy + drift[f].astype(np.int64)), ccm[f])
        wm, wc, w = M.retry_frame(geo, col[f], mg, m0[f], c0[f], K.MARGIN)
        if w:
            # the chain's per-block flags of the colour blocks are what the model works out for itself
            blocks = M.stream_bytes(geo, col[f])
            lacking = [cb for cb in range(geo.COL_BLOCKS) if not (int(m0[f]) >> ((geo.SYM_BLOCKS + cb) // (geo.CHUNK // geo.RS_DATA))) & 1]
            assert all(bool(rs_ok[f, geo.SYM_BLOCKS + cb]) == M.errors_only_ok(blocks[cb], geo.RS_PARITY) for cb in lacking), f
        want_c.append(wc.reshape(-1)); want_m.append(wm); want_mg.append(mg); worked.append(w)
    return (c1.reshape(n, -1), m1.astype(np.uint32)), (np.stack(want_c), np.array(want_m, np.uint32)), tap, np.stack(want_mg), flood, np.array(worked)


def test_margin_tap_and_model_equality(MODE):
    frames, _, _, _ = K.glare_set(MODE)
    clean, _ = K.frames(MODE, 2, 77)
    batch = np.concatenate([_with_shifted(frames), _washed(MODE, 6, 55), clean])
    (c1, m1), (wc, wm), tap, want_mg, flood, worked = _device_and_model(MODE, batch)
    print(f"mode {MODE}: {int(worked.sum())} of {len(batch)} frames retried, {int(flood[worked].sum())} of them flooded")
    assert not worked[-2:].any() and worked.any()
    assert flood[worked].any() and not flood[worked].all(), "the retried frames must include flooded and not flooded ones"
    for f in range(len(batch)):
        if worked[f]:
            assert (tap[f] == want_mg[f]).all(), (f, int((tap[f] != want_mg[f]).sum()))
        else:
            assert (tap[f] == M.SKIPPED).all(), f
    assert (m1 == wm).all(), (m1, wm)
    assert (c1 == wc).all()


def test_glare_superset_and_recovery(MODE):
    geo = geometry.for_mode(MODE)
    frames, payload, kinds, _ = K.glare_set(MODE)
    symbits = np.uint32((1 << K.sym_chunks(geo)) - 1)
    t0, c0, m0 = _decode(MODE, frames)
    t1, c1, m1 = _decode(MODE, frames, (K.MARGIN,))
    ts, cs, ms = _decode(MODE, frames, None, (T_SYM,))
    tb, cb, mb = _decode(MODE, frames, (K.MARGIN,), (T_SYM,))
    assert ((m0 & m1) == m0).all(), "the mask lost a chunk"
    assert ((m0 ^ m1) & symbits == 0).all(), "the colour retry changed a symbol bit"
    good1, in1 = K.chunk_ok(geo, c1, payload, m1)
    _, in0 = K.chunk_ok(geo, c0, payload, m0)
    r = lambda c: c.reshape(len(frames), geo.CHUNKS_PER_FRAME, -1)
    assert (r(c0)[in0] == r(c1)[in0]).all(), "bytes changed on a chunk the old mask had"
    assert good1[in1].all(), "a chunk in the new mask differs from the payload"
    assert (r(c1)[~in1] == 0).all(), "a slot outside the mask is not zero"
    assert t1 == geo.CHUNK * int(in1.sum())
    n0, n1 = _colour_count(geo, m0), _colour_count(geo, m1)
    print(f"mode {MODE}: colour chunks {n0} -> {n1} of {len(frames) * (geo.CHUNKS_PER_FRAME - K.sym_chunks(geo))}; all chunks {int(in0.sum())} -> "
          f"colour retry {int(in1.sum())}, symbol retry {bin(int.from_bytes(ms.tobytes(), 'little')).count('1')}, both "
          f"{bin(int.from_bytes(mb.tobytes(), 'little')).count('1')} of {in0.size}; per frame gained",
          [(k, bin(int(m1[f]) ^ int(m0[f])).count("1")) for f, k in enumerate(kinds)])
    assert n1 > n0, "colour erasure decoding recovered nothing on the glare frames"
    # both on: the union of the two single-setting masks, each chunk the payload's
    assert (mb == (m1 | ms)).all(), (mb, m1, ms)
    goodb, inb = K.chunk_ok(geo, cb, payload, mb)
    assert goodb[inb].all() and (r(cb)[~inb] == 0).all() and tb == geo.CHUNK * int(inb.sum())


def test_overload_never_wrong(MODE):
    geo = geometry.for_mode(MODE)
    n = 240
    frames, payload = K.frames(MODE, n, 31)
    K.overload(frames)
    _, c0, m0 = _decode(MODE, frames)
    _, c1, m1 = _decode(MODE, frames, (K.MARGIN,))
    _, cb, mb = _decode(MODE, frames, (K.MARGIN,), (T_SYM,))
    assert ((m0 & m1) == m0).all() and ((m1 & mb) == m1).all()
    good1, in1 = K.chunk_ok(geo, c1, payload, m1)
    goodb, inb = K.chunk_ok(geo, cb, payload, mb)
    print(f"mode {MODE} overload: colour chunks {_colour_count(geo, m0)} without the colour retry, {_colour_count(geo, m1)} with, "
          f"of {n * (geo.CHUNKS_PER_FRAME - K.sym_chunks(geo))}; all chunks with both retries {int(inb.sum())} of {inb.size}")
    assert good1[in1].all() and goodb[inb].all(), "a wrong chunk reached the mask"


def test_pipelined_matches_batch(MODE):
    frames, _, _, _ = K.glare_set(MODE)
    frames = frames[:9]
    _, c_ref, m_ref = _decode(MODE, frames, (K.MARGIN,), (T_SYM,))
    dev = torch.device("cuda", 0)
    geo = geometry.for_mode(MODE)
    fb = geo.CHUNKS_PER_FRAME * geo.CHUNK
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_colour_erasure_decode(K.MARGIN)
        dec.set_erasure_decode(T_SYM)
        st = torch.cuda.current_stream(dev).cuda_stream
        tens = [torch.from_numpy(np.ascontiguousarray(frames[3 * k:3 * k + 3])).to(dev) for k in range(3)]
        outs = [(torch.zeros((3, fb), dtype=torch.uint8, device=dev), torch.zeros((3,), dtype=torch.int32, device=dev)) for _ in tens]
        for t, (c, m) in zip(tens, outs):
            dec.decode_batch_pipelined(t.data_ptr(), 3, c.data_ptr(), m.data_ptr(), False, 2, st)
        dec.pipeline_wait(st)
        torch.cuda.synchronize()
        c = np.concatenate([o[0].cpu().numpy() for o in outs])
        m = np.concatenate([o[1].cpu().numpy() for o in outs]).astype(np.uint32)
    finally:
        dec.close()
    assert (m == m_ref).all() and (c == c_ref).all()


def test_frame_async_matches_batch(MODE):
    frames, _, _, _ = K.glare_set(MODE)
    frames = frames[3:9]
    _, c_ref, m_ref = _decode(MODE, frames, (K.MARGIN,))
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_colour_erasure_decode(K.MARGIN)
        tickets = []
        got = []
        for f in range(len(frames)):
            tickets.append(dec.decode_frame_async(frames[f]))
            if len(tickets) == 2:
                got.append(dec.decode_frame_wait(tickets.pop(0)))
        while tickets:
            got.append(dec.decode_frame_wait(tickets.pop(0)))
    finally:
        dec.close()
    for f, (_, c, m) in enumerate(got):
        assert m == m_ref[f] and (c.reshape(-1) == c_ref[f]).all(), f
    assert (m_ref != _decode(MODE, frames)[2]).any(), "the frames chosen must be ones the retry changes"


def test_capture_path_matches_batch(MODE):
    geo = geometry.for_mode(MODE)
    frames, _, _, _ = K.glare_set(MODE)
    quad = {68: ((500, 40), (1484, 60), (480, 1034), (1494, 1024)), 67: ((300, 150), (1600, 170), (290, 930), (1620, 915)),
            66: ((400, 60), (1500, 75), (395, 1010), (1510, 1000))}[MODE]
    cams = np.stack([F.camera_frame(frames[k], quad=quad, background=96) for k in (0, 3, 6, 9)])      # (the white discs: large black or noise ones can make the anchor search fail)
    dec = D.HipDecoder(0, MODE)
    try:
        status, _, ext = dec.extract_batch(cams)
        assert (status > 0).all(), status
        # (preprocess given, not left to the extractor's verdict per capture: one decode_batch call is then the same work)
        _, c_off, m_off = _decode(MODE, ext, pre=False)
        _, c_ref, m_ref = _decode(MODE, ext, (K.MARGIN,), pre=False)
        dec.set_colour_erasure_decode(K.MARGIN)
        _, c, m, st = dec.scan_extract_decode_batch(cams, preprocess=0)
        assert (st == status).all()
        assert (m == m_ref).all() and (c.reshape(len(cams), -1) == c_ref).all()
        assert ((m_off & m) == m_off).all()
        print(f"mode {MODE} capture path: colour chunks {_colour_count(geo, m_off)} -> {_colour_count(geo, m)}")
    finally:
        dec.close()


def test_combined_picks_up_the_members_retry(MODE):
    geo = geometry.for_mode(MODE)
    frames, payload, _, _ = K.glare_set(MODE)
    # two captures of each frame: the glare one and the same disc mirrored left to right (other cells damaged)
    clean, _ = K.frames(MODE, K.GLARE_N, K.GLARE_SEED)
    caps, groups = [], []
    for k in range(3, 9):
        other = clean[k].copy()
        damaged = (frames[k] != clean[k]).any(axis=2)
        other[damaged[:, ::-1]] = 255
        caps += [frames[k], other]
        groups += [k - 3, k - 3]
    caps = np.stack(caps)
    off, on = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        on.set_colour_erasure_decode(K.MARGIN)
        ng0, c0, m0, _, _, g0 = off.decode_batch_combined(caps, groups=groups)
        ng1, c1, m1, _, gc1, g1 = on.decode_batch_combined(caps, groups=groups)
        _, cr, mr = _decode(MODE, caps, (K.MARGIN,))
    finally:
        off.close()
        on.close()
    assert ng0 == ng1 == 6
    assert (m1 == mr).all() and (c1.reshape(len(caps), -1) == cr).all(), "the per-capture part differs from decode_batch"
    g0, g1 = g0[:6].astype(np.uint32), g1[:6].astype(np.uint32)
    assert ((g0 & g1) == g0).all()
    supplied = 0
    for g in range(6):
        members = m1[2 * g] | m1[2 * g + 1]
        assert (int(g1[g]) & int(members)) == int(members), "gmask is not a superset of a member's mask"
        goodg, ing = K.chunk_ok(geo, gc1[g][None], payload[g + 3][None], g1[g:g + 1])
        assert goodg[ing].all(), g
        supplied += bin(int(g1[g]) & ~int(g0[g])).count("1")
    print(f"mode {MODE} combined: the members' colour retry supplied {supplied} group chunks; members gained "
          f"{_colour_count(geo, m1) - _colour_count(geo, m0)} colour chunks")
    assert _colour_count(geo, m1) > _colour_count(geo, m0)
