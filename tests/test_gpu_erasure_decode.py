"""GPU: erasure decoding inside the decode chain (cimbar_hip_set_erasure_decode -> k_erasure_frame), modes 68 / 67 / 66, on frames the
device encoder renders from known payloads.

- Off and clean: never set, set on then off, and on but given clean frames -- chunks and masks byte-identical to a context without it.
- Glare: a saturated white disc, a black disc and a random-noise patch at two sizes each. The mask with erasure decoding is a superset of the
  mask without it, the bytes are equal on the old mask, every chunk in the new mask equals the encoded payload, and the chunk count is
  strictly higher over the set.
- Overload: noise patches far past what erasures can repair, over a few hundred frames: no chunk that differs from the payload is ever in
  the mask; prints how often a chunk was added.
- Pipelined: the glare frames through decode_batch_pipelined / pipeline_wait give what decode_batch gives.
- Settings: get reflects set; modes 4 / 8 refuse it; decode_plain_batch refuses to run while it is on.
Which chunks the retry must deliver is pinned in tests/test_gpu_symbol_erasure_model.py (the model: tests/symbol_erasure_model.py).
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen

pytestmark = pytest.mark.gpu

MODES = [68, 67, 66]
T_SYM = 6


@pytest.fixture(scope="module", params=MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


def _frames(mode, n, seed):
    payload = framegen.synth_payload(n, seed=seed, mode=mode)
    frames = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
    return frames, payload.numpy().reshape(n, -1)


def _glare(frames, seed):
    """per frame: white / black disc or a noise patch, at two radii (fractions of the frame's width), centred a little off the middle"""
    g = np.random.default_rng(seed)
    n, h, w, _ = frames.shape
    yy, xx = np.mgrid[0:h, 0:w]
    kinds = []
    for f in range(n):
        kind, size = ("white", "black", "noise")[f % 3], (0.10, 0.13)[(f // 3) % 2]
        cy, cx = h * (0.45 + 0.1 * g.random()), w * (0.45 + 0.1 * g.random())
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= (size * w) ** 2
        if kind == "white":
            frames[f][disc] = 255
        elif kind == "black":
            frames[f][disc] = 0
        else:
            frames[f][disc] = g.integers(0, 256, (int(disc.sum()), 3), dtype=np.uint8)
        kinds.append((kind, size))
    return kinds


def _decode(mode, frames, setting=None):
    dec = D.HipDecoder(0, mode)
    try:
        if setting is not None:
            dec.set_erasure_decode(*setting)
        total, chunks, masks = dec.decode_batch(frames)
    finally:
        dec.close()
    return total, chunks.reshape(len(frames), -1), masks.astype(np.uint32)


def _chunk_ok(mode, chunks, payload, masks):
    geo = D.geometry.for_mode(mode)
    c = chunks.reshape(len(chunks), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    p = payload.reshape(len(chunks), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    good = (c == p).all(axis=2)
    inmask = ((masks[:, None] >> np.arange(geo.CHUNKS_PER_FRAME)) & 1).astype(bool)
    return good, inmask


def test_erasure_setting_roundtrip(MODE):
    dec = D.HipDecoder(0, MODE)
    try:
        geo = dec.geo
        assert dec.get_erasure_decode() == (False, 0, -1, geo.RS_PARITY - 8)
        dec.set_erasure_decode(T_SYM)
        assert dec.get_erasure_decode() == (True, T_SYM, -1, geo.RS_PARITY - 8)
        dec.set_erasure_decode(T_SYM, 3, 12)
        assert dec.get_erasure_decode() == (True, T_SYM, 3, 12)
        frames, _ = _frames(MODE, 1, 5)
        with pytest.raises(D.CimbarHipError):
            dec.decode_plain_batch(frames)
        with pytest.raises(D.CimbarHipError):
            dec.set_erasure_decode(T_SYM, -1, geo.RS_PARITY + 1)
        dec.set_erasure_decode(0)
        assert dec.get_erasure_decode()[0] is False
        dec.decode_plain_batch(frames)
    finally:
        dec.close()


@pytest.mark.parametrize("legacy", [4, 8])
def test_erasure_refused_in_legacy_modes(legacy):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dec = D.HipDecoder(0, legacy)
    try:
        with pytest.raises(D.CimbarHipError):
            dec.set_erasure_decode(T_SYM)
        dec.set_erasure_decode(0)
        assert dec.get_erasure_decode()[0] is False
    finally:
        dec.close()


def test_off_and_clean_identical(MODE):
    frames, payload = _frames(MODE, 6, 11)
    glare = frames.copy()
    _glare(glare, 3)
    for fr in (frames, glare):
        base = _decode(MODE, fr)
        dec = D.HipDecoder(0, MODE)
        try:
            dec.set_erasure_decode(T_SYM)
            dec.set_erasure_decode(0)
            got = dec.decode_batch(fr)
        finally:
            dec.close()
        assert got[0] == base[0] and (got[1].reshape(len(fr), -1) == base[1]).all() and (got[2] == base[2]).all()
    on = _decode(MODE, frames, (T_SYM,))
    base = _decode(MODE, frames)
    assert on[0] == base[0] and (on[1] == base[1]).all() and (on[2] == base[2]).all()
    assert (base[1] == payload).all()


def test_glare_superset_and_recovery(MODE):
    frames, payload = _frames(MODE, 12, 21)
    kinds = _glare(frames, 7)
    t0, c0, m0 = _decode(MODE, frames)
    t1, c1, m1 = _decode(MODE, frames, (T_SYM,))
    assert ((m0 & m1) == m0).all(), "the mask lost a chunk"
    good0, in0 = _chunk_ok(MODE, c0, payload, m0)
    good1, in1 = _chunk_ok(MODE, c1, payload, m1)
    geo = D.geometry.for_mode(MODE)
    c0r, c1r = c0.reshape(len(frames), geo.CHUNKS_PER_FRAME, -1), c1.reshape(len(frames), geo.CHUNKS_PER_FRAME, -1)
    assert (c0r[in0] == c1r[in0]).all(), "bytes changed on a chunk the old mask had"
    assert good1[in1].all(), "a chunk in the new mask differs from the payload"
    assert (c1r[~in1] == 0).all(), "a slot outside the mask is not zero"
    assert t1 == geo.CHUNK * int(in1.sum())
    gained = int(in1.sum() - in0.sum())
    print(f"mode {MODE}: chunks {int(in0.sum())} -> {int(in1.sum())} of {in0.size}; per frame gained",
          [(k, int(in1[f].sum() - in0[f].sum())) for f, k in enumerate(kinds)])
    assert gained > 0, "erasure decoding recovered nothing on the glare frames"


def test_overload_never_wrong(MODE):
    n = 240
    frames, payload = _frames(MODE, n, 31)
    g = np.random.default_rng(9)
    h, w = frames.shape[1:3]
    for f in range(n):       # 6 .. 12 noise patches of 40..90 px: far more damage than a block's parity covers
        for _ in range(int(g.integers(6, 13))):
            s = int(g.integers(40, 91))
            y, x = int(g.integers(60, h - 60 - s)), int(g.integers(60, w - 60 - s))
            frames[f, y:y + s, x:x + s] = g.integers(0, 256, (s, s, 3), dtype=np.uint8)
    _, c0, m0 = _decode(MODE, frames)
    _, c1, m1 = _decode(MODE, frames, (T_SYM,))
    assert ((m0 & m1) == m0).all()
    good1, in1 = _chunk_ok(MODE, c1, payload, m1)
    _, in0 = _chunk_ok(MODE, c0, payload, m0)
    print(f"mode {MODE} overload: {int(in0.sum())} chunks without erasures, {int(in1.sum())} with, of {in1.size}")
    assert good1[in1].all(), "a wrong chunk reached the mask"


def test_pipelined_matches_batch(MODE):
    frames, payload = _frames(MODE, 9, 41)
    _glare(frames, 13)
    _, c_ref, m_ref = _decode(MODE, frames, (T_SYM,))
    dev = torch.device("cuda", 0)
    geo = D.geometry.for_mode(MODE)
    fb = geo.CHUNKS_PER_FRAME * geo.CHUNK
    dec = D.HipDecoder(0, MODE)
    try:
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
