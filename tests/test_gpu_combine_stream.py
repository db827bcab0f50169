"""GPU: multi-capture decoding across calls (cimbar_hip_decode_batch_combined_stream / _scan_extract_decode_batch_combined_stream_fmt /
cimbar_hip_combine_stream_reset), frames rendered from known payloads, in every mode unless noted. Fresh contexts per comparison.

1. Split equivalence: A A A B B T C C C D' D'' (T = B's top half over C's bottom half, D', D'' a disc-damaged pair) cut into two calls at
   every place, into one capture per call and into (2, 3, 4, 2) reports the groups of ONE decode_batch_combined call, in order, with its
   per-capture outputs and carried colour matrix; groups_out is the stream model's.
2. Recovery across a boundary: a disjoint-disc pair, one capture per call -- nothing closes in the first call, the second delivers every
   chunk; decode_batch_combined on the same single captures delivers no symbol chunk.
3. Model parity with a carried member: the group-cells and margin taps of the closing call equal tests/combine_model.combine_cells.
4. Cap and unanimous skip: six copies as (3, 3) and one per call with max_group 4 close as 4 + 2, the 4 in the call of its fourth member,
   which is not flushed.
5. The carry is a copy: other calls on the context between the two stream calls of case 2 change nothing.
6. Parameters and edges.
7. Capture path (formats 3 and 12): blank captures close groups at the end of a call and at the start of the next; recovery as in 2.
8. Device outputs: (2, 3, 4, 2) with poisoned buffers and no synchronise between the calls equals the host-output run.
9. Erasure decoding on: the split run's group outputs equal the one-call run's; no wrong chunk in any gmask.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from tests import capture_formats as CF
from tests import combine_model as CM
from tests import combine_stream_model as SM
from tests import frames as F
from tests import group_walk_cases as GW

pytestmark = pytest.mark.gpu

MODES = [68, 67, 66, 4, 8]


@pytest.fixture(scope="module", params=MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


# ---- the frame helpers of tests/test_gpu_capture_combine.py
def _frames(mode, n, seed):
    payload = framegen.synth_payload(n, seed=seed, mode=mode)
    frames = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
    return frames, payload.numpy().reshape(n, -1)


def _disc(frame, cx, cy, r, kind, seed):
    h, w, _ = frame.shape
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * min(h, w)) ** 2
    if kind == "white":
        frame[d] = 255
    elif kind == "black":
        frame[d] = 0
    else:
        frame[d] = np.random.default_rng(seed).integers(0, 256, (int(d.sum()), 3), dtype=np.uint8)
    return frame


def _band(frame, x0, x1, kind, seed):
    """a fill over columns [x0, x1) and rows [0.1, 0.9) of the frame (fractions; the corner anchors stay clean)"""
    h, w, _ = frame.shape
    ys, xs = slice(int(0.1 * h), int(0.9 * h)), slice(int(x0 * w), int(x1 * w))
    if kind == "white":
        frame[ys, xs] = 255
    elif kind == "black":
        frame[ys, xs] = 0
    else:
        frame[ys, xs] = np.random.default_rng(seed).integers(0, 256, frame[ys, xs].shape, dtype=np.uint8)
    return frame


PLACES = [(0.30, 0.50), (0.70, 0.50)]
R = 0.19
KINDS = ("white", "black", "noise")


def _damaged_group(frame, m, seed, kinds=KINDS):
    if m == 2:
        return [_disc(frame.copy(), cx, cy, R, kinds[(seed + c) % len(kinds)], seed * 10 + c) for c, (cx, cy) in enumerate(PLACES)]
    return [_band(frame.copy(), c / m, (c + 1) / m, kinds[(seed + c) % len(kinds)], seed * 10 + c) for c in range(m)]


def _sym_mask(geo):
    return (1 << geo.CHUNKS_PER_FRAME) - 1 if geo.LEGACY else (1 << (geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA))) - 1


def _chunks_ok(geo, chunks, payload, mask):
    c = chunks.reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    p = payload.reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    return all((c[j] == p[j]).all() for j in range(geo.CHUNKS_PER_FRAME) if (int(mask) >> j) & 1)


# ---- stream helpers
def _stream(dec, batch, sizes, **kw):
    """the batch as stream calls of the given sizes, the last one flushed: the per-call results"""
    assert sum(sizes) == len(batch)
    out, lo = [], 0
    for c, size in enumerate(sizes):
        out.append(dec.decode_batch_combined_stream(batch[lo:lo + size], flush=c == len(sizes) - 1, **kw))
        lo += size
    return out


def _check_call_shape(res, n):
    """n + 1 group slots, zero from n_closed on"""
    ng, chunks, masks, groups, gchunks, gmasks, gsizes = res
    assert len(chunks) == len(masks) == len(groups) == n and len(gchunks) == len(gmasks) == len(gsizes) == n + 1
    assert 0 <= ng <= n + 1
    assert (gmasks[ng:] == 0).all() and (gchunks[ng:] == 0).all() and (gsizes[ng:] == 0).all()
    assert (gsizes[:ng] >= 1).all()


def _closed(results):
    """the closed groups of a sequence of calls, concatenated: (gsizes, gmasks, gchunks)"""
    return (np.concatenate([r[6][:r[0]] for r in results]), np.concatenate([r[5][:r[0]] for r in results]),
            np.concatenate([r[4][:r[0]] for r in results]))


# ---- 1. split equivalence
CUTS = [(k, 11 - k) for k in range(1, 11)] + [(1,) * 11, (2, 3, 4, 2)]


@pytest.fixture(scope="module")
def SPLIT_REF(MODE):
    geo = geometry.for_mode(MODE)
    frames, payload = _frames(MODE, 4, seed=700 + MODE)
    A, B, C, Dm = frames
    T = C.copy()
    T[:geo.IMG_H // 2] = B[:geo.IMG_H // 2]
    batch = np.stack([A, A, A, B, B, T, C, C, C] + _damaged_group(Dm, 2, 1))
    ref = D.HipDecoder(0, MODE)
    try:
        ng, chunks, masks, groups, gchunks, gmasks = ref.decode_batch_combined(batch)
        sym, col = ref.tap(D.TAP_SYMBOLS, len(batch)), ref.tap(D.TAP_COLORS, len(batch))
        ccm = ref.get_ccm()
    finally:
        ref.close()
    assert ng == 5 and groups.tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 3, 4, 4]
    sizes = np.bincount(groups[groups >= 0], minlength=ng)
    return dict(batch=batch, ng=ng, chunks=chunks, masks=masks, gchunks=gchunks, gmasks=gmasks, gsizes=sizes, sym=sym, col=col, ccm=ccm, payload=payload)


@pytest.mark.parametrize("cut", CUTS, ids=lambda c: "x".join(map(str, c)))
def test_split_equivalence(MODE, SPLIT_REF, cut):
    ref = SPLIT_REF
    dec = D.HipDecoder(0, MODE)
    try:
        res = _stream(dec, ref["batch"], cut)
        ccm = dec.get_ccm()
    finally:
        dec.close()
    starts = np.concatenate([[0], np.cumsum(cut)])
    model = SM.run([(ref["sym"][starts[c]:starts[c + 1]], ref["col"][starts[c]:starts[c + 1]], None) for c in range(len(cut))],
                   [False] * (len(cut) - 1) + [True])
    for c, r in enumerate(res):
        _check_call_shape(r, cut[c])
        assert r[3].tolist() == model[c][0].tolist(), (c, r[3], model[c][0])
        assert r[6][:r[0]].tolist() == model[c][2]
    gsizes, gmasks, gchunks = _closed(res)
    assert sum(r[0] for r in res) == ref["ng"]
    assert gsizes.tolist() == ref["gsizes"].tolist()
    assert (gmasks == ref["gmasks"][:ref["ng"]]).all()
    assert (gchunks == ref["gchunks"][:ref["ng"]]).all()
    assert (np.concatenate([r[1] for r in res]) == ref["chunks"]).all() and (np.concatenate([r[2] for r in res]) == ref["masks"]).all()
    assert ccm[0] == ref["ccm"][0] and np.array_equal(np.asarray(ccm[1]), np.asarray(ref["ccm"][1]))


# ---- 2. recovery across a boundary (and 5: the carry is a copy)
def _pair(mode):
    frames, payload = _frames(mode, 3, seed=300 + mode + 2)           # the frames of test_recovery_from_disjoint_damage[m = 2]
    return _damaged_group(frames[0], 2, 0), payload[0]


def test_recovery_across_a_call_boundary(MODE):
    geo = geometry.for_mode(MODE)
    pair, payload = _pair(MODE)
    dec, plain = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        first = dec.decode_batch_combined_stream(pair[0][None])
        _check_call_shape(first, 1)
        assert first[0] == 0 and first[3].tolist() == [D.GROUP_OPEN]
        second = dec.decode_batch_combined_stream(pair[1][None], flush=True)
        _check_call_shape(second, 1)
        assert second[0] == 1 and second[3].tolist() == [0] and second[6].tolist() == [2, 0]
        assert second[5][0] == geo.FULL_MASK, hex(int(second[5][0]))
        assert (second[4][0].reshape(-1) == payload).all()
        # what the feature replaces: the plain combined call, fed the same single captures, never sees the pair
        for k in range(2):
            ng, _, masks, groups, _, gmasks = plain.decode_batch_combined(pair[k][None])
            assert ng == 1 and groups.tolist() == [0]
            assert not (int(gmasks[0]) & _sym_mask(geo)) and not (int(masks[0]) & _sym_mask(geo))
    finally:
        dec.close()
        plain.close()


def test_the_carry_is_a_copy():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mode = 68
    geo = geometry.for_mode(mode)
    pair, _ = _pair(mode)
    others, _ = _frames(mode, 4, seed=909)
    quiet, busy = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        quiet.decode_batch_combined_stream(pair[0][None])
        want = quiet.decode_batch_combined_stream(pair[1][None], flush=True)
        first = busy.decode_batch_combined_stream(pair[0][None])
        assert first[3].tolist() == [D.GROUP_OPEN]
        busy.decode_batch(others)
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(others).to(dev)
        ch = torch.zeros((4, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
        mk = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        busy.decode_batch_pipelined(fr.data_ptr(), 4, ch.data_ptr(), mk.data_ptr())
        busy.pipeline_wait()
        torch.cuda.synchronize()
        got = busy.decode_batch_combined_stream(pair[1][None], flush=True)
        assert got[0] == want[0] == 1
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)
    finally:
        quiet.close()
        busy.close()


# ---- 3. model parity with a carried member
AGREE_3 = GW.AGREE_3   # per mille: below what two captures with a third of the frame damaged each share, 16 times what two different frames do


@pytest.mark.parametrize("cut", [(1, 2), (2, 1)], ids=["1x2", "2x1"])
def test_model_parity_with_a_carried_member(MODE, cut):
    geo = geometry.for_mode(MODE)
    frames, _ = _frames(MODE, 2, seed=200 + MODE)
    batch = np.stack(_damaged_group(frames[1], 3, 2))
    dec = D.HipDecoder(0, MODE)
    try:
        taps = {t: [] for t in (D.TAP_BITPLANE, D.TAP_SYMBOLS, D.TAP_COLORS, D.TAP_DRIFT, D.TAP_FLOOD_PATH)}
        lo = 0
        for c, size in enumerate(cut):
            res = dec.decode_batch_combined_stream(batch[lo:lo + size], flush=c == 1, min_agree_permille=AGREE_3)
            for t in taps:
                taps[t].append(dec.tap(t, size))
            lo += size
        planes, sym, col, drift, path = (np.concatenate(taps[t]) for t in (D.TAP_BITPLANE, D.TAP_SYMBOLS, D.TAP_COLORS, D.TAP_DRIFT, D.TAP_FLOOD_PATH))
        mutual = CM.agree(sym, col)
        assert (mutual * 1000 >= AGREE_3 * geo.NCELLS).all() and AGREE_3 * 64 >= 16 * 1000, (mutual, geo.NCELLS)
        assert res[0] == 1 and res[6].tolist()[0] == 3
        cells, margins = dec.tap(D.TAP_GROUP_CELLS, 1), dec.tap(D.TAP_GROUP_MARGIN, 1)
        mc, mm = CM.combine_cells(MODE, planes, sym, col, drift, path, [0, 1, 2], tiles=D.tile_hashes())
        assert (cells[0] == mc).all(), np.flatnonzero(cells[0] != mc)[:10]
        assert (margins[0] == mm).all(), np.flatnonzero(margins[0] != mm)[:10]
        assert int((mm != CM.MARGIN_NONE).sum()) > 100
    finally:
        dec.close()


# ---- 4. cap and unanimous skip
@pytest.mark.parametrize("cut", [(3, 3), (1,) * 6], ids=["3x3", "1x6"])
def test_cap_and_unanimous_groups(MODE, cut):
    geo = geometry.for_mode(MODE)
    frames, payload = _frames(MODE, 1, seed=400 + MODE)
    six = np.repeat(frames[:1], 6, axis=0)
    dec = D.HipDecoder(0, MODE)
    try:
        _, one_chunks, one_masks = D.HipDecoder(0, MODE).decode_batch(frames[:1])
        lo, closed_sizes, closing_call = 0, [], []
        # (no call that brings captures is flushed: what closes there closes by the cap; an empty flushed call ends the stream)
        for c, size in enumerate(cut + (0,)):
            res = dec.decode_batch_combined_stream(six[lo:lo + size] if size else None, flush=size == 0, max_group=4)
            _check_call_shape(res, size)
            for g in range(res[0]):
                closed_sizes.append(int(res[6][g]))
                closing_call.append(c)
                assert res[5][g] == one_masks[0] == geo.FULL_MASK
                assert (res[4][g] == one_chunks[0]).all() and (res[4][g].reshape(-1) == payload[0]).all()
            if res[0]:
                assert (dec.tap(D.TAP_GROUP_MARGIN, res[0]) == 0xFFFF).all()
            lo += size
        assert closed_sizes == [4, 2]
        # the full group is reported by the call that holds its fourth member, the rest by the flush
        assert closing_call == [int(np.searchsorted(np.cumsum(cut), 4)), len(cut)]
    finally:
        dec.close()


# ---- 6. parameters and edges
def test_parameters_and_edges():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mode = 68
    geo = geometry.for_mode(mode)
    frames, payload = _frames(mode, 2, seed=606)
    dec = D.HipDecoder(0, mode)
    try:
        res = dec.decode_batch_combined_stream(None, flush=True)                      # nothing open
        assert res[0] == 0 and len(res[4]) == 1 and (res[4] == 0).all() and (res[5] == 0).all() and (res[6] == 0).all()
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(None, flush=False)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(frames[:1], max_group=9)
        first = dec.decode_batch_combined_stream(frames[:1])                          # fixes 750 / 4
        assert first[0] == 0 and first[3].tolist() == [D.GROUP_OPEN]
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(frames[:1], max_group=3)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(frames[:1], min_agree_permille=500)
        dec.decode_batch_combined_stream(frames[:1], min_agree_permille=750, max_group=4)   # the same values spelled out
        dec.combine_stream_reset()                                                    # drops the two open captures and the parameters
        assert dec.decode_batch_combined_stream(None, flush=True, max_group=1)[0] == 0
        # max_group 1: every capture closes at once as a group of its own
        res = dec.decode_batch_combined_stream(np.stack([frames[0], frames[0], frames[1]]), max_group=1)
        assert res[0] == 3 and res[3].tolist() == [0, 1, 2] and res[6].tolist() == [1, 1, 1, 0]
        assert (res[5][:3] == geo.FULL_MASK).all()
        for g, k in enumerate((0, 0, 1)):
            assert (res[4][g].reshape(-1) == payload[k]).all()
        dec.combine_stream_reset()
        res = dec.decode_batch_combined_stream(frames[:1], min_agree_permille=500, max_group=3)   # accepted after the reset
        assert res[3].tolist() == [D.GROUP_OPEN]
        res = dec.decode_batch_combined_stream(None, flush=True, min_agree_permille=500, max_group=3)
        assert res[0] == 1 and res[6].tolist() == [1] and res[5][0] == geo.FULL_MASK
    finally:
        dec.close()


# ---- 7. capture path
@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path_blank_captures_and_recovery(fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mode = 68
    geo = geometry.for_mode(mode)
    frames, payload = _frames(mode, 2, seed=500 + fmt)
    quad = ((500, 40), (1480, 70), (470, 1030), (1500, 1000))
    cams = [F.camera_frame(f, quad=quad, background=96) for k in range(2) for f in _damaged_group(frames[k], 2, k, kinds=("white",))]
    blank = np.full_like(cams[0], 96)
    A1, A2, B1, B2, BL = (CF.rgb_to_format(c, fmt) for c in cams + [blank])
    dec = D.HipDecoder(0, mode)
    kw = dict(size=(1920, 1080), fmt=fmt)
    try:
        # one capture, nothing closes
        ng, _, masks, status, groups, _, _, _ = dec.scan_extract_decode_batch_combined_stream(np.stack([A1]), **kw)
        assert ng == 0 and status[0] > 0 and groups.tolist() == [D.GROUP_OPEN] and not (masks & _sym_mask(geo)).any()
        # its partner and a blank capture: the blank one, last of the call, closes the pair here -- recovery across the boundary
        ng, _, masks, status, groups, gchunks, gmasks, gsizes = dec.scan_extract_decode_batch_combined_stream(np.stack([A2, BL]), **kw)
        assert status[0] > 0 and status[1] <= 0 and not (masks & _sym_mask(geo)).any()
        assert ng == 1 and groups.tolist() == [0, -1] and gsizes.tolist() == [2, 0, 0]
        assert gmasks[0] == geo.FULL_MASK and _chunks_ok(geo, gchunks[0], payload[0], gmasks[0]) and (gmasks[1:] == 0).all()
        # a pair left open ...
        ng, _, _, _, groups, _, _, _ = dec.scan_extract_decode_batch_combined_stream(np.stack([B1, B2]), **kw)
        assert ng == 0 and groups.tolist() == [D.GROUP_OPEN] * 2
        # ... is closed by a blank capture that opens the next call
        ng, _, _, status, groups, gchunks, gmasks, gsizes = dec.scan_extract_decode_batch_combined_stream(np.stack([BL]), **kw)
        assert status[0] <= 0 and ng == 1 and groups.tolist() == [-1] and gsizes.tolist() == [2, 0]
        assert gmasks[0] == geo.FULL_MASK and _chunks_ok(geo, gchunks[0], payload[1], gmasks[0])
        assert dec.scan_extract_decode_batch_combined_stream(None, flush=True)[0] == 0
    finally:
        dec.close()


# ---- 8. device outputs
def test_device_outputs_match_host_outputs(MODE, SPLIT_REF):
    geo = geometry.for_mode(MODE)
    batch, cut = SPLIT_REF["batch"], (2, 3, 4, 2)
    host, dec = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        want = _stream(host, batch, cut)
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(batch).to(dev)
        outs = []
        for n in cut:
            outs.append(dict(chunks=torch.full((n, geo.FRAME_BYTES), 9, dtype=torch.uint8, device=dev), masks=torch.full((n,), 9, dtype=torch.int32, device=dev),
                             groups=torch.full((n,), 7, dtype=torch.int32, device=dev), gchunks=torch.full((n + 1, geo.FRAME_BYTES), 9, dtype=torch.uint8, device=dev),
                             gmasks=torch.full((n + 1,), 9, dtype=torch.int32, device=dev), gsizes=torch.full((n + 1,), 9, dtype=torch.int32, device=dev),
                             ng=torch.full((1,), 9, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize()
        lo = 0
        for c, n in enumerate(cut):
            o = outs[c]
            dec.decode_batch_combined_stream_device(fr[lo:lo + n].data_ptr(), n, o["chunks"].data_ptr(), o["masks"].data_ptr(), o["groups"].data_ptr(),
                                                    o["gchunks"].data_ptr(), o["gmasks"].data_ptr(), o["gsizes"].data_ptr(), o["ng"].data_ptr(),
                                                    flush=c == len(cut) - 1)
            lo += n
        torch.cuda.synchronize()
        for c, n in enumerate(cut):
            o, w = outs[c], want[c]
            assert int(o["ng"].item()) == w[0]
            assert (o["chunks"].cpu().numpy() == w[1].reshape(n, -1)).all() and (o["masks"].cpu().numpy().view(np.uint32) == w[2]).all()
            assert (o["groups"].cpu().numpy() == w[3]).all()
            assert (o["gchunks"].cpu().numpy() == w[4].reshape(n + 1, -1)).all() and (o["gmasks"].cpu().numpy().view(np.uint32) == w[5]).all()
            assert (o["gsizes"].cpu().numpy() == w[6]).all()
    finally:
        host.close()
        dec.close()


# ---- 9. erasure decoding on
@pytest.mark.parametrize("mode", [68, 67, 66])
def test_erasure_retry_across_calls(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    geo = geometry.for_mode(mode)
    agree = 200          # per mille: heavily damaged captures of one frame still share more, two different frames about 16
    enc, one, split = D.HipDecoder(0, mode), D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    one.set_erasure_decode(6)
    split.set_erasure_decode(6)
    try:
        payload = framegen.synth_payload(20, seed=600 + 10 * mode, mode=mode).numpy().reshape(20, -1)
        frames = enc.encode_batch(payload)
        g = np.random.default_rng(mode)
        caps = []
        for k in range(20):
            for c in range(2):
                f = frames[k].copy()
                for _ in range(2):
                    _disc(f, g.uniform(0.15, 0.85), g.uniform(0.15, 0.85), g.uniform(0.12, 0.24), KINDS[int(g.integers(0, 3))], int(g.integers(1 << 30)))
                caps.append(f)
        caps = np.stack(caps)
        ng, _, _, groups, gchunks, gmasks = one.decode_batch_combined(caps, min_agree_permille=agree)
        res = _stream(split, caps, (1, 3, 7, 2, 9, 5, 13), min_agree_permille=agree)      # cuts inside and between the pairs
        gsizes, smasks, schunks = _closed(res)
        assert sum(r[0] for r in res) == ng
        assert gsizes.tolist() == np.bincount(groups[groups >= 0], minlength=ng).tolist()
        assert (smasks == gmasks[:ng]).all() and (schunks == gchunks[:ng]).all()
        print(f"mode {mode}: {ng} groups of sizes {gsizes.tolist()}, {sum(bin(int(m)).count('1') for m in smasks)} chunks")
        for q in range(ng):
            frame = np.flatnonzero(groups == q) // 2
            assert (frame == frame[0]).all()            # (the reference's grouping never joins captures of two frames at this threshold)
            assert _chunks_ok(geo, schunks[q], payload[frame[0]], smasks[q]), q
    finally:
        enc.close()
        one.close()
        split.close()
