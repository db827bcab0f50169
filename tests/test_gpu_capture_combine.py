"""GPU: multi-capture decoding (cimbar_hip_decode_batch_combined / _scan_extract_decode_batch_combined_fmt), frames rendered from known
payloads, in every mode unless noted.

- Identity: groups of 1-4 copies of one frame give decode_batch's chunks and mask for that frame; the per-capture outputs and the carried
  colour-correction matrix equal decode_batch's on the same batch.
- Model parity: on damaged groups the group-cells, margin and groups taps equal tests/combine_model.py bit for bit.
- Recovery: two or three captures of a frame, each with a white, black or noise disc (three: band) at places the others leave clean,
  sized so that no capture alone delivers any symbol chunk (modes 4 / 8: any chunk): the group delivers every chunk, and every chunk in any gmask is the
  payload's.
- Grouping: A A A B B T C C C (T = B's top half over C's bottom half) -> 0 0 0 1 1 2 3 3 3; a run of 6 splits 4 + 2; groups_in is used as
  given; invalid groups_in and max_group > 8 are EINVAL; the device-output call matches the host-output one.
- Capture path: 1080p camera captures in formats 3 and 12 recover as above (white discs); a blank capture gets -1 and splits its neighbours.
- Erasure (modes 68 / 67 / 66): the group mask with erasure decoding on is a superset of the mask with it off; over 200 heavily damaged
  groups no wrong chunk enters a gmask.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from tests import capture_formats as CF
from tests import combine_model as CM
from tests import frames as F
from tests import group_walk_cases as GW

pytestmark = pytest.mark.gpu

MODES = [68, 67, 66, 4, 8]


@pytest.fixture(scope="module", params=MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


def _frames(mode, n, seed):
    payload = framegen.synth_payload(n, seed=seed, mode=mode)
    frames = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
    return frames, payload.numpy().reshape(n, -1)


# (the damage helpers live in tests/group_walk_cases.py, which builds its batches from them too)
_disc, _band, _damaged_group = GW.disc, GW.band, GW.damaged_group
PLACES, R, KINDS = GW.PLACES, GW.R, GW.KINDS


def _sym_mask(geo):
    return (1 << geo.CHUNKS_PER_FRAME) - 1 if geo.LEGACY else (1 << (geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA))) - 1


def _chunks_ok(geo, chunks, payload, mask):
    c = chunks.reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    p = payload.reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    return all((c[j] == p[j]).all() for j in range(geo.CHUNKS_PER_FRAME) if (int(mask) >> j) & 1)


def test_identity_groups_of_copies(MODE):
    geo = geometry.for_mode(MODE)
    frames, payload = _frames(MODE, 4, seed=100 + MODE)
    batch = np.concatenate([np.repeat(frames[k:k + 1], k + 1, axis=0) for k in range(4)])     # A, B B, C C C, D D D D
    ref = D.HipDecoder(0, MODE)
    dec = D.HipDecoder(0, MODE)
    try:
        _, rchunks, rmasks = ref.decode_batch(batch)
        rccm = ref.get_ccm()
        ng, chunks, masks, groups, gchunks, gmasks = dec.decode_batch_combined(batch)
        assert ng == 4
        assert groups.tolist() == [0, 1, 1, 2, 2, 2, 3, 3, 3, 3]
        assert (chunks == rchunks).all() and (masks == rmasks).all()
        assert dec.get_ccm()[0] == rccm[0] and np.array_equal(np.asarray(dec.get_ccm()[1]), np.asarray(rccm[1]))
        _, one_chunks, one_masks = D.HipDecoder(0, MODE).decode_batch(frames)
        for g in range(4):
            assert gmasks[g] == one_masks[g] == geo.FULL_MASK
            assert (gchunks[g] == one_chunks[g]).all()
            assert (gchunks[g].reshape(-1) == payload[g]).all()
        assert (gmasks[4:] == 0).all() and (gchunks[4:] == 0).all()
        cells = dec.tap(D.TAP_GROUP_CELLS, ng)
        sym, col = dec.tap(D.TAP_SYMBOLS, len(batch)), dec.tap(D.TAP_COLORS, len(batch))
        for g, k in enumerate((0, 1, 3, 6)):
            assert (cells[g] == ((col[k] << 4) | (sym[k] & 15))).all()
        assert (dec.tap(D.TAP_GROUP_MARGIN, ng) == 0xFFFF).all()
    finally:
        ref.close()
        dec.close()


def test_model_parity_on_damaged_groups(MODE):
    frames, _ = _frames(MODE, 3, seed=200 + MODE)
    batch = np.stack(_damaged_group(frames[0], 2, 1) + _damaged_group(frames[1], 3, 2) + [frames[2]])
    dec = D.HipDecoder(0, MODE)
    try:
        # (the three-capture group is given: each of its captures has a third of the frame damaged, so neighbours agree on less than 750 per mille)
        given = [0, 0, 1, 1, 1, 2]
        ng, _, _, groups, _, _ = dec.decode_batch_combined(batch, groups=given)
        n = len(batch)
        planes, sym, col = dec.tap(D.TAP_BITPLANE, n), dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)
        drift, path = dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_FLOOD_PATH, n)
        want = CM.group_captures(sym, col, groups_in=given)
        assert groups.tolist() == want.tolist() == given
        assert (dec.tap(D.TAP_GROUPS, n) == groups).all()
        cells, margins = dec.tap(D.TAP_GROUP_CELLS, ng), dec.tap(D.TAP_GROUP_MARGIN, ng)
        tiles = D.tile_hashes()
        disputed = 0
        for g in range(ng):
            mc, mm = CM.combine_cells(MODE, planes, sym, col, drift, path, CM.members(want, g), tiles=tiles)
            assert (cells[g] == mc).all(), (g, np.flatnonzero(cells[g] != mc)[:10])
            assert (margins[g] == mm).all(), (g, np.flatnonzero(margins[g] != mm)[:10])
            disputed += int((mm != CM.MARGIN_NONE).sum())
        assert disputed > 100
        # the device's own grouping of the same batch (the taps above describe the call before this one)
        auto = dec.decode_batch_combined(batch)[3]
        assert auto.tolist() == CM.group_captures(sym, col).tolist()
    finally:
        dec.close()


@pytest.mark.parametrize("m", [2, 3])
def test_recovery_from_disjoint_damage(MODE, m):
    geo = geometry.for_mode(MODE)
    frames, payload = _frames(MODE, 3, seed=300 + MODE + m)
    batch = np.stack([c for k in range(3) for c in _damaged_group(frames[k], m, k)])
    dec = D.HipDecoder(0, MODE)
    try:
        given = [g for g in range(3) for _ in range(m)]      # (three captures with a third of the frame damaged each agree on less than 750 per mille)
        ng, chunks, masks, groups, gchunks, gmasks = dec.decode_batch_combined(batch, groups=given if m == 3 else None)
        assert ng == 3 and groups.tolist() == given
        assert not (masks & _sym_mask(geo)).any(), masks          # no capture alone delivers a symbol chunk (legacy: any chunk)
        for g in range(3):
            assert gmasks[g] == geo.FULL_MASK, (g, hex(int(gmasks[g])))
            assert _chunks_ok(geo, gchunks[g], payload[g], gmasks[g])
    finally:
        dec.close()


def test_grouping_torn_capture_cap_and_groups_in(MODE):
    geo = geometry.for_mode(MODE)
    frames, payload = _frames(MODE, 3, seed=400 + MODE)
    A, B, C = frames
    T = C.copy()
    T[:geo.IMG_H // 2] = B[:geo.IMG_H // 2]
    batch = np.stack([A, A, A, B, B, T, C, C, C])
    dec = D.HipDecoder(0, MODE)
    try:
        ng, _, masks, groups, gchunks, gmasks = dec.decode_batch_combined(batch)
        assert groups.tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 3] and ng == 4
        for g, k in ((0, 0), (1, 1), (3, 2)):
            assert gmasks[g] == geo.FULL_MASK and (gchunks[g].reshape(-1) == payload[k]).all()
        six = np.repeat(A[None], 6, axis=0)
        ng, _, _, groups, _, _ = dec.decode_batch_combined(six, max_group=4)
        assert groups.tolist() == [0, 0, 0, 0, 1, 1] and ng == 2
        given = [0, 0, -1, 1, 2, 2, 2, 3, 3]
        ng, _, _, groups, _, gmasks = dec.decode_batch_combined(batch, groups=given)
        assert groups.tolist() == given and ng == 4 and (gmasks[4:] == 0).all()
        for bad in ([1] * 9, [0, 1, 0, 2, 2, 2, 3, 3, 3], [0] * 5 + [1] * 4):
            with pytest.raises(D.CimbarHipError, match="EINVAL"):
                dec.decode_batch_combined(batch, groups=bad)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined(batch, max_group=9)
        # device outputs: the same results, the group count written on the device, nothing synchronised by the call
        ref = dec.decode_batch_combined(batch)
        n = len(batch)
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(batch).to(dev)
        out = dict(chunks=torch.zeros((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev), masks=torch.zeros(n, dtype=torch.int32, device=dev),
                   groups=torch.full((n,), 7, dtype=torch.int32, device=dev), gchunks=torch.full((n, geo.FRAME_BYTES), 9, dtype=torch.uint8, device=dev),
                   gmasks=torch.full((n,), 9, dtype=torch.int32, device=dev), ng=torch.zeros(1, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        dec.decode_batch_combined_device(fr.data_ptr(), n, out["chunks"].data_ptr(), out["masks"].data_ptr(), out["groups"].data_ptr(),
                                         out["gchunks"].data_ptr(), out["gmasks"].data_ptr(), out["ng"].data_ptr())
        torch.cuda.synchronize()
        assert int(out["ng"].item()) == ref[0]
        assert (out["chunks"].cpu().numpy() == ref[1].reshape(n, -1)).all() and (out["masks"].cpu().numpy().view(np.uint32) == ref[2]).all()
        assert (out["groups"].cpu().numpy() == ref[3]).all()
        assert (out["gchunks"].cpu().numpy() == ref[4].reshape(n, -1)).all() and (out["gmasks"].cpu().numpy().view(np.uint32) == ref[5]).all()
    finally:
        dec.close()


@pytest.mark.parametrize("fmt", [3, 12])
def test_capture_path_recovery_and_blank_capture(fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mode = 68
    geo = geometry.for_mode(mode)
    frames, payload = _frames(mode, 2, seed=500 + fmt)
    quad = ((500, 40), (1480, 70), (470, 1030), (1500, 1000))
    cams = []
    for k in range(2):
        for f in _damaged_group(frames[k], 2, k, kinds=("white",)):     # (large black or noise discs can make the anchor search fail)
            cams.append(F.camera_frame(f, quad=quad, background=96))
    blank = np.full_like(cams[0], 96)
    cams = cams[:2] + [blank] + cams[2:]                      # A1 A2 blank B1 B2
    raw = np.stack([CF.rgb_to_format(c, fmt) for c in cams])
    dec = D.HipDecoder(0, mode)
    try:
        ng, chunks, masks, status, groups, gchunks, gmasks = dec.scan_extract_decode_batch_combined(raw, size=(1920, 1080), fmt=fmt)
        assert status[2] <= 0 and (status[[0, 1, 3, 4]] > 0).all(), status
        assert groups.tolist() == [0, 0, -1, 1, 1] and ng == 2
        _, pc, pm, pst = D.HipDecoder(0, mode).scan_extract_decode_batch(raw, size=(1920, 1080), fmt=fmt)
        assert (pc == chunks).all() and (pm == masks).all() and (pst == status).all()
        assert not (masks & _sym_mask(geo)).any(), masks
        for g in range(2):
            assert gmasks[g] == geo.FULL_MASK, (g, hex(int(gmasks[g])))
            assert _chunks_ok(geo, gchunks[g], payload[g], gmasks[g])
        # the blank capture between two captures of ONE frame still splits them
        ng, _, _, _, groups, _, _ = dec.scan_extract_decode_batch_combined(raw[[0, 2, 1]], size=(1920, 1080), fmt=fmt)
        assert groups.tolist() == [0, -1, 1] and ng == 2
    finally:
        dec.close()


@pytest.mark.parametrize("mode", [68, 67, 66])
def test_erasure_superset_and_no_wrong_chunk(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    geo = geometry.for_mode(mode)
    enc = D.HipDecoder(0, mode)
    off, on = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    on.set_erasure_decode(6)
    gained = wrong = groups_seen = 0
    try:
        for batch_no in range(2):
            payload = framegen.synth_payload(100, seed=600 + 10 * mode + batch_no, mode=mode).numpy().reshape(100, -1)
            frames = enc.encode_batch(payload)
            g = np.random.default_rng(batch_no + mode)
            caps = []
            for k in range(100):
                for c in range(2):
                    f = frames[k].copy()
                    for _ in range(2):
                        _disc(f, g.uniform(0.15, 0.85), g.uniform(0.15, 0.85), g.uniform(0.12, 0.24), KINDS[int(g.integers(0, 3))], int(g.integers(1 << 30)))
                    caps.append(f)
            caps = np.stack(caps)
            groups = np.repeat(np.arange(100), 2)
            r_off = off.decode_batch_combined(caps, groups=groups)
            r_on = on.decode_batch_combined(caps, groups=groups)
            assert r_off[0] == r_on[0] == 100
            m_off, m_on = r_off[5][:100], r_on[5][:100]
            assert ((m_off & ~m_on) == 0).all()
            for k in range(100):
                wrong += not _chunks_ok(geo, r_on[4][k], payload[k], m_on[k])
                wrong += not _chunks_ok(geo, r_off[4][k], payload[k], m_off[k])
                gained += bin(int(m_on[k]) & ~int(m_off[k])).count("1")
            groups_seen += 100
        print(f"mode {mode}: {groups_seen} groups, erasure retry added {gained} chunks")
        assert wrong == 0
    finally:
        enc.close()
        off.close()
        on.close()
