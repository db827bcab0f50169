"""GPU: the colour vote of the group decode and the group colour retry (cimbar_hip_set_group_colour_vote -> k_group_colour,
k_group_colour_retry), modes 68 / 67 / 66, against tests/group_colour_model.py fed from the call's own per-capture taps.

1. Device equals model: with the setting on, the colour nibble of TAP_GROUP_CELLS, TAP_GROUP_COLOUR_MARGIN, TAP_GROUP_COLOUR_WEIGHTS, gchunks and
   gmasks equal the model bit for bit on a batch of a pair with disjoint discs, a triple with one damaged member, a pair of identical
   captures (skipped: no margin, outputs equal to the setting-off call) and a capture in no group; one member of each damaged group took
   the flood pass (TAP_FLOOD). Every mode.
2. Off is off: the same batch with the setting off before and after an on-call on one context gives what a fresh context gives; the two taps
   are EINVAL.
3. Only colour moves: on against off, the symbol nibble of the group cells, the symbol margin, the per-capture chunks / masks and the symbol
   bits of gmask are equal; a colour nibble differs only where the members' colours differ.
4. Retry: the crafted pair of group_colour_cases (chosen on the CPU: tests/test_group_colour_model.py) -- neither member's own colour retry delivers the colour chunk, the
   group lacks it after the vote, the retry delivers it equal to the payload; with six more flagged bytes than parity - 8 it stays lost and unwritten.
5. Capture path: four small captures (two groups of two, format 3) equal the model fed from that call's taps; a blank capture is in no group
   and contributes no weight.
6. Arguments: modes 4 / 8 refuse it, the getter round-trips, the stream calls give identical outputs with the setting on and off.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import capture_formats as CF
from tests import colour_erasure_model as CE
from tests import frames as F
from tests import group_colour_cases as GC
from tests import group_colour_model as GM

pytestmark = pytest.mark.gpu

CORNER_MODE = 66          # the smallest frame: the corner cases run there


@pytest.fixture(scope="module", params=GC.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _batch(mode):
    """pair (disjoint white / washed discs, member 1 shifted), triple (member 1 noise-damaged and shifted), two identical captures, a single
    capture given as in no group -> (captures, payload per group, groups_in)"""
    fr, payload = GC.K.frames(mode, 4, 81 + mode)
    shape = fr[0].shape
    a = GC.damage(fr[0].copy(), GC.disc(shape, 0.32, 0.45, 0.09), "washed", 1)
    b = F.shift(GC.damage(fr[0].copy(), GC.disc(shape, 0.68, 0.55, 0.08), "white", 2), 1, 0)
    t1 = F.shift(GC.damage(fr[1].copy(), GC.disc(shape, 0.5, 0.5, 0.10), "noise", 3), 1, 0)
    caps = np.stack([a, b, fr[1], t1, fr[1], fr[2], fr[2], fr[3]])
    return caps, payload, [0, 0, 1, 1, 1, 2, 2, -1]


def _model(geo, caps, dec, n, ng, groups, chunks, masks, colour_margin=0):
    """the model over the taps of the call `dec` just made -> per group (colour nibble or None where skipped, gm, weights by capture), gmasks, gchunks"""
    col, drift, ccm = dec.tap(D.TAP_COLORS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_CCM, n)
    sym = dec.tap(D.TAP_SYMBOLS, n)
    cells = dec.tap(D.TAP_GROUP_CELLS, ng)
    xy = geo.cell_positions().astype(np.int64)
    want_gm = np.full((ng, geo.NCELLS), GM.NONE, np.uint32)
    want_w = np.zeros((n, geo.NCELLS), np.uint32)
    want_col = [None] * ng
    want_mask, want_chunks = np.zeros(ng, np.uint32), np.zeros((ng, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    ch = np.asarray(chunks).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    for g in range(ng):
        mem = [k for k in range(n) if groups[k] == g]
        cols = np.stack([col[k] for k in mem])
        syms = np.stack([sym[k] & 15 for k in mem])
        disputed = bool((cols != cols[0]).any() or (syms != syms[0]).any())
        vc, gm = cols[0], None
        if disputed:
            mgs = np.stack([CE.margins(CE.cell_means(caps[k], xy + drift[k].astype(np.int64)), ccm[k]) for k in mem])
            vc, gm, w = GM.vote(cols, mgs)
            want_gm[g], want_col[g] = gm, vc
            for c, k in enumerate(mem):
                want_w[k] = w[c]
        m, c, _ = GM.decode_group(geo, cells[g] & 15, vc, gm, [masks[k] for k in mem], [ch[k] for k in mem], disputed, colour_margin=colour_margin)
        want_mask[g], want_chunks[g] = m, c
    return want_col, want_gm, want_w, want_mask, want_chunks


def _compare(geo, dec, n, ng, gchunks, gmasks, model):
    want_col, want_gm, want_w, want_mask, want_chunks = model
    cells = dec.tap(D.TAP_GROUP_CELLS, ng)
    tap_gm, tap_w = dec.tap(D.TAP_GROUP_COLOUR_MARGIN, ng), dec.tap(D.TAP_GROUP_COLOUR_WEIGHTS, n)
    for g in range(ng):
        if want_col[g] is not None:
            assert ((cells[g] >> 4) == want_col[g]).all(), (g, np.flatnonzero((cells[g] >> 4) != want_col[g])[:10])
        assert (tap_gm[g] == want_gm[g]).all(), (g, np.flatnonzero(tap_gm[g] != want_gm[g])[:10])
    assert (tap_w == want_w).all(), np.argwhere(tap_w != want_w)[:10]
    assert (gmasks[:ng].astype(np.uint32) == want_mask).all(), (gmasks[:ng], want_mask)
    assert (np.asarray(gchunks)[:ng].reshape(ng, geo.CHUNKS_PER_FRAME, geo.CHUNK) == want_chunks).all()


def test_device_equals_model(MODE):
    geo = geometry.for_mode(MODE)
    caps, payload, given = _batch(MODE)
    n = len(caps)
    off, dec = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        r0 = off.decode_batch_combined(caps, groups=given)
        dec.set_group_colour_vote(True)
        ng, chunks, masks, groups, gchunks, gmasks = dec.decode_batch_combined(caps, groups=given)
        assert ng == 3 and groups.tolist() == given
        flood = dec.tap(D.TAP_FLOOD, n)
        assert flood[1] and flood[3] and not flood[0] and not flood[2], flood
        model = _model(geo, caps, dec, n, ng, given, chunks, masks)
        disputed = [int((model[1][g] != GM.NONE).sum()) for g in range(ng)]
        print(f"mode {MODE}: colour-disputed cells per group {disputed}")
        assert disputed[0] > 50 and disputed[1] > 50 and disputed[2] == 0
        _compare(geo, dec, n, ng, gchunks, gmasks, model)
        # the group of identical captures is skipped: no margin, no weight, the setting-off outputs
        assert (dec.tap(D.TAP_GROUP_COLOUR_MARGIN, ng)[2] == GM.NONE).all()
        assert not dec.tap(D.TAP_GROUP_COLOUR_WEIGHTS, n)[5:].any()
        assert gmasks[2] == r0[5][2] and (gchunks[2] == r0[4][2]).all()
        p = payload.reshape(len(payload), geo.CHUNKS_PER_FRAME, geo.CHUNK)
        gc = np.asarray(gchunks).reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        for g in range(ng):
            for j in range(geo.CHUNKS_PER_FRAME):
                if (int(gmasks[g]) >> j) & 1:
                    assert (gc[g, j] == p[g, j]).all(), (g, j)
    finally:
        off.close()
        dec.close()


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_off_is_off(gpu):
    caps, _, given = _batch(CORNER_MODE)
    fresh, dec = D.HipDecoder(0, CORNER_MODE), D.HipDecoder(0, CORNER_MODE)
    try:
        want = fresh.decode_batch_combined(caps, groups=given)
        want_cells, want_margin = fresh.tap(D.TAP_GROUP_CELLS, want[0]), fresh.tap(D.TAP_GROUP_MARGIN, want[0])
        assert dec.get_group_colour_vote() is False
        before = dec.decode_batch_combined(caps, groups=given)
        for what in (D.TAP_GROUP_COLOUR_MARGIN, D.TAP_GROUP_COLOUR_WEIGHTS):
            with pytest.raises(D.CimbarHipError, match="EINVAL"):
                dec.tap(what, want[0])
        dec.set_group_colour_vote(True)
        dec.decode_batch_combined(caps, groups=given)
        dec.tap(D.TAP_GROUP_COLOUR_MARGIN, want[0])
        dec.set_group_colour_vote(False)
        after = dec.decode_batch_combined(caps, groups=given)
        assert _same(before, want) and _same(after, want)
        assert (dec.tap(D.TAP_GROUP_CELLS, want[0]) == want_cells).all() and (dec.tap(D.TAP_GROUP_MARGIN, want[0]) == want_margin).all()
        for what in (D.TAP_GROUP_COLOUR_MARGIN, D.TAP_GROUP_COLOUR_WEIGHTS):
            with pytest.raises(D.CimbarHipError, match="EINVAL"):
                dec.tap(what, want[0])
    finally:
        fresh.close()
        dec.close()


def test_only_colour_moves(gpu):
    geo = geometry.for_mode(CORNER_MODE)
    caps, _, given = _batch(CORNER_MODE)
    n = len(caps)
    off, on = D.HipDecoder(0, CORNER_MODE), D.HipDecoder(0, CORNER_MODE)
    try:
        on.set_group_colour_vote(True)
        r0, r1 = off.decode_batch_combined(caps, groups=given), on.decode_batch_combined(caps, groups=given)
        ng = r0[0]
        c0, c1 = off.tap(D.TAP_GROUP_CELLS, ng), on.tap(D.TAP_GROUP_CELLS, ng)
        assert ((c0 & 15) == (c1 & 15)).all()
        assert (off.tap(D.TAP_GROUP_MARGIN, ng) == on.tap(D.TAP_GROUP_MARGIN, ng)).all()
        assert r0[0] == r1[0] and _same(r0[1:4], r1[1:4])
        symbits = (1 << GC.K.sym_chunks(geo)) - 1
        assert ((r0[5].astype(np.uint32) ^ r1[5].astype(np.uint32)) & symbits == 0).all()
        col = on.tap(D.TAP_COLORS, n)
        moved = 0
        for g in range(ng):
            mem = [k for k in range(n) if given[k] == g]
            agreed = (col[mem] == col[mem[0]]).all(axis=0)
            assert ((c0[g] >> 4) == (c1[g] >> 4))[agreed].all()
            moved += int(((c0[g] >> 4) != (c1[g] >> 4)).sum())
        print(f"mode {CORNER_MODE}: the vote changed the colour of {moved} cells")
    finally:
        off.close()
        on.close()


def test_retry_recovers_crafted_pair_and_overload_stays_lost(gpu):
    mode = CORNER_MODE
    geo = geometry.for_mode(mode)
    fr, payload = GC.K.frames(mode, 2, 71)
    true = GC.true_colours(mode, payload)
    e_max = geo.RS_PARITY - 8
    symc = GC.K.sym_chunks(geo)
    a0, b0, _ = GC.crafted_pair(mode, fr[0], true[0], e_max, extra=6)
    a1, b1, _ = GC.crafted_pair(mode, fr[1], true[1], e_max + 6)
    caps = np.stack([a0, b0, a1, b1])
    given = [0, 0, 1, 1]
    vote, dec = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        vote.set_group_colour_vote(True)
        rv = vote.decode_batch_combined(caps, groups=given, color_correction=0)
        dec.set_group_colour_vote(True)
        dec.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)
        ng, chunks, masks, groups, gchunks, gmasks = dec.decode_batch_combined(caps, groups=given, color_correction=0)
        assert ng == 2
        assert not ((masks >> symc) & 1).any(), "a member delivers the chunk alone"
        assert not ((rv[5][:2] >> symc) & 1).any(), "the vote alone delivers the chunk"
        model = _model(geo, caps, dec, 4, ng, given, chunks, masks, colour_margin=D.COLOUR_MARGIN_SUGGESTED)
        assert (int(model[3][0]) >> symc) & 1 and not (int(model[3][1]) >> symc) & 1, "the model's retry must recover group 0's chunk and not group 1's"
        _compare(geo, dec, 4, ng, gchunks, gmasks, model)
        gc = np.asarray(gchunks).reshape(4, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        assert (int(gmasks[0]) >> symc) & 1 and (gc[0, symc] == payload[0].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[symc]).all()
        assert not (int(gmasks[1]) >> symc) & 1 and not gc[1, symc].any()
        # chunks the vote-only call had are the same bytes
        for g in range(2):
            for j in range(geo.CHUNKS_PER_FRAME):
                if (int(rv[5][g]) >> j) & 1:
                    assert (gc[g, j] == np.asarray(rv[4]).reshape(4, geo.CHUNKS_PER_FRAME, geo.CHUNK)[g, j]).all()
    finally:
        vote.close()
        dec.close()


def test_capture_path_equals_model(gpu):
    mode = CORNER_MODE
    geo = geometry.for_mode(mode)
    fr, payload = GC.K.frames(mode, 2, 91)
    size = (1280, 720)
    quad = ((270, 20), (1010, 30), (260, 690), (1020, 680))
    cams = []
    for k in range(2):
        for c, cx in enumerate((0.35, 0.65)):
            f = GC.damage(fr[k].copy(), GC.disc(fr[k].shape, cx, 0.5, 0.08), "washed", k)
            cams.append(F.camera_frame(f, width=size[0], height=size[1], quad=quad, background=96))
    cams.insert(2, np.full_like(cams[0], 96))                    # A1 A2 blank B1 B2
    raw = np.stack([CF.rgb_to_format(c, 3) for c in cams])
    dec, other = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        # the frames the call decodes: the same captures through the extractor alone (on another context)
        _, _, ext = other.extract_batch(raw, size=size, fmt=3)
        dec.set_group_colour_vote(True)
        ng, chunks, masks, status, groups, gchunks, gmasks = dec.scan_extract_decode_batch_combined(raw, size=size, fmt=3, preprocess=0)
        assert status[2] <= 0 and (status[[0, 1, 3, 4]] > 0).all(), status
        assert groups.tolist() == [0, 0, -1, 1, 1] and ng == 2
        model = _model(geo, ext, dec, 5, ng, groups.tolist(), chunks, masks)
        assert (model[1] != GM.NONE).sum() > 20
        _compare(geo, dec, 5, ng, gchunks, gmasks, model)
        assert not dec.tap(D.TAP_GROUP_COLOUR_WEIGHTS, 5)[2].any()
    finally:
        dec.close()
        other.close()


@pytest.mark.parametrize("legacy", [4, 8])
def test_refused_in_legacy_modes(gpu, legacy):
    dec = D.HipDecoder(0, legacy)
    try:
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.set_group_colour_vote(True)
        dec.set_group_colour_vote(False)
        assert dec.get_group_colour_vote() is False
    finally:
        dec.close()


def test_getter_and_stream_calls_unaffected(gpu):
    caps, _, _ = _batch(CORNER_MODE)
    off, on = D.HipDecoder(0, CORNER_MODE), D.HipDecoder(0, CORNER_MODE)
    try:
        assert on.get_group_colour_vote() is False
        on.set_group_colour_vote(True)
        assert on.get_group_colour_vote() is True
        on.set_group_colour_vote(False)
        assert on.get_group_colour_vote() is False
        on.set_group_colour_vote(True)
        for lo, hi, flush in ((0, 3, False), (3, 8, True)):
            r0 = off.decode_batch_combined_stream(caps[lo:hi], flush=flush)
            r1 = on.decode_batch_combined_stream(caps[lo:hi], flush=flush)
            assert _same(r0, r1)
            assert (off.tap(D.TAP_GROUP_CELLS, max(r0[0], 1)) == on.tap(D.TAP_GROUP_CELLS, max(r1[0], 1))).all()
            with pytest.raises(D.CimbarHipError, match="EINVAL"):
                on.tap(D.TAP_GROUP_COLOUR_MARGIN, max(r1[0], 1))
    finally:
        off.close()
        on.close()
