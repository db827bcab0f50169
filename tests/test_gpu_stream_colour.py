"""GPU: the colour vote in the stream calls (cimbar_hip_set_stream_colour_vote -> k_group_colour_stream, k_group_carry_weights, k_group_colour_retry),
modes 68 / 67 / 66 unless noted. The reference is existing code, pinned to its model by tests/test_gpu_group_colour.py: ONE plain combined call
with cimbar_hip_set_group_colour_vote on over the concatenation of the captures. Fresh contexts per comparison.

1. Split equivalence: group_colour_cases.pair_set followed by the triple and the identical pair of test_gpu_group_colour._batch (17 captures, the
   device groups them), cut into one capture per call, into two calls inside a pair / between two groups / inside the triple, and into
   (2, 3, 4, rest): the closed groups' gsizes, gmasks, gchunks, colour nibbles and colour-margin taps, concatenated, equal the reference's; the
   weights tap of every call holds the reference's rows of the captures whose group closed in it and 0 elsewhere; per-capture chunks, masks
   and the carried matrix are unchanged. Fed one per call the triple keeps member 0 in slot 0 over three calls.
2. Recovery across a call boundary: pair_set one capture per call -- with the setting on group 4 (the largest washed disc) has every chunk,
   equal to the payload; on a context with only cimbar_hip_set_group_colour_vote on it has no colour chunk, as before this setting existed.
3. Carry weights: after a call that leaves a two-member group open, one member from the flood pass, TAP_STREAM_CARRY_WEIGHTS equals margins + 1
   over all cells, the margins from that call's TAP_DRIFT / TAP_CCM; the same one capture per call.
4. Retry across calls (mode 66): the crafted pair one capture per call with colour erasure on: parity - 8 touched bytes are recovered, six
   more stay lost and unwritten; both as the plain vote-on call reports them.
5. Off is off (mode 66): set and cleared before the first call is a fresh context; the three taps are EINVAL.
6. Arguments: modes 4 / 8 refuse it; the getter; a toggle in mid-stream is EINVAL and leaves the carry intact; reset accepts the other value.
7. Device outputs (mode 66): (2, 3, 4, rest) with poisoned buffers and no synchronise between the calls equals the host-output run.
8. Capture path (format 3): A1 A2 blank B1 B2 as (2, 3) and one per call equals scan_extract_decode_batch_combined with the plain vote on.
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

pytestmark = pytest.mark.gpu

CORNER_MODE = 66
WANT_GROUPS = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 7, 7]
CUTS = [(1,) * 17, (5, 12), (6, 11), (14, 3), (2, 3, 4, 8)]


@pytest.fixture(scope="module", params=GC.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _triple_and_twins(mode):
    """the triple (member 1 noise-damaged and shifted: the flood pass) and the two identical captures of test_gpu_group_colour._batch"""
    fr, _ = GC.K.frames(mode, 4, 81 + mode)
    t1 = F.shift(GC.damage(fr[1].copy(), GC.disc(fr[1].shape, 0.5, 0.5, 0.10), "noise", 3), 1, 0)
    return [fr[1], t1, fr[1]], [fr[2], fr[2]]


def _stream(dec, caps, cut, **kw):
    """the captures as stream calls of the given sizes, the last one flushed, with the colour taps of every call -> the closed groups
    concatenated, the per-capture outputs concatenated, and the per-call results"""
    assert sum(cut) == len(caps)
    geo = dec.geo
    calls, lo = [], 0
    closed = dict(gsizes=[], gmasks=[], gchunks=[], col=[], gm=[])
    weights = []
    for c, n in enumerate(cut):
        r = dec.decode_batch_combined_stream(caps[lo:lo + n], flush=c == len(cut) - 1, **kw)
        ng = r[0]
        assert (r[5][ng:] == 0).all() and (r[4][ng:] == 0).all() and (r[6][ng:] == 0).all()
        closed["gsizes"].append(r[6][:ng]); closed["gmasks"].append(r[5][:ng]); closed["gchunks"].append(r[4][:ng])
        if ng:
            closed["col"].append(dec.tap(D.TAP_GROUP_CELLS, ng) >> 4)
            closed["gm"].append(dec.tap(D.TAP_GROUP_COLOUR_MARGIN, ng))
        weights.append(dec.tap(D.TAP_GROUP_COLOUR_WEIGHTS, n))
        calls.append(r)
        lo += n
    empty = {"col": np.zeros((0, geo.NCELLS), np.uint8), "gm": np.zeros((0, geo.NCELLS), np.uint32)}
    out = {k: np.concatenate(v) if v else empty[k] for k, v in closed.items()}
    out.update(chunks=np.concatenate([r[1] for r in calls]), masks=np.concatenate([r[2] for r in calls]),
               groups=[r[3] for r in calls], weights=weights, calls=calls)
    return out


def _reference(mode, caps, colour_margin=0, **kw):
    """the plain vote-on call over all captures"""
    ref = D.HipDecoder(0, mode)
    try:
        ref.set_group_colour_vote(True)
        if colour_margin:
            ref.set_colour_erasure_decode(colour_margin)
        ng, chunks, masks, groups, gchunks, gmasks = ref.decode_batch_combined(caps, **kw)
        n = len(caps)
        return dict(ng=ng, chunks=chunks, masks=masks, groups=groups, gchunks=gchunks[:ng], gmasks=gmasks[:ng],
                    gsizes=np.bincount(groups[groups >= 0], minlength=ng), col=ref.tap(D.TAP_GROUP_CELLS, ng) >> 4,
                    gm=ref.tap(D.TAP_GROUP_COLOUR_MARGIN, ng), weights=ref.tap(D.TAP_GROUP_COLOUR_WEIGHTS, n), flood=ref.tap(D.TAP_FLOOD, n),
                    ccm=ref.get_ccm())
    finally:
        ref.close()


def _same_groups(got, ref):
    assert got["gsizes"].tolist() == ref["gsizes"].tolist(), (got["gsizes"], ref["gsizes"])
    assert (got["gmasks"] == ref["gmasks"]).all(), (got["gmasks"], ref["gmasks"])
    assert (got["gchunks"] == ref["gchunks"]).all()
    assert (got["col"] == ref["col"]).all(), np.argwhere(got["col"] != ref["col"])[:10]
    assert (got["gm"] == ref["gm"]).all(), np.argwhere(got["gm"] != ref["gm"])[:10]


# ---- 1. split equivalence
@pytest.fixture(scope="module")
def SPLIT_REF(MODE):
    pairs, payload, _ = GC.pair_set(MODE)
    triple, twins = _triple_and_twins(MODE)
    caps = np.concatenate([pairs, np.stack(triple + twins)])
    ref = _reference(MODE, caps)
    # the device finds the intended groups by itself, and the triple's member 1 took the flood pass: carried, its weights come from mean6x6
    assert ref["groups"].tolist() == WANT_GROUPS and ref["ng"] == 8, ref["groups"]
    assert ref["flood"][13] and not ref["flood"][12], ref["flood"]
    disputed = [int((ref["gm"][g] != 0xFFFFFFFF).sum()) for g in range(8)]
    print(f"mode {MODE}: colour-disputed cells per group {disputed}")
    assert min(disputed[:7]) > 20 and disputed[7] == 0
    ref.update(caps=caps, payload=payload)
    return ref


@pytest.mark.parametrize("cut", CUTS, ids=lambda c: "x".join(map(str, c)) if len(c) < 17 else "1x17")
def test_split_equivalence(MODE, SPLIT_REF, cut):
    ref = SPLIT_REF
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_stream_colour_vote(True)
        got = _stream(dec, ref["caps"], cut)
        ccm = dec.get_ccm()
    finally:
        dec.close()
    _same_groups(got, ref)
    assert (got["chunks"] == ref["chunks"]).all() and (got["masks"] == ref["masks"]).all()
    assert ccm[0] == ref["ccm"][0] and np.array_equal(np.asarray(ccm[1]), np.asarray(ref["ccm"][1]))
    lo = 0
    for c, n in enumerate(cut):
        want = np.where((got["groups"][c] >= 0)[:, None], ref["weights"][lo:lo + n], 0)
        assert (got["weights"][c] == want).all(), (c, np.argwhere(got["weights"][c] != want)[:10])
        lo += n
    if len(cut) == 17:
        # the triple: member 0 opens the group in call 12 and stays in slot 0 through calls 13 and 14; the first twin closes it in call 15
        assert [g.tolist() for g in got["groups"][12:16]] == [[D.GROUP_OPEN]] * 4
        assert [r[0] for r in got["calls"][12:16]] == [1, 0, 0, 1] and got["calls"][15][6][0] == 3


# ---- 2. recovery across a call boundary
def test_recovery_across_a_call_boundary(MODE):
    geo = geometry.for_mode(MODE)
    caps, payload, _ = GC.pair_set(MODE)
    symc = GC.K.sym_chunks(geo)
    on, plain_only = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        on.set_stream_colour_vote(True)
        plain_only.set_group_colour_vote(True)
        masks = {}
        for name, dec in (("on", on), ("plain", plain_only)):
            closed_masks, closed_chunks = [], []
            for k in range(len(caps)):
                r = dec.decode_batch_combined_stream(caps[k:k + 1], flush=k == len(caps) - 1)
                closed_masks += r[5][:r[0]].tolist()
                closed_chunks += list(r[4][:r[0]])
            assert len(closed_masks) == 6
            masks[name] = (closed_masks, closed_chunks)
        print(f"mode {MODE}: group masks, stream vote on {[hex(m) for m in masks['on'][0]]}, off {[hex(m) for m in masks['plain'][0]]}")
        assert masks["on"][0][4] == geo.FULL_MASK, hex(masks["on"][0][4])
        assert (masks["on"][1][4].reshape(-1) == np.asarray(payload[4]).reshape(-1)).all()
        # today's behaviour, which stays: the plain calls' setting does not reach the stream calls, and the plurality colour loses the frame
        assert masks["plain"][0][4] >> symc == 0, hex(masks["plain"][0][4])
    finally:
        on.close()
        plain_only.close()


# ---- 3. carry weights
def _want_weights(geo, dec, caps):
    n = len(caps)
    drift, ccm = dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_CCM, n)
    xy = geo.cell_positions().astype(np.int64)
    return np.stack([CE.margins(CE.cell_means(caps[k], xy + drift[k].astype(np.int64)), ccm[k]).astype(np.int64) + 1 for k in range(n)]).astype(np.uint32)


def test_carry_weights(MODE):
    geo = geometry.for_mode(MODE)
    triple, _ = _triple_and_twins(MODE)
    two = np.stack(triple[:2])
    dec, single = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        dec.set_stream_colour_vote(True)
        r = dec.decode_batch_combined_stream(two)
        assert r[0] == 0 and r[3].tolist() == [D.GROUP_OPEN] * 2
        flood = dec.tap(D.TAP_FLOOD, 2)
        assert flood[1] and not flood[0], flood
        want = _want_weights(geo, dec, two)
        got = dec.tap(D.TAP_STREAM_CARRY_WEIGHTS, 2)
        assert (got == want).all(), np.argwhere(got != want)[:10]
        assert (got >= 1).all()
        assert (dec.tap(D.TAP_STREAM_CARRY_WEIGHTS, 1) == want[:1]).all()
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.tap(D.TAP_STREAM_CARRY_WEIGHTS, 3)
        # nothing closed: no group margin rows, and no capture gave a weight to a closed group
        assert not dec.tap(D.TAP_GROUP_COLOUR_WEIGHTS, 2).any()
        # one capture per call: slot 0 keeps its row when slot 1 arrives
        single.set_stream_colour_vote(True)
        single.decode_batch_combined_stream(two[:1])
        assert (single.tap(D.TAP_STREAM_CARRY_WEIGHTS, 1) == want[:1]).all()
        single.decode_batch_combined_stream(two[1:])
        assert (single.tap(D.TAP_STREAM_CARRY_WEIGHTS, 2) == want).all()
        # a flush empties the store
        assert single.decode_batch_combined_stream(None, flush=True)[0] == 1
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            single.tap(D.TAP_STREAM_CARRY_WEIGHTS, 1)
    finally:
        dec.close()
        single.close()


# ---- 4. retry across calls
@pytest.mark.parametrize("over", [0, 6], ids=["at-the-limit", "six-more"])
def test_retry_across_calls(gpu, over):
    mode = CORNER_MODE
    geo = geometry.for_mode(mode)
    fr, payload = GC.K.frames(mode, 2, 71)
    true = GC.true_colours(mode, payload)
    symc = GC.K.sym_chunks(geo)
    count = geo.RS_PARITY - 8 + over
    a, b, _ = GC.crafted_pair(mode, fr[0], true[0], count, extra=0 if over else 6)
    pair = np.stack([a, b])
    ref = _reference(mode, pair, colour_margin=D.COLOUR_MARGIN_SUGGESTED, color_correction=0)
    assert ref["ng"] == 1 and ref["groups"].tolist() == [0, 0]
    dec = D.HipDecoder(0, mode)
    try:
        dec.set_stream_colour_vote(True)
        dec.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)
        got = _stream(dec, pair, (1, 1), color_correction=0)
    finally:
        dec.close()
    assert not ((got["masks"] >> symc) & 1).any(), "a member delivers the chunk alone"
    _same_groups(got, ref)
    gmask, gchunks = int(got["gmasks"][0]), got["gchunks"][0].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    if over:
        assert not (gmask >> symc) & 1 and not gchunks[symc].any()
    else:
        assert (gmask >> symc) & 1 and (gchunks[symc] == payload[0].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[symc]).all()


# ---- 5. off is off
def test_off_is_off(gpu):
    mode = CORNER_MODE
    triple, twins = _triple_and_twins(mode)
    caps = np.concatenate([GC.pair_set(mode)[0][8:10], np.stack(triple + twins)])
    fresh, dec = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        assert dec.get_stream_colour_vote() is False
        dec.set_stream_colour_vote(True)
        dec.set_stream_colour_vote(False)
        lo = 0
        for c, n in enumerate((3, 4)):
            want = fresh.decode_batch_combined_stream(caps[lo:lo + n], flush=c == 1)
            got = dec.decode_batch_combined_stream(caps[lo:lo + n], flush=c == 1)
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(want, got))
            ng = max(want[0], 1)
            assert (fresh.tap(D.TAP_GROUP_CELLS, ng) == dec.tap(D.TAP_GROUP_CELLS, ng)).all()
            for d in (fresh, dec):
                for what in (D.TAP_GROUP_COLOUR_MARGIN, D.TAP_GROUP_COLOUR_WEIGHTS, D.TAP_STREAM_CARRY_WEIGHTS):
                    with pytest.raises(D.CimbarHipError, match="EINVAL"):
                        d.tap(what, 1)
            lo += n
    finally:
        fresh.close()
        dec.close()


# ---- 6. arguments
@pytest.mark.parametrize("legacy", [4, 8])
def test_refused_in_legacy_modes(gpu, legacy):
    dec = D.HipDecoder(0, legacy)
    try:
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.set_stream_colour_vote(True)
        dec.set_stream_colour_vote(False)
        assert dec.get_stream_colour_vote() is False
    finally:
        dec.close()


def test_getter_toggle_and_reset(gpu):
    mode = CORNER_MODE
    caps = GC.pair_set(mode)[0][8:10]                 # group 4 of the pair set
    ref = _reference(mode, caps)
    dec = D.HipDecoder(0, mode)
    try:
        assert dec.get_stream_colour_vote() is False and dec.get_group_colour_vote() is False
        dec.set_stream_colour_vote(True)
        assert dec.get_stream_colour_vote() is True and dec.get_group_colour_vote() is False
        first = dec.decode_batch_combined_stream(caps[:1])
        assert first[0] == 0 and first[3].tolist() == [D.GROUP_OPEN]
        # a toggle in mid-stream: refused before anything is enqueued, the open group untouched
        dec.set_stream_colour_vote(False)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(caps[1:], flush=True)
        dec.set_stream_colour_vote(True)
        second = dec.decode_batch_combined_stream(caps[1:], flush=True)
        assert second[0] == 1 and second[6][0] == 2
        assert second[5][0] == ref["gmasks"][0] and (second[4][0] == ref["gchunks"][0]).all()
        assert (dec.tap(D.TAP_GROUP_COLOUR_MARGIN, 1) == ref["gm"]).all()
        # the stream is empty but still holds the value; a reset lets the next call choose again
        dec.set_stream_colour_vote(False)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.decode_batch_combined_stream(caps[:1])
        dec.combine_stream_reset()
        off = dec.decode_batch_combined_stream(caps, flush=True)
        assert off[0] == 1
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.tap(D.TAP_GROUP_COLOUR_MARGIN, 1)
    finally:
        dec.close()


# ---- 7. device outputs
def test_device_outputs_match_host_outputs(gpu):
    mode = CORNER_MODE
    geo = geometry.for_mode(mode)
    triple, twins = _triple_and_twins(mode)
    caps = np.concatenate([GC.pair_set(mode)[0], np.stack(triple + twins)])
    cut = (2, 3, 4, 8)
    host, dec = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        host.set_stream_colour_vote(True)
        dec.set_stream_colour_vote(True)
        want = _stream(host, caps, cut)["calls"]
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(caps).to(dev)
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


# ---- 8. capture path
@pytest.mark.parametrize("cut", [(2, 3), (1,) * 5], ids=["2x3", "1x5"])
def test_capture_path(gpu, cut):
    mode = CORNER_MODE
    fr, _ = GC.K.frames(mode, 2, 91)
    size = (1280, 720)
    quad = ((270, 20), (1010, 30), (260, 690), (1020, 680))
    cams = []
    for k in range(2):
        for c, cx in enumerate((0.35, 0.65)):
            f = GC.damage(fr[k].copy(), GC.disc(fr[k].shape, cx, 0.5, 0.08), "washed", k)
            cams.append(F.camera_frame(f, width=size[0], height=size[1], quad=quad, background=96))
    cams.insert(2, np.full_like(cams[0], 96))                    # A1 A2 blank B1 B2
    raw = np.stack([CF.rgb_to_format(c, 3) for c in cams])
    ref, dec = D.HipDecoder(0, mode), D.HipDecoder(0, mode)
    try:
        ref.set_group_colour_vote(True)
        ng, chunks, masks, status, groups, gchunks, gmasks = ref.scan_extract_decode_batch_combined(raw, size=size, fmt=3, preprocess=0)
        assert groups.tolist() == [0, 0, -1, 1, 1] and ng == 2
        want_col, want_gm = ref.tap(D.TAP_GROUP_CELLS, ng) >> 4, ref.tap(D.TAP_GROUP_COLOUR_MARGIN, ng)
        assert (want_gm != 0xFFFFFFFF).sum() > 20
        dec.set_stream_colour_vote(True)
        got_masks, got_chunks, got_sizes, got_col, got_gm, per_capture = [], [], [], [], [], []
        lo = 0
        for c, n in enumerate(cut):
            r = dec.scan_extract_decode_batch_combined_stream(raw[lo:lo + n], flush=c == len(cut) - 1, size=size, fmt=3, preprocess=0)
            k = r[0]
            got_masks += r[6][:k].tolist(); got_chunks += list(r[5][:k]); got_sizes += r[7][:k].tolist()
            if k:
                got_col += list(dec.tap(D.TAP_GROUP_CELLS, k) >> 4)
                got_gm += list(dec.tap(D.TAP_GROUP_COLOUR_MARGIN, k))
            per_capture.append((r[1], r[2], r[3]))
            lo += n
        assert got_sizes == [2, 2] and got_masks == gmasks[:2].tolist()
        assert (np.stack(got_chunks) == gchunks[:2]).all()
        assert (np.stack(got_col) == want_col).all() and (np.stack(got_gm) == want_gm).all()
        assert (np.concatenate([p[0] for p in per_capture]) == chunks).all() and (np.concatenate([p[1] for p in per_capture]) == masks).all()
        assert (np.concatenate([p[2] for p in per_capture]) == status).all()
    finally:
        ref.close()
        dec.close()
