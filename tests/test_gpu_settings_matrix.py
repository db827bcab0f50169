"""GPU: every opt-in decode setting (symbol erasure, colour erasure, the relaxed flood with and without its fallback, and all of them
together) through every entry point and every chain shape of enqueue() (host.hip.inc). Inputs: tests/setting_cases.py.

The reference of every cell is the BASELINE of its setting: a fresh context, the setting, reset_ccm(), one small unsplit decode_batch of the
pool -- the entry point the settings' own suites hold to the oracle and to their numpy models. The matrix is tied down twice more: the rounds
flood of the baseline equals tests/relaxed_flood_model.py on the device's bit plane, and in every cell every chunk in a mask equals the
payload the frame was rendered from and every slot outside it is zero.

1. test_baseline*: the payload rule, the model anchor, and that the pool makes every setting bite (the matrix is not vacuous).
2. mode 68, setting x entry point on one context per setting, every entry point in turn: device batch, pipelined (default depth and depth 2),
   frame, frame-async, combined (+stream), stitched (+stream), once (+stream; the pool as it is and every frame shown three times), the capture
   path (preprocess 0 and the guess), the undistort composite.
3. mode 66, the relaxed flood in every chain shape: split in two and in four, a caller's stream, the dense replay, a rounds grid of two, no
   certifying pass, the spill-test build -- against the baseline per pool frame and against a context that never splits.

The certifying pass (k_flood_wave) declines a frame as soon as one of its rules fires, and on frames with large flat areas (the white discs of
radius 0.10) whether one fires depends on the order its lanes queue cells in: such a frame is path 2 in one run and 1 / 3 in the next. The
default chain delivers the same bytes either way; with the relaxed flood on, the frame is then flooded exactly in one run and in rounds in the
other. The pool holds frames on which this did not happen in repeated runs (a white disc of radius 0.13, noise discs).
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import build as hipbuild
from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import distorted_captures as DC
from tests import frames as F
from tests import relaxed_flood_model as M
from tests import repeat_skip_model as RM
from tests import setting_cases as SC
from tests.test_gpu_flood_verify import decoder_with

pytestmark = pytest.mark.gpu

POISON = 0xA5
KEPT_TAPS = (D.TAP_SYMBOLS, D.TAP_DRIFT, D.TAP_FLOOD_PATH, D.TAP_FLOOD_ROUNDS, D.TAP_RS_OK)
ANCHOR_FRAMES = (SC.POOL_NAMES.index("rescale6"), SC.POOL_NAMES.index("tear"))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ the baseline
def make_baseline(mode, name, env=None, lib_path=None):
    frames, _ = SC.pool(mode)
    n = len(frames)
    dec = decoder_with(env or {}, mode, lib_path) if env or lib_path else D.HipDecoder(0, mode)
    try:
        SC.BY_NAME[name](dec)
        dec.reset_ccm()
        total, chunks, masks = dec.decode_batch(frames)
        b = {"total": total, "chunks": chunks.copy(), "masks": masks.copy(), "stats": dec.relaxed_flood_stats(),
             "taps": {t: dec.tap(t, n) for t in KEPT_TAPS}}
        if name == "rf_accept":
            b["plane"] = dec.tap(D.TAP_BITPLANE, n)[list(ANCHOR_FRAMES)]
    finally:
        dec.close()
    b["path"] = b["taps"][D.TAP_FLOOD_PATH]
    for v in [b["chunks"], b["masks"], b["path"]] + list(b["taps"].values()):
        v.setflags(write=False)
    return b


class Baselines(dict):
    """setting -> its baseline, made once, when a test first asks for it, and left unchanged"""

    def __init__(self, mode, **kw):
        super().__init__()
        self.mode, self.kw = mode, kw

    def __missing__(self, name):
        self[name] = make_baseline(self.mode, name, **self.kw)
        return self[name]


@pytest.fixture(scope="module")
def base68():
    return Baselines(68)


@pytest.fixture(scope="module")
def base66():
    return Baselines(66)


def frame_stats(geo, b, fallback):
    """what each pool frame adds to relaxed_flood_stats(): (n, 4) -- flooded in rounds, accepted, handed to the exact replay, rounds"""
    info, path = b["taps"][D.TAP_FLOOD_ROUNDS], b["path"]
    rounds = info != 0
    if fallback:
        accepted = rounds & (path == 3)
    else:
        accepted = rounds & b["taps"][D.TAP_RS_OK][:, :geo.SYM_BLOCKS].all(1)
    return np.stack([rounds, accepted, rounds & (path == 1), info & 0xFFFF], 1).astype(np.int64)


def is_fallback(name):
    return name in ("rf_fallback", "all")


def check_cell(geo, b, chunks, masks, payload, tag, idx=None):
    """a cell of the matrix: per-capture chunks and masks equal the baseline's (of pool frames idx), and the payload rule"""
    idx = np.arange(len(b["masks"])) if idx is None else np.asarray(idx)
    masks = np.asarray(masks).astype(np.uint32)
    chunks = np.asarray(chunks).reshape(len(masks), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    SC.assert_payload_rule(geo, chunks, masks, payload[idx], tag)
    want = b["masks"][idx]
    assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want], f"{tag}: masks"
    assert (chunks == b["chunks"][idx]).all(), f"{tag}: chunks differ in frames {np.flatnonzero((chunks != b['chunks'][idx]).any((1, 2))).tolist()}"


@pytest.mark.parametrize("mode", [68, 66])
def test_baseline_obeys_the_payload_and_every_setting_bites(mode, base68, base66):
    base = base68 if mode == 68 else base66
    geo = geometry.for_mode(mode)
    _, payload = SC.pool(mode)
    symc = SC.K.sym_chunks(geo)
    sym_bits, col_bits = (1 << symc) - 1, ((1 << geo.CHUNKS_PER_FRAME) - 1) & ~((1 << symc) - 1)
    for name in SC.NAMES:
        b = base[name]
        print(f"mode {mode} {name}: path {b['path'].tolist()} masks {[hex(int(m)) for m in b['masks']]} stats {b['stats']}")
        SC.assert_payload_rule(geo, b["chunks"], b["masks"], payload, f"mode {mode} {name}")
        assert b["total"] == geo.CHUNK * int(SC.chunk_bits(geo, b["masks"]).sum())
        if name in SC.RELAXED:
            assert tuple(frame_stats(geo, b, is_fallback(name)).sum(0)) == b["stats"], name
        else:
            assert b["stats"] == (0, 0, 0, 0) and not b["taps"][D.TAP_FLOOD_ROUNDS].any()
    m = {name: base[name]["masks"].astype(np.int64) for name in SC.NAMES}
    p = {name: base[name]["path"] for name in SC.NAMES}

    def gains(a, over, bits):
        return ((a & bits) & ~(over & bits) != 0) & ((over & bits) & ~(a & bits) == 0)

    assert gains(m["sym"], m["off"], sym_bits).any(), "sym: no frame gains symbol chunks"
    assert (m["sym"] & m["off"] == m["off"]).all()
    assert gains(m["col"], m["off"], col_bits).any(), "col: no frame gains colour chunks"
    assert (m["col"] & m["off"] == m["off"]).all()
    assert (p["rf_accept"] == 3).sum() >= 4, p["rf_accept"]
    flooded = p["off"] == 1
    fb = p["rf_fallback"]
    assert (fb[flooded] == 1).any() and (fb[flooded] == 3).any(), fb
    assert set(fb[flooded].tolist()) <= {1, 3} and (fb[~flooded] == p["off"][~flooded]).all(), (fb, p["off"])
    assert np.flatnonzero(flooded & (fb == 1))[0] < np.flatnonzero(flooded & (fb == 3))[-1], "a path-1 frame precedes a path-3 one"
    # include/cimbar_hip.h: with the fallback on, a frame that falls back is the default policy's byte for byte
    back = flooded & (fb == 1)
    for key in ("chunks", "masks"):
        assert (base["rf_fallback"][key][back] == base["off"][key][back]).all(), f"a frame that fell back differs from the default policy's {key}"
    for t in (D.TAP_SYMBOLS, D.TAP_DRIFT, D.TAP_RS_OK):
        assert (base["rf_fallback"]["taps"][t][back] == base["off"]["taps"][t][back]).all(), f"a frame that fell back differs from the default policy's tap {t}"
    every = (1 << geo.CHUNKS_PER_FRAME) - 1
    assert (((p["all"] == 3) | (p["all"] == 1)) & gains(m["all"], m["rf_fallback"], every)).any(), (p["all"], m["all"], m["rf_fallback"])
    # what sequence() is built on
    assert fb[SC.FALLS_BACK[mode]] == 1 and p["all"][SC.FALLS_BACK[mode]] == 1
    assert fb[SC.ACCEPTED[mode]] == 3 and p["all"][SC.ACCEPTED[mode]] == 3
    assert (p["off"][list(SC.CLEAN)] == 0).all()
    # the flood of a frame depends on the frame alone: where two settings took a frame down the same path, symbols and drift are equal
    for name in SC.NAMES[1:]:
        same = p[name] == p["off"]
        assert (base[name]["taps"][D.TAP_SYMBOLS][same] == base["off"]["taps"][D.TAP_SYMBOLS][same]).all(), name
        moved = same & (p["off"] != 0)
        assert (base[name]["taps"][D.TAP_DRIFT][moved] == base["off"]["taps"][D.TAP_DRIFT][moved]).all(), name


def test_baseline_rounds_equal_the_model(base68):
    """the anchor: two rf_accept pool frames with path 3 against tests/relaxed_flood_model.py on the device's own bit plane"""
    b = base68["rf_accept"]
    ncells = geometry.for_mode(68).NCELLS
    for row, k in enumerate(ANCHOR_FRAMES):
        assert b["path"][k] == 3, (k, b["path"])
        sym, drift, rounds, dist = M.relaxed_flood(b["plane"][row], 68, SC.RF_ACCEPT)
        info = int(b["taps"][D.TAP_FLOOD_ROUNDS][k])
        print(f"pool frame {k} ({SC.POOL_NAMES[k]}): {rounds} rounds (device {info & 0xFFFF})")
        assert (dist >= 0).all()
        assert (b["taps"][D.TAP_SYMBOLS][k] == sym).all(), f"frame {k}: {(b['taps'][D.TAP_SYMBOLS][k] != sym).sum()} symbols differ from the model"
        assert (b["taps"][D.TAP_DRIFT][k] == drift).all(), f"frame {k}: drift differs from the model"
        assert info & 0xFFFF == rounds and info >> 16 == ncells, (k, hex(info), rounds)


# ------------------------------------------------------------------ 2. setting x entry point, mode 68
@pytest.fixture(scope="module")
def ctx68():
    """one context per setting for the whole column, and a second one created the same way for the calls a model drives"""
    made = {}
    for name in SC.NAMES:
        made[name] = (D.HipDecoder(0, 68), D.HipDecoder(0, 68))
        for d in made[name]:
            SC.BY_NAME[name](d)
    yield made
    for a, b in made.values():
        a.close()
        b.close()


def fresh(dec):
    dec.reset_ccm()
    dec.combine_stream_reset()
    dec.stitch_stream_reset()
    dec.once_stream_reset()
    return np.array(dec.relaxed_flood_stats(), np.int64)


def check_stats(dec, before, name, want, tag):
    if name in SC.RELAXED:
        got = np.array(dec.relaxed_flood_stats(), np.int64) - before
        assert tuple(got) == tuple(int(x) for x in want), f"{tag}: relaxed_flood_stats moved by {tuple(got)}, the baseline's are {tuple(want)}"


def check_path(dec, b, tag, idx=None):
    idx = np.arange(len(b["path"])) if idx is None else np.asarray(idx)
    got = dec.tap(D.TAP_FLOOD_PATH, len(idx))
    assert got.tolist() == b["path"][idx].tolist(), f"{tag}: path"


def device_outputs(geo, n, dev):
    return (torch.full((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), POISON, dtype=torch.uint8, device=dev),
            torch.full((n,), -0x5A5A5A5B, dtype=torch.int32, device=dev))


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_batch_device(name, base68, ctx68):
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    n = len(frames)
    dev = torch.device("cuda", 0)
    before = fresh(dec)
    d_in = torch.from_numpy(frames.copy()).to(dev)
    chunks, masks = device_outputs(dec.geo, n, dev)
    dec.decode_batch_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), False, 2, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    check_cell(dec.geo, b, host(chunks), host(masks), payload, f"{name} decode_batch_device")
    check_path(dec, b, name)
    for t in (D.TAP_SYMBOLS, D.TAP_FLOOD_ROUNDS):
        assert (dec.tap(t, n) == b["taps"][t]).all(), (name, t)
    check_stats(dec, before, name, b["stats"], name)


def pipelined(dec, frames, per):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    assert dec.pipeline_depth >= 2
    ins, outs = [], []
    for k in range(0, len(frames), per):
        ins.append(torch.from_numpy(frames[k:k + per].copy()).to(dev))
        outs.append(device_outputs(dec.geo, per, dev))
        if len(ins) > dec.pipeline_depth:          # all in flight that the context takes
            dec.pipeline_wait(st, keep_newest=dec.pipeline_depth - 1)
        dec.decode_batch_pipelined(ins[-1].data_ptr(), per, outs[-1][0].data_ptr(), outs[-1][1].data_ptr(), False, 2, st)
    dec.pipeline_wait(st)
    torch.cuda.synchronize(dev)
    return np.concatenate([host(o[0]) for o in outs]), np.concatenate([host(o[1]) for o in outs])


@pytest.mark.parametrize("depth", ["default", 2])
@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_batch_pipelined(name, depth, base68, ctx68):
    b = base68[name]
    frames, payload = SC.pool(68)
    if depth == "default":
        dec = ctx68[name][0]
    else:
        dec = decoder_with({"CIMBAR_HIP_PIPE_DEPTH": str(depth)})
        SC.BY_NAME[name](dec)
        assert dec.pipeline_depth == depth
    try:
        before = fresh(dec)
        chunks, masks = pipelined(dec, frames, 3)
        check_cell(dec.geo, b, chunks, masks, payload, f"{name} pipelined depth {depth}")
        check_stats(dec, before, name, b["stats"], name)
    finally:
        if depth != "default":
            dec.close()


@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_frame(name, base68, ctx68):
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    before = fresh(dec)
    got = [dec.decode_frame(f) for f in frames]
    check_cell(dec.geo, b, np.stack([g[1] for g in got]), [g[2] for g in got], payload, f"{name} decode_frame")
    assert [g[0] for g in got] == [dec.geo.CHUNK * bin(int(m)).count("1") for m in b["masks"]]
    check_stats(dec, before, name, b["stats"], name)


@pytest.mark.parametrize("name", SC.NAMES)
def test_decode_frame_async(name, base68, ctx68):
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    before = fresh(dec)
    tickets, got = [], []
    for f in frames:
        if len(tickets) == dec.pipeline_depth:
            got.append(dec.decode_frame_wait(tickets.pop(0)))
        tickets.append(dec.decode_frame_async(f))
    while tickets:
        got.append(dec.decode_frame_wait(tickets.pop(0)))
    check_cell(dec.geo, b, np.stack([g[1] for g in got]), [g[2] for g in got], payload, f"{name} decode_frame_async")
    check_stats(dec, before, name, b["stats"], name)


@pytest.mark.parametrize("name", SC.NAMES)
def test_combined_calls(name, base68, ctx68):
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    n = len(frames)
    before = fresh(dec)
    ng, chunks, masks, groups, gchunks, gmasks = dec.decode_batch_combined(frames, groups=None)
    check_cell(dec.geo, b, chunks, masks, payload, f"{name} combined")
    check_path(dec, b, f"{name} combined")
    check_stats(dec, before, name, b["stats"], f"{name} combined")
    # one capture per stream call, flush on the last: per capture the baseline's, the closed groups concatenated the combined call's
    before = fresh(dec)
    s_chunks, s_masks, s_gchunks, s_gmasks = [], [], [], []
    for k in range(n):
        r = dec.decode_batch_combined_stream(frames[k:k + 1], flush=k == n - 1)
        s_chunks.append(r[1][0]); s_masks.append(r[2][0])
        s_gchunks += list(r[4][:r[0]]); s_gmasks += list(r[5][:r[0]])
    check_cell(dec.geo, b, np.stack(s_chunks), s_masks, payload, f"{name} combined stream")
    check_stats(dec, before, name, b["stats"], f"{name} combined stream")
    assert len(s_gmasks) == ng and [int(x) for x in s_gmasks] == [int(x) for x in gmasks[:ng]]
    assert (np.stack(s_gchunks) == gchunks[:ng]).all()
    # (every pool frame is a frame of its own: the groups are the captures)
    SC.assert_payload_rule(dec.geo, gchunks[:ng], gmasks[:ng], payload[[int(np.flatnonzero(groups == g)[0]) for g in range(ng)]], f"{name} groups")


@pytest.mark.parametrize("name", SC.NAMES)
def test_stitched_calls(name, base68, ctx68):
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    n = len(frames)
    before = fresh(dec)
    r = dec.decode_batch_stitched(frames)
    check_cell(dec.geo, b, r[1], r[2], payload, f"{name} stitched")
    check_path(dec, b, f"{name} stitched")
    check_stats(dec, before, name, b["stats"], f"{name} stitched")
    before = fresh(dec)
    got = [dec.decode_batch_stitched_stream(frames[k:k + 1]) for k in range(n)]
    check_cell(dec.geo, b, np.stack([g[1][0] for g in got]), [g[2][0] for g in got], payload, f"{name} stitched stream")
    check_stats(dec, before, name, b["stats"], f"{name} stitched stream")


@pytest.mark.parametrize("name", SC.NAMES)
def test_once_calls_on_the_pool(name, base68, ctx68):
    """every pool frame is another displayed frame: every capture is its own run, pass 1 decodes the input in place"""
    dec, b = ctx68[name][0], base68[name]
    frames, payload = SC.pool(68)
    n = len(frames)
    before = fresh(dec)
    n_runs, chunks, masks, runs, roles, rchunks, rmasks = dec.decode_batch_once(frames)
    assert n_runs == n and runs.tolist() == list(range(n)) and roles.tolist() == [D.ONCE_REPRESENTATIVE] * n
    check_cell(dec.geo, b, chunks, masks, payload, f"{name} once")
    check_cell(dec.geo, b, rchunks, rmasks, payload, f"{name} once, runs")
    check_path(dec, b, f"{name} once")
    check_stats(dec, before, name, b["stats"], f"{name} once")
    before = fresh(dec)
    n_runs, continued, chunks, masks, runs, roles, rchunks, rmasks = dec.decode_batch_once_stream(frames)
    assert n_runs == n and continued == 0 and runs.tolist() == list(range(n))
    check_cell(dec.geo, b, chunks, masks, payload, f"{name} once stream")
    check_cell(dec.geo, b, rchunks, rmasks, payload, f"{name} once stream, runs")
    check_stats(dec, before, name, b["stats"], f"{name} once stream")


@pytest.fixture(scope="module")
def shown_thrice():
    frames, payload = SC.pool(68)
    fr, pay = SC.thrice(frames, payload)
    _, _, runs, members, list1 = RM.plan(68, fr)
    assert runs.tolist() == [k // 3 for k in range(len(fr))], "the light noise was meant to leave every triple one run"
    return fr, pay, runs, members, list1


@pytest.mark.parametrize("name", SC.NAMES)
def test_once_calls_on_frames_shown_three_times(name, ctx68, shown_thrice):
    """enqueue() on a gathered list, twice in the call where a representative is incomplete: against tests/repeat_skip_model.py driven by plain
    decode_batch calls on a context with the same setting"""
    dec, ref = ctx68[name]
    geo = dec.geo
    fr, pay, want_runs, members, list1 = shown_thrice
    n = len(fr)
    before_ref = fresh(ref)
    want_chunks, want_masks = np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8), np.zeros(n, np.uint32)
    _, c1, m1 = ref.decode_batch(fr[list1])
    want_chunks[list1], want_masks[list1] = c1, m1
    list2 = RM.fallback_list(68, members, m1)
    assert list2, "some representative was meant to be incomplete: the second pass runs"
    _, c2, m2 = ref.decode_batch(fr[list2])
    want_chunks[list2], want_masks[list2] = c2, m2
    want_stats = np.array(ref.relaxed_flood_stats(), np.int64) - before_ref
    want_roles = RM.roles(n, want_runs, list1, list2)
    want_rc, want_rm = RM.run_fill(68, n, members, want_chunks, want_masks)
    SC.assert_payload_rule(geo, want_chunks, want_masks, pay, f"{name} plain calls")
    for call in ("once", "once_stream"):
        before = fresh(dec)
        got = dec.decode_batch_once(fr) if call == "once" else dec.decode_batch_once_stream(fr)
        if call == "once_stream":
            assert got[1] == 0
            got = (got[0],) + got[2:]
        n_runs, chunks, masks, runs, roles, rchunks, rmasks = got
        tag = f"{name} {call} x3"
        assert n_runs == len(members) and runs.tolist() == want_runs.tolist() and roles.tolist() == want_roles.tolist(), tag
        SC.assert_payload_rule(geo, chunks, masks, pay, tag)
        assert [hex(int(m)) for m in masks] == [hex(int(m)) for m in want_masks], tag
        assert (chunks == want_chunks).all(), tag
        assert (rmasks == want_rm).all() and (rchunks == want_rc).all(), tag
        check_stats(dec, before, name, want_stats, tag)
        (a_on, a_m), (b_on, b_m) = dec.get_ccm(), ref.get_ccm()
        assert a_on == b_on and (a_m == b_m).all(), tag


QUADS = [((500, 40), (1480, 70), (470, 1030), (1500, 1000)), ((520, 60), (1450, 40), (540, 1010), (1430, 1040)),
         ((480, 30), (1460, 50), (500, 1040), (1480, 1010)), ((510, 50), (1470, 30), (490, 1020), (1490, 1045))]
CAPTURED = [SC.POOL_NAMES.index(k) for k in ("clean0", "white13", "shift+2+1", "clean1")]


@pytest.fixture(scope="module")
def captures():
    frames, payload = SC.pool(68)
    cams = np.ascontiguousarray(np.stack([F.camera_frame(frames[p], quad=QUADS[k], background=12) for k, p in enumerate(CAPTURED)]))
    return cams, payload[CAPTURED]


@pytest.mark.parametrize("preprocess", [0, -1])
@pytest.mark.parametrize("name", SC.NAMES)
def test_capture_path(name, preprocess, ctx68, captures):
    dec, ref = ctx68[name]
    cams, payload = captures
    n = len(cams)
    status, corners, frames = ref.extract_batch(cams)
    assert (status > 0).all(), status
    before_ref = fresh(ref)
    if preprocess == 0:
        total, chunks, masks = ref.decode_batch(frames, should_preprocess=False)
        path = ref.tap(D.TAP_FLOOD_PATH, n)
    else:
        # the guess: the extractor's verdict per capture (2: the capture wants sharpening)
        rows = [ref.decode_batch(frames[k:k + 1], should_preprocess=status[k] == 2) for k in range(n)]
        total, chunks, masks = sum(r[0] for r in rows), np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])
        path = None
    want_stats = np.array(ref.relaxed_flood_stats(), np.int64) - before_ref
    before = fresh(dec)
    t, c, m, st = dec.scan_extract_decode_batch(cams, preprocess=preprocess)
    tag = f"{name} capture path, preprocess {preprocess}"
    assert (st == status).all(), tag
    SC.assert_payload_rule(dec.geo, c, m, payload, tag)
    assert [hex(int(x)) for x in m] == [hex(int(x)) for x in masks] and (c == chunks).all() and t == total, tag
    if path is not None:
        assert dec.tap(D.TAP_FLOOD_PATH, n).tolist() == path.tolist(), tag
    check_stats(dec, before, name, want_stats, tag)


@pytest.fixture(scope="module")
def lens_captures():
    from libcimbar_amd import framegen
    caps = np.ascontiguousarray(np.stack([DC.case("barrel_1080"), DC.case("mild_barrel_1080")]))
    payload = framegen.synth_payload(1, seed=11, mode=68).numpy().reshape(1, -1)          # (distorted_captures.CASES: both draw the frame of seed 11)
    return caps, np.concatenate([payload, payload])


@pytest.mark.parametrize("name", SC.NAMES)
def test_undistort_composite(name, ctx68, lens_captures):
    dec, ref = ctx68[name]
    caps, payload = lens_captures
    imgs, ok, _ = ref.undistort_batch(caps)
    before_ref = fresh(ref)
    t2, c2, m2, s2 = ref.scan_extract_decode_batch(imgs)
    want_stats = np.array(ref.relaxed_flood_stats(), np.int64) - before_ref
    before = fresh(dec)
    total, chunks, masks, status, uok = dec.scan_undistort_extract_decode_batch(caps)
    tag = f"{name} undistort composite"
    assert (uok == ok).all() and (status == s2).all() and (status > 0).all(), tag
    SC.assert_payload_rule(dec.geo, chunks, masks, payload, tag)
    assert (masks == m2).all() and (chunks == c2).all() and total == t2, tag
    check_stats(dec, before, name, want_stats, tag)


# ------------------------------------------------------------------ 3. the relaxed flood in every chain shape, mode 66
@pytest.fixture(scope="module")
def d_pool66():
    return torch.from_numpy(SC.pool(66)[0].copy()).to(torch.device("cuda", 0))


def run_batches(dec, d_pool, batches, stream=None, taps=True):
    """each batch (pool indices) through decode_batch_device into poisoned outputs -> per batch (chunks, masks, taps)"""
    dev = d_pool.device
    out = []
    for idx in batches:
        n = len(idx)
        frames = d_pool[torch.tensor(idx, device=dev)].contiguous()
        chunks, masks = device_outputs(dec.geo, n, dev)
        torch.cuda.synchronize(dev)
        dec.decode_batch_device(frames.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), False, 2, stream.cuda_stream if stream is not None else None)
        torch.cuda.synchronize(dev)
        out.append((host(chunks), host(masks), {t: dec.tap(t, n) for t in KEPT_TAPS} if taps else None))
        del frames
    return out


_unsplit = {}


def unsplit(name, key, batches, d_pool, wave=True):
    """the same sequence on a context that never splits, in batches of 16: chunks, masks per batch and the carried matrix at the end
    (wave=False: without the certifying pass either, for the shape that has none)"""
    key = key + (wave,)
    if (name, key) not in _unsplit:
        dec = decoder_with({"CIMBAR_HIP_TAIL_SPLIT": "0", **({} if wave else {"CIMBAR_HIP_FLOOD_WAVE": "0"})}, 66)
        try:
            SC.BY_NAME[name](dec)
            dec.reset_ccm()
            res = []
            for idx in batches:
                rows = run_batches(dec, d_pool, [idx[k:k + 16] for k in range(0, len(idx), 16)], taps=False)
                res.append((np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])))
            _unsplit[(name, key)] = (res, dec.get_ccm())
        finally:
            dec.close()
    return _unsplit[(name, key)]


SHAPES = {
    # name: (environment, spill-test build, n, parts, caller's stream, settings)
    "split2": ({}, False, 128, 2, False, ("rf_accept", "rf_fallback", "all")),
    "split4": ({"CIMBAR_HIP_TAIL_PARTS": "4"}, False, 256, 4, False, ("rf_fallback", "all")),
    "split2_stream": ({}, False, 128, 2, True, ("rf_accept", "rf_fallback", "all")),
    "dense": ({"CIMBAR_HIP_FLOOD_DENSE": "1"}, False, 16, 0, False, ("rf_fallback", "all")),
    "rounds_grid2": ({"CIMBAR_HIP_ROUNDS_GRID": "2"}, False, 16, 0, False, ("rf_fallback", "all")),
    "no_wave": ({"CIMBAR_HIP_FLOOD_WAVE": "0"}, False, 16, 0, False, ("rf_fallback", "all")),
    "spilltest": ({}, True, 16, 0, False, ("rf_fallback", "all")),
}


@pytest.fixture(scope="module")
def base66_no_wave():
    """the baseline of the shape without the certifying pass: what that pass settles in the other shapes (path 2) is flooded here, so the frame's
    path is another. Made like every baseline; test_chain_shapes ties it to base66 on the frames the pass does not settle."""
    return Baselines(66, env={"CIMBAR_HIP_FLOOD_WAVE": "0"})


@pytest.mark.parametrize("shape,name", [(s, n) for s, v in SHAPES.items() for n in v[5]])
def test_chain_shapes(shape, name, base66, base66_no_wave, d_pool66):
    env, spill, n, parts, own_stream, _ = SHAPES[shape]
    geo = geometry.for_mode(66)
    _, payload = SC.pool(66)
    b = base66[name]
    if shape == "no_wave":
        nw = base66_no_wave[name]
        SC.assert_payload_rule(geo, nw["chunks"], nw["masks"], payload, "no_wave baseline")
        keep = b["path"] != 2
        assert (nw["path"][keep] == b["path"][keep]).all() and (nw["path"][~keep] != 2).all(), (nw["path"], b["path"])
        assert (nw["taps"][D.TAP_SYMBOLS][keep] == b["taps"][D.TAP_SYMBOLS][keep]).all()
        assert (nw["masks"][keep] == b["masks"][keep]).all() and (nw["chunks"][keep] == b["chunks"][keep]).all()
        b = nw
    if parts:
        first = SC.sequence(n, parts)
        batches = [first, first[::-1]]
        assert n >= 64 * parts and all(4 * sum(b["path"][k] != 0 for k in idx) <= n for idx in batches)      # both batches split (host.hip.inc)
    else:
        first = SC.short_sequence(n)
        batches = [first, first[5:] + first[:5]]
    want, want_ccm = unsplit(name, (n, parts), batches, d_pool66, wave=shape != "no_wave")
    per_frame = frame_stats(geo, b, is_fallback(name))
    dec = decoder_with(env, 66, hipbuild.OUT_SPILLTEST if spill else None)
    stream = torch.cuda.Stream(d_pool66.device) if own_stream else None
    try:
        SC.BY_NAME[name](dec)
        dec.reset_ccm()
        got = run_batches(dec, d_pool66, batches, stream)
        stats = dec.relaxed_flood_stats()
        ccm = dec.get_ccm()
    finally:
        dec.close()
    for k, idx in enumerate(batches):
        chunks, masks, taps = got[k]
        idx = np.asarray(idx)
        tag = f"{shape} {name} batch {k}"
        SC.assert_payload_rule(geo, chunks, masks, payload[idx], tag)
        path = taps[D.TAP_FLOOD_PATH]
        assert path.tolist() == b["path"][idx].tolist(), f"{tag}: path differs at {np.flatnonzero(path != b['path'][idx]).tolist()}"
        bad = np.flatnonzero((taps[D.TAP_SYMBOLS] != b["taps"][D.TAP_SYMBOLS][idx]).any(1))
        assert bad.size == 0, f"{tag}: symbols differ from the baseline's at positions {bad.tolist()} (pool frames {idx[bad].tolist()})"
        moved = path != 0
        assert (taps[D.TAP_DRIFT][moved] == b["taps"][D.TAP_DRIFT][idx][moved]).all(), f"{tag}: drift"
        assert (taps[D.TAP_FLOOD_ROUNDS] == b["taps"][D.TAP_FLOOD_ROUNDS][idx]).all(), f"{tag}: rounds"
        w_chunks, w_masks = want[k]
        bad = np.flatnonzero(masks != w_masks)
        assert bad.size == 0, f"{tag}: masks differ from the unsplit context's at positions {bad.tolist()}"
        bad = np.flatnonzero((chunks != w_chunks).any((1, 2)))
        assert bad.size == 0, f"{tag}: chunks differ from the unsplit context's at positions {bad.tolist()}"
    total = sum(per_frame[np.asarray(idx)].sum(0) for idx in batches)
    assert stats == tuple(int(x) for x in total), f"{shape} {name}: stats {stats}, the sums over the sequence {tuple(total)}"
    assert ccm[0] == want_ccm[0] and (ccm[1] == want_ccm[1]).all(), f"{shape} {name}: carried matrix"
