"""GPU: the symbol erasure retry (cimbar_hip_set_erasure_decode -> k_erasure_frame; group_end_body with e_on) against tests/symbol_erasure_model.py fed
by the oracle, chunk for chunk, modes 68 / 67 / 66, on the case set of tests/symbol_erasure_cases.py (which tests/test_symbol_erasure_model.py
shows to be sensitive to every rule of the retry).

- decode_batch: TAP_SYMBOLS, TAP_DRIFT and TAP_BITPLANE equal the oracle's (the precondition), masks and chunks equal the model's, TAP_RS_OK and
  the colour chunks equal the run without the retry. A frame with TAP_FLOOD == 0 has the oracle's positions on the grid: "grid position" and
  "final position" are one definition there.
- settings: t_sym in {1, 6, above every distance, 64} x max_erasures in {default, 1, parity, 0}.
- entry points: decode_frame, decode_frame_async with several frames in flight, decode_batch_pipelined, device-output decode_batch on a caller's
  stream, scan_extract_decode_batch on 1280x720 captures (expected: the model fed with the oracle's co_extract frame) and the undistort
  composite on an axis-aligned capture, whose calibration fails.
- both retries on: the symbol model's symbol chunks and the colour model's colour chunks.
- groups of two and three captures through decode_batch_combined and, one capture per call, decode_batch_combined_stream: gmask / gchunks
  equal retry_group fed with combine_model.combine_cells of the taps.
"""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from oracle import pyref
from tests import colour_erasure_model as CEM
from tests import combine_model as CM
from tests import frames as F
from tests import symbol_erasure_cases as K
from tests import symbol_erasure_model as M

pytestmark = pytest.mark.gpu
COLOUR_MARGIN = D.COLOUR_MARGIN_SUGGESTED


@pytest.fixture(scope="module", params=K.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


def _symc(geo):
    return geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)


def _explain(geo, f, got_mask, got_chunks, want):
    """None if equal, else a message naming the frame, the chunk and the first block of it whose record explains the model's side"""
    wm, wc, rec = want[0], want[1], want[2]
    got_chunks = np.asarray(got_chunks).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    bpc = geo.CHUNK // geo.RS_DATA
    for j in range(geo.CHUNKS_PER_FRAME):
        if ((int(got_mask) ^ wm) >> j) & 1 or (got_chunks[j] != wc[j]).any():
            msg = f"frame {f} chunk {j}: device mask bit {(int(got_mask) >> j) & 1}, model {(wm >> j) & 1}, {int((got_chunks[j] != wc[j]).sum())} bytes differ"
            if rec and j < _symc(geo):
                for q in range(bpc):
                    rb = rec[j * bpc + q]
                    if rb["status"] != 1 or q == bpc - 1:
                        return msg + f"; block {j * bpc + q}: model status {rb['status']}, errors-only ok {rb['ok']}, erasures {rb['erasures']}"
            return msg
    return None


def _assert_frames(geo, masks, chunks, want, what=""):
    for f in range(len(want)):
        bad = _explain(geo, f, masks[f], chunks[f], want[f])
        assert bad is None, what + bad


def _want(mode, t_sym=K.T_SYM, max_erasures=None):
    return K.model_frames(mode, K.oracle_frames(mode), t_sym, max_erasures)


def test_decode_batch_equals_model(MODE):
    geo = geometry.for_mode(MODE)
    frames, runs = K.case_set(MODE)["frames"], K.oracle_frames(MODE)
    n = len(frames)
    grid = geo.cell_positions().astype(np.int64)
    off, on = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        _, c0, m0 = off.decode_batch(frames)
        ok0 = off.tap(D.TAP_RS_OK, n)
        on.set_erasure_decode(K.T_SYM)
        _, c1, m1 = on.decode_batch(frames)
        sym, drift, plane = on.tap(D.TAP_SYMBOLS, n), on.tap(D.TAP_DRIFT, n), on.tap(D.TAP_BITPLANE, n)
        ok1, flood = on.tap(D.TAP_RS_OK, n), on.tap(D.TAP_FLOOD, n)
    finally:
        off.close()
        on.close()
    # the precondition: what the retry reads is the oracle's
    for f, r in enumerate(runs):
        assert (plane[f] == r["plane"]).all(), f"frame {f}: bit plane"
        assert ((sym[f] & 15) == (r["symbols"] & 15)).all(), f"frame {f}: symbols"
        if flood[f]:
            assert (drift[f].astype(np.int64) == r["positions"] - grid).all(), f"frame {f}: drift"
        else:
            assert (r["positions"] == grid).all(), f"frame {f}: the oracle drifts on a frame that did not take the flood pass"
        assert int(m0[f]) == r["mask"] and (c0[f] == r["chunks"]).all(), f"frame {f}: the result without the retry"
    assert flood[3] and not flood[0]
    want = _want(MODE)
    _assert_frames(geo, m1, c1, want)
    assert (ok1 == ok0).all(), "the retry changed a per-block flag"
    symc = _symc(geo)
    assert (c1[:, symc:] == c0[:, symc:]).all() and ((m1 ^ m0) >> symc == 0).all(), "the retry changed a colour chunk"
    for f, w in enumerate(want):
        for b, rb in enumerate(w[2] or []):
            if rb["status"] != 2:
                assert bool(ok1[f, b]) == rb["ok"], (f, b)
    assert (m1 != m0).any()


def test_settings_matrix(MODE):
    geo = geometry.for_mode(MODE)
    frames, runs = K.case_set(MODE)["frames"], K.oracle_frames(MODE)
    top = max(int(w[3].max()) for w in _want(MODE)) + 1
    assert top <= 64
    dec = D.HipDecoder(0, MODE)
    try:
        caps = [-1, 1, geo.RS_PARITY, 0]               # (0 is within the header's "at most the parity bytes": accepted, and nothing is ever erased)
        with pytest.raises(D.CimbarHipError):
            dec.set_erasure_decode(K.T_SYM, -1, geo.RS_PARITY + 1)
        for t_sym in (1, K.T_SYM, top, 64):
            for cap in caps:
                dec.set_erasure_decode(t_sym, -1, cap)
                assert dec.get_erasure_decode() == (True, t_sym, -1, geo.RS_PARITY - 8 if cap < 0 else cap)
                dec.reset_ccm()
                _, c, m = dec.decode_batch(frames)
                want = _want(MODE, t_sym, cap)
                _assert_frames(geo, m, c, want, f"t_sym {t_sym} max_erasures {cap}: ")
                if t_sym >= top or cap == 0:
                    # nothing is erased: the result is the one without the retry, but for a chunk whose blocks errors-only decoding all
                    # accepted (aligned_stream drops the chunk after a bad last block; the retry decodes its blocks again with no erasure)
                    bpc = geo.CHUNK // geo.RS_DATA
                    for f, r in enumerate(runs):
                        rec = want[f][2] or []
                        assert not any(rb["erasures"] for rb in rec), (t_sym, cap, f)
                        again = sum(1 << j for j in range(_symc(geo)) if rec and all(rec[j * bpc + q]["ok"] for q in range(bpc)))
                        assert int(m[f]) == r["mask"] | again, (t_sym, cap, f)
                        keep = [j for j in range(geo.CHUNKS_PER_FRAME) if not (again >> j) & 1]
                        assert (c[f][keep] == r["chunks"][keep]).all(), (t_sym, cap, f)
    finally:
        dec.close()


def test_entry_points(MODE):
    geo = geometry.for_mode(MODE)
    frames = K.case_set(MODE)["frames"]
    n = len(frames)
    want = _want(MODE)
    dev = torch.device("cuda", 0)
    fb = geo.CHUNKS_PER_FRAME * geo.CHUNK

    def fresh():
        d = D.HipDecoder(0, MODE)
        d.set_erasure_decode(K.T_SYM)
        return d

    dec = fresh()
    try:
        got = [dec.decode_frame(frames[f]) for f in range(n)]
        _assert_frames(geo, [g[2] for g in got], [g[1] for g in got], want, "decode_frame: ")
    finally:
        dec.close()
    dec = fresh()
    try:
        tickets, got = [], []
        for f in range(n):
            tickets.append(dec.decode_frame_async(frames[f]))
            if len(tickets) == 3:
                got.append(dec.decode_frame_wait(tickets.pop(0)))
        while tickets:
            got.append(dec.decode_frame_wait(tickets.pop(0)))
        _assert_frames(geo, [g[2] for g in got], [g[1] for g in got], want, "decode_frame_async: ")
    finally:
        dec.close()
    dec = fresh()
    try:
        st = torch.cuda.current_stream(dev).cuda_stream
        tens = [torch.from_numpy(np.ascontiguousarray(frames[k:k + 2])).to(dev) for k in range(0, n, 2)]
        outs = [(torch.zeros((len(t), fb), dtype=torch.uint8, device=dev), torch.zeros((len(t),), dtype=torch.int32, device=dev)) for t in tens]
        for t, (c, m) in zip(tens, outs):
            dec.decode_batch_pipelined(t.data_ptr(), len(t), c.data_ptr(), m.data_ptr(), False, 2, st)
        dec.pipeline_wait(st)
        torch.cuda.synchronize()
        c = np.concatenate([o[0].cpu().numpy() for o in outs])
        m = np.concatenate([o[1].cpu().numpy() for o in outs]).astype(np.uint32)
        _assert_frames(geo, m, c, want, "decode_batch_pipelined: ")
    finally:
        dec.close()
    dec = fresh()
    try:
        mine = torch.cuda.Stream(device=dev)
        t = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        c = torch.zeros((n, fb), dtype=torch.uint8, device=dev)
        m = torch.zeros((n,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        dec.decode_batch_device(t.data_ptr(), n, c.data_ptr(), m.data_ptr(), stream=mine.cuda_stream)
        mine.synchronize()
        _assert_frames(geo, m.cpu().numpy().astype(np.uint32), c.cpu().numpy(), want, "decode_batch on a caller's stream: ")
    finally:
        dec.close()


QUADS = {68: ((285, 4), (995, 8), (280, 715), (1000, 710)), 67: ((160, 20), (1120, 30), (150, 700), (1130, 690)),
         66: ((250, 15), (1030, 25), (245, 700), (1040, 690))}
STRAIGHT = {68: ((290, 10), (990, 10), (290, 710), (990, 710)), 67: ((150, 20), (1130, 20), (150, 709), (1130, 709)),
            66: ((240, 20), (1040, 20), (240, 712), (1040, 712))}
BACKGROUND = {68: 0, 67: 96, 66: 96}          # (a 1024 x 1024 frame at 710 capture rows: the anchors are found against black only)


def _capture_model(mode, cams):
    """the oracle's co_extract frame of each capture through the oracle and the model -> (status, [(mask, chunks, record, d, the mask without the retry)])"""
    geo = geometry.for_mode(mode)
    O = pyref.oracle_lib(mode)
    n, h, w = cams.shape[:3]
    status, want, ccm = [], [], None
    for k in range(n):
        fr = np.zeros(geo.FRAME_SHAPE, np.uint8)
        c8 = (ctypes.c_float * 8)()
        st = O.co_extract(pyref.P(np.ascontiguousarray(cams[k])), w, h, pyref.P(fr), c8)
        status.append(st)
        assert st > 0, k
        pre = 1 if st == 2 else 0
        _, chunks, mask, ccm = pyref.oracle_decode(fr, pre, 2, ccm, mode=mode)
        sym, col, pos = pyref.oracle_stage(mode=mode)
        plane = np.zeros(geo.IMG_W * geo.IMG_H // 8, np.uint8)
        O.co_threshold_bitplane(pyref.P(fr), geo.IMG_W, geo.IMG_H, pre, pyref.P(plane))
        d = M.cell_distances(mode, plane, sym, pos, True, absolute=True)
        want.append(M.retry_frame(geo, sym, d, mask, chunks, K.T_SYM) + (d, int(mask)))
    return status, want


def test_capture_path_and_undistort_composite(MODE):
    geo = geometry.for_mode(MODE)
    frames = K.case_set(MODE)["frames"]
    # two designed frames (the resampling blurs their graded cells: the retry works on them and is turned down) and a glare disc of 0.12 of
    # the frame's size, white and noise, over the clean frame (the retry wins chunks back)
    shots = [frames[1], frames[4], K._disc(frames[0].copy(), 0.5, 0.5, 0.12, "white", 3), K._disc(frames[0].copy(), 0.5, 0.5, 0.12, "noise", 3)]
    cams = np.ascontiguousarray(np.stack([F.camera_frame(s, width=1280, height=720, quad=QUADS[MODE], background=BACKGROUND[MODE]) for s in shots]))
    status, want = _capture_model(MODE, cams)
    print(f"mode {MODE} capture path: masks without / with the retry {[(hex(w[4]), hex(w[0])) for w in want]}")
    assert any(w[0] != w[4] for w in want), "the retry must win a chunk back on at least one capture"
    assert any(rb["erasures"] and rb["status"] != 1 for w in want for rb in (w[2] or [])), "... and turn a block down on one"
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_erasure_decode(K.T_SYM)
        _, c, m, st = dec.scan_extract_decode_batch(cams)
        assert list(st) == status
        _assert_frames(geo, m, c, want, "scan_extract_decode_batch: ")
    finally:
        dec.close()
    straight = np.ascontiguousarray(np.stack([F.camera_frame(frames[1], width=1280, height=720, quad=STRAIGHT[MODE], background=BACKGROUND[MODE])]))
    status, want = _capture_model(MODE, straight)
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_erasure_decode(K.T_SYM)
        _, c, m, st, ok = dec.scan_undistort_extract_decode_batch(straight)
        assert list(ok) == [0], "the calibration of an axis-aligned capture must fail"
        assert list(st) == status
        _assert_frames(geo, m, c, want, "scan_undistort_extract_decode_batch: ")
    finally:
        dec.close()


def test_both_retries_on(MODE):
    geo = geometry.for_mode(MODE)
    frames, runs = K.case_set(MODE)["frames"], K.oracle_frames(MODE)
    n, symc = len(frames), _symc(geo)
    want = _want(MODE)
    dec = D.HipDecoder(0, MODE)
    try:
        dec.set_erasure_decode(K.T_SYM)
        dec.set_colour_erasure_decode(COLOUR_MARGIN)
        _, c, m = dec.decode_batch(frames)
        tap = dec.tap(D.TAP_COLOUR_MARGIN, n)
    finally:
        dec.close()
    for f, r in enumerate(runs):
        mg = CEM.margins(CEM.cell_means(frames[f], r["positions"]), r["ccm"])
        cm, cc, worked = CEM.retry_frame(geo, r["colours"], mg, r["mask"], r["chunks"], COLOUR_MARGIN)
        assert (tap[f] == (mg if worked else CEM.SKIPPED)).all(), f"frame {f}: colour margin tap"
        both_mask = want[f][0] | cm
        both = np.concatenate([want[f][1][:symc], cc[symc:]])
        bad = _explain(geo, f, m[f], c[f], (both_mask, both, want[f][2]))
        assert bad is None, bad


def _group_want(mode, dec_on, n, groups, gm0, gc0, m1, c1):
    """retry_group for every group, from the taps of the retry-on context's last call"""
    geo = geometry.for_mode(mode)
    planes, sym, col = dec_on.tap(D.TAP_BITPLANE, n), dec_on.tap(D.TAP_SYMBOLS, n), dec_on.tap(D.TAP_COLORS, n)
    drift, path = dec_on.tap(D.TAP_DRIFT, n), dec_on.tap(D.TAP_FLOOD_PATH, n)
    out = []
    for g in range(CM.n_groups(groups)):
        mem = CM.members(groups, g)
        cells, margins = CM.combine_cells(mode, planes, sym, col, drift, path, mem, tiles=D.tile_hashes())
        s, c = np.stack([sym[k] & 15 for k in mem]), np.stack([col[k] for k in mem])
        disputed = bool((s != s[0]).any() or (c != c[0]).any())
        out.append(M.retry_group(geo, cells, margins, gm0[g], gc0[g], [m1[k] for k in mem], [c1[k] for k in mem], disputed=disputed))
    return out


def test_groups(MODE):
    geo = geometry.for_mode(MODE)
    cs, runs = K.case_set(MODE), K.oracle_group_caps(MODE)
    caps, groups = cs["group_caps"], cs["groups"]
    n = len(caps)
    members_want = K.model_frames(MODE, runs)
    off, on, one = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        on.set_erasure_decode(K.T_SYM)
        one.set_erasure_decode(K.T_SYM)
        ng0, _, _, _, gc0, gm0 = off.decode_batch_combined(caps, groups=groups)
        ng1, c1, m1, _, gc1, gm1 = on.decode_batch_combined(caps, groups=groups)
        assert ng0 == ng1 == 3
        _assert_frames(geo, m1, c1, members_want, "members: ")
        want = _group_want(MODE, on, n, groups, gm0, gc0, m1, c1)
        for g, w in enumerate(want):
            rec = [rb if rb else dict(status=2, ok=None, erasures=[]) for rb in w[2]]
            bad = _explain(geo, g, gm1[g], gc1[g], (w[0], w[1], rec))
            assert bad is None, "group " + bad
        print(f"mode {MODE}: group masks without / with the retry", [(hex(int(gm0[g])), hex(int(gm1[g]))) for g in range(3)])
        assert (gm1[:3] != gm0[:3]).any()
        # one capture per call. The stream calls take no groups: the expected result is the model over the device's own grouping of the batch
        ng2, c2, m2, auto, gc2, gm2 = on.decode_batch_combined(caps)
        assert auto.tolist() == CM.group_captures(on.tap(D.TAP_SYMBOLS, n), on.tap(D.TAP_COLORS, n)).tolist()
        _, _, _, _, gc0a, gm0a = off.decode_batch_combined(caps)
        want2 = _group_want(MODE, on, n, auto, gm0a, gc0a, m2, c2)
        closed_c, closed_m = [], []
        for k in range(n):
            nc, _, _, _, gc, gm, _ = one.decode_batch_combined_stream(caps[k:k + 1], flush=(k == n - 1))
            closed_c += [gc[i] for i in range(nc)]
            closed_m += [int(gm[i]) for i in range(nc)]
        assert len(closed_m) == ng2 == len(want2)
        for g, w in enumerate(want2):
            rec = [rb if rb else dict(status=2, ok=None, erasures=[]) for rb in w[2]]
            for what, gm, gc in (("combined", gm2[g], gc2[g]), ("stream", closed_m[g], closed_c[g])):
                bad = _explain(geo, g, gm, gc, (w[0], w[1], rec))
                assert bad is None, f"{what}, the device's grouping {auto.tolist()}: group " + bad
    finally:
        off.close()
        on.close()
        one.close()
