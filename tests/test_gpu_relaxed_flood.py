"""GPU: the relaxed flood (cimbar_hip_set_relaxed_flood; k_flood_rounds, k_rounds_check and their place in the chain).
  * with the fallback off the device equals the numpy model of the rule (tests/relaxed_flood_model.py) cell for cell: symbols, drift, rounds;
  * with the fallback on, exactly the frames with a failing symbol block take the exact replay and equal a default context's byte for byte,
    the others have every symbol block decoded and deliver the default context's symbol chunks wherever that one delivered them;
  * a workgroup that walks several frames, the setting switched off again, invalid settings, the other entry points."""
import os

import numpy as np
import pytest

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from tests import frames as F
from tests import relaxed_flood_model as M

pytestmark = pytest.mark.gpu


def tear(c, cut):
    return np.concatenate([F.shift(c, 1, 0)[:cut], F.shift(c, 0, 1)[cut:]], 0)


def decoder(mode=68, **env):
    """a decoder created under CIMBAR_HIP_<name>=<value> for every keyword. FLOOD_WAVE=0: no certifying pass, so that clean shifts and wipes --
    which it would settle -- reach the pass behind it as well"""
    env = {"CIMBAR_HIP_" + k: str(v) for k, v in env.items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return D.HipDecoder(0, mode)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def clean68(synth):
    return F.clean_frames(synth, 3, seed=123)[1]


@pytest.fixture(scope="module")
def model_frames(clean68):
    c = clean68
    # frame 0 is clean: it must keep path 0. shift(2,1): rounds of more cells than the workgroup has lanes; noise 120: many tiny rounds;
    # rescale(10): drift reaches the +-7 clamp; a wipe; a tear; noise over a rescale
    return np.ascontiguousarray(np.stack([
        c[2], F.shift(c[0], 2, 1), F.add_noise(c[0], 120, 0), F.rescale(c[0], 10), F.blank_region(F.shift(c[1], 1, 1), 300, 500, 200, 700, value=128),
        tear(c[1], 500), F.add_noise(F.rescale(c[1], 5), 60, 1)]))


@pytest.fixture(scope="module")
def default_outputs(model_frames):
    dec = D.HipDecoder(0)
    out = all_outputs(dec, model_frames)
    dec.close()
    return out


def all_outputs(dec, frames, color_correction=2):
    n = len(frames)
    dec.reset_ccm()
    total, chunks, masks = dec.decode_batch(frames, color_correction=color_correction)
    taps = {t: dec.tap(t, n) for t in (D.TAP_BITPLANE, D.TAP_SYMBOLS, D.TAP_COLORS, D.TAP_DRIFT, D.TAP_RS_OK, D.TAP_FLOOD, D.TAP_CCM, D.TAP_FLOOD_PATH,
                                      D.TAP_FLOOD_INFO, D.TAP_FLOOD_ROUNDS)}
    return total, chunks.copy(), masks.copy(), taps


def assert_same(a, b):
    """two all_outputs() results agree in every output and tap (the drift of a frame that never left the parallel path is never written)"""
    assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    for t in a[3]:
        x, y = a[3][t], b[3][t]
        if t == D.TAP_DRIFT:
            flooded = a[3][D.TAP_FLOOD_PATH] != 0
            x, y = x[flooded], y[flooded]
        if t == D.TAP_FLOOD_INFO:
            # where the certifying pass declines a frame, the rule that fired first and the cells decoded by then depend on the order in which its
            # lanes queued cells (two default contexts differ there too): what is compared is whether it certified, and the words of the frames it did
            assert ((x & 0xFF) == 0).tolist() == ((y & 0xFF) == 0).tolist()
            keep = ((x & 0xFF) == 0) | (x == 0xFFFFFFFF)
            x, y = x[keep], y[keep]
        assert x.tobytes() == y.tobytes(), t


def check_against_model(dec, frames, mode, threshold, default=None):
    n = len(frames)
    ncells = dec.geo.NCELLS
    dec.set_relaxed_flood(threshold, fallback=False)
    assert dec.get_relaxed_flood() == (True, threshold, False)
    total, chunks, masks, taps = all_outputs(dec, frames)
    path, info = taps[D.TAP_FLOOD_PATH], taps[D.TAP_FLOOD_ROUNDS]
    flooded = 0
    for k in range(n):
        if path[k] in (0, 2):          # exact in the parallel pass, or certified: the relaxed flood never saw the frame
            assert info[k] == 0
            if default is not None:
                assert (taps[D.TAP_SYMBOLS][k] == default[3][D.TAP_SYMBOLS][k]).all() and masks[k] == default[2][k] and (chunks[k] == default[1][k]).all(), k
            continue
        assert path[k] == 3, (k, path[k])
        flooded += 1
        sym, drift, rounds, dist = M.relaxed_flood(taps[D.TAP_BITPLANE][k], mode, threshold)
        print(f"mode {mode} threshold {threshold} frame {k}: {rounds} rounds (device {info[k] & 0xFFFF}), {int((taps[D.TAP_SYMBOLS][k] != sym).sum())} symbols differ")
        assert (dist >= 0).all()
        assert (taps[D.TAP_SYMBOLS][k] == sym).all(), f"frame {k}: {(taps[D.TAP_SYMBOLS][k] != sym).sum()} symbols differ from the model"
        assert (taps[D.TAP_DRIFT][k] == drift).all(), f"frame {k}: {(taps[D.TAP_DRIFT][k] != drift).any(1).sum()} cells' drift differs from the model"
        assert info[k] & 0xFFFF == rounds and info[k] >> 16 == ncells, (k, hex(info[k]), rounds)
    st = dec.relaxed_flood_stats()
    assert st[0] == flooded and st[2] == 0 and st[3] == int((info & 0xFFFF).sum()), st
    assert st[1] == sum(1 for k in range(n) if path[k] == 3 and taps[D.TAP_RS_OK][k, :dec.geo.SYM_BLOCKS].all()), st
    return path


@pytest.mark.parametrize("threshold", [0, 12, 32])
def test_device_equals_the_model(model_frames, default_outputs, threshold):
    dec = decoder(FLOOD_WAVE=0)
    path = check_against_model(dec, model_frames, 68, threshold, default_outputs)
    dec.close()
    assert path[0] == 0, "the clean frame stays on the parallel path"
    assert (path[1:] == 3).all(), f"every other frame takes the rounds ({path})"


@pytest.mark.parametrize("mode", [67, 66])
def test_device_equals_the_model_in_the_smaller_modes(mode):
    synth = framegen.FrameSynth("cpu", mode)
    c = F.clean_frames(synth, 3, seed=600 + mode)[1]
    h = c.shape[1]
    frames = np.ascontiguousarray(np.stack([F.add_noise(F.shift(c[0], 2, 1), 30, 1), F.rescale(c[1], 6), F.add_noise(c[2], 120, 2)]))
    dec = decoder(mode, FLOOD_WAVE=0)
    path = check_against_model(dec, frames, mode, 12)
    dec.close()
    assert (path == 3).all(), path
    assert h == geometry.for_mode(mode).IMG_H


def fallback_frames(clean68):
    c = clean68
    # threshold 32 degrades on shifts and rescales (DESIGN_WIDENING.md "Relaxed flood"): some of these lose symbol blocks, some do not. A frame
    # that falls back (shift(-3,3): 571 wrong cells in the model) comes first, in front of accepted ones (shift(2,1): 35)
    return np.ascontiguousarray(np.stack([
        F.shift(c[0], -3, 3), F.shift(c[0], 2, 1), F.rescale(c[0], 6), F.rescale(c[1], 6), c[2], F.add_noise(F.shift(c[0], 1, -2), 60, 0),
        F.rescale(c[0], 10), F.add_noise(F.rescale(c[1], 5), 60, 1), F.shift(c[1], 2, 1), tear(c[0], 500)]))


def test_fallback_takes_exactly_the_frames_with_a_failing_symbol_block(clean68):
    frames = fallback_frames(clean68)
    n = len(frames)
    d0 = decoder(FLOOD_WAVE=0)
    geo = d0.geo
    want = all_outputs(d0, frames)          # color_correction on: the carry runs from frame to frame
    d0.close()
    dec = decoder(FLOOD_WAVE=0)
    dec.set_relaxed_flood(32, fallback=False)
    off = all_outputs(dec, frames)
    flooded = off[3][D.TAP_FLOOD_PATH] == 3
    failing = flooded & ~off[3][D.TAP_RS_OK][:, :geo.SYM_BLOCKS].all(1)
    print("paths without fallback", off[3][D.TAP_FLOOD_PATH], "failing", failing.astype(int))
    assert failing.any() and (flooded & ~failing).any(), "the case needs frames of both kinds"
    dec.set_relaxed_flood(32, fallback=True)
    assert dec.relaxed_flood_stats() == (0, 0, 0, 0)
    got = all_outputs(dec, frames)
    path = got[3][D.TAP_FLOOD_PATH]
    print("paths with fallback", path)
    assert (path[failing] == 1).all() and (path[flooded & ~failing] == 3).all() and (path[~flooded] == want[3][D.TAP_FLOOD_PATH][~flooded]).all(), path
    assert np.flatnonzero(path == 1)[0] < np.flatnonzero(path == 3)[-1], "a fallen-back frame precedes an accepted one"
    sym_mask = (1 << geo.SYM_BLOCKS // (geo.BLOCKS // geo.CHUNKS_PER_FRAME)) - 1          # the symbol chunks are the first ones
    nsym = bin(sym_mask).count("1")
    for k in range(n):
        same_symbols = (got[3][D.TAP_SYMBOLS][k] == want[3][D.TAP_SYMBOLS][k]).all()
        if path[k] == 1:
            # replayed exactly inside the call: everything is the default context's, byte for byte
            assert same_symbols and (got[3][D.TAP_DRIFT][k] == want[3][D.TAP_DRIFT][k]).all(), k
            assert got[2][k] == want[2][k] and (got[1][k] == want[1][k]).all(), k
        elif path[k] == 3:
            assert got[3][D.TAP_RS_OK][k, :geo.SYM_BLOCKS].all(), k
            for ch in range(nsym):
                if (want[2][k] >> ch) & 1:
                    assert (got[2][k] >> ch) & 1 and (got[1][k, ch] == want[1][k, ch]).all(), (k, ch)
        if same_symbols:
            # the carry is taken after the fallback: a frame whose symbols are the default context's decodes to the default context's chunks
            assert got[2][k] == want[2][k] and (got[1][k] == want[1][k]).all(), k
    st = dec.relaxed_flood_stats()
    assert st[0] == int(flooded.sum()) and st[2] == int(failing.sum()) and st[1] == st[0] - st[2], st
    assert st[3] == int((got[3][D.TAP_FLOOD_ROUNDS] & 0xFFFF).sum())
    dec.close()


def test_a_workgroup_walks_several_frames(clean68):
    c = clean68
    frames = np.ascontiguousarray(np.stack([F.add_noise(c[0], 90, 3), F.rescale(c[1], 6), c[2], F.add_noise(F.shift(c[2], 1, -2), 60, 4), F.rescale(c[0], 4),
                                            F.add_noise(c[1], 120, 5)]))
    outs = []
    for env in ({}, {"ROUNDS_GRID": 2}):
        dec = decoder(**env)
        dec.set_relaxed_flood(12, fallback=False)
        outs.append(all_outputs(dec, frames))
        dec.close()
    a, b = outs
    assert (a[3][D.TAP_FLOOD_PATH] == 3).sum() == 5, a[3][D.TAP_FLOOD_PATH]
    assert_same(a, b)


def test_switched_off_again_it_is_the_default_chain(model_frames, default_outputs):
    dec = D.HipDecoder(0)
    dec.set_relaxed_flood(12, fallback=True)
    dec.decode_batch(model_frames)
    dec.set_relaxed_flood(-1, 0)
    assert dec.get_relaxed_flood() == (False, -1, False)
    got = all_outputs(dec, model_frames)
    dec.close()
    want = default_outputs
    assert_same(got, want)
    assert not (got[3][D.TAP_FLOOD_PATH] == 3).any() and not got[3][D.TAP_FLOOD_ROUNDS].any()


def test_invalid_settings_are_refused():
    dec = D.HipDecoder(0)
    for bad in (33, -2, 1000):
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            dec.set_relaxed_flood(bad)
    assert dec.get_relaxed_flood() == (False, -1, False)
    dec.set_relaxed_flood(32)
    assert dec.get_relaxed_flood() == (True, 32, True)
    dec.close()
    for mode in (4, 8):
        d = D.HipDecoder(0, mode)
        with pytest.raises(D.CimbarHipError, match="EINVAL"):
            d.set_relaxed_flood(12)
        d.set_relaxed_flood(-1)          # off is what they are
        assert d.get_relaxed_flood() == (False, -1, False)
        d.close()


def test_the_pipelined_entry_point_reports_the_same(clean68):
    import torch
    dev = torch.device("cuda", 0)
    c = clean68
    # at threshold 32: a rescale loses symbol blocks and falls back, noise over a shift and a tear are accepted
    frames = np.ascontiguousarray(np.stack([F.rescale(c[1], 6), F.add_noise(F.shift(c[0], 1, -2), 60, 0), c[2], tear(c[0], 500)]))
    n = len(frames)
    dec = D.HipDecoder(0)
    dec.set_relaxed_flood(32, fallback=True)
    want = all_outputs(dec, frames)
    dec.reset_ccm()
    t = torch.from_numpy(frames).to(dev)
    chunks = torch.zeros((n, dec.geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.zeros((n,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    dec.decode_batch_pipelined(t.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), False, 2, st)
    dec.pipeline_wait(st)
    torch.cuda.synchronize()
    assert (dec.tap(D.TAP_FLOOD_PATH, n) == want[3][D.TAP_FLOOD_PATH]).all()
    assert {1, 3} <= set(want[3][D.TAP_FLOOD_PATH].tolist()), want[3][D.TAP_FLOOD_PATH]
    assert (masks.cpu().numpy().astype(np.uint32) == want[2]).all() and (chunks.cpu().numpy().reshape(want[1].shape) == want[1]).all()
    dec.close()


def test_the_capture_path_reports_the_same(synth):
    payload, fr = F.clean_frames(synth, 2, seed=90)
    quads = [((500, 40), (1480, 70), (470, 1030), (1500, 1000)), ((520, 60), (1450, 40), (540, 1010), (1430, 1040))]
    cams = np.ascontiguousarray(np.stack([F.camera_frame(fr[k], quad=quads[k], background=12) for k in range(2)]))
    dec = D.HipDecoder(0)
    status, corners, frames = dec.extract_batch(cams)
    assert (status != 0).all()
    dec.set_relaxed_flood(12, fallback=True)
    want = all_outputs(dec, np.ascontiguousarray(frames))
    dec.reset_ccm()
    total, chunks, masks, st = dec.scan_extract_decode_batch(cams, preprocess=0)
    assert (st == status).all()
    assert (dec.tap(D.TAP_FLOOD_PATH, 2) == want[3][D.TAP_FLOOD_PATH]).all()
    assert (want[3][D.TAP_FLOOD_PATH] != 0).all(), "deskewed captures leave the parallel path"
    assert total == want[0] and (masks == want[2]).all() and (chunks == want[1]).all()
    dec.close()
